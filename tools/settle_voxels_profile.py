"""What rt_settle_voxels costs beside its floor (profiles/settle_voxels_bench.txt, DESIGN.md "Voxel settling").

    python tools/settle_voxels_profile.py                  # every configuration, each under rocprofv3 in a process of its own
    python tools/settle_voxels_profile.py BOX MODE         # one configuration (what the first form runs under the profiler)

One configuration: a box of the generated region — BOX = one (a chunk), eight (the eight chunks round the view's terrain) or limit
(the whole region, 2^24 texels) — settled down z.  MODE most: a slab four texels thick is carved through the box under the view's
terrain and every occupied voxel is loose, max_fall 4: whatever lies over the slab falls.  MODE few: 1000 voxels of one word are
sprinkled on unoccupied texels and the mask selects that word alone (the pass fetches the word of every occupied cell).  MODE nothing:
every occupied voxel is loose on a box that an unlimited call has compacted before.  REPS times rt_settle_voxels_async, the box put
back from a stamp between the calls; and in the same process the yardstick: REPS times rt_edit_shapes of one box shape equal to the
box that changes nothing (k_shape_chunks + k_rebuild_chunk_maps: the floor for a call that rebuilds every chunk).  The first form
runs `rocprofv3 --kernel-trace --stats` (nothing else traced; the program after `--`) and writes the mean duration of the flag fill,
the column pass, the chunk pass and the map rebuild, the yardstick, and the time the column pass's minefield bytes (1 per texel)
would take at 6.3 TB/s, the chip's measured streaming rate.  There is no pass/fail bar."""
import csv, glob, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 10
CONFIGS = tuple((box, mode) for box in ("one", "eight", "limit") for mode in ("nothing", "few", "most"))
KERNELS = ("fillBuffer", "k_settle_columns", "k_settle_chunks", "k_rebuild_chunk_maps", "k_shape_chunks")
STREAM_TBS = 6.3
WORD = 0xD1CE0001


def one(box, mode):
    import numpy as np
    import torch
    from raytrace_amd import abi, render, world
    with render.Context(render.make_config(256, 144, spp=1, depth=2)) as ctx:
        ctx.generate_world(world.DEFAULT_SEED)
        u = render.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 5)
        hit = ctx.pick_pixels(u, np.array([[128, 72]], dtype=np.int32))[0]
        c = np.array(hit["texel"] if hit["kind"] == abi.RT_HIT_SOLID else (128, 128, 128), dtype=np.int64)
        if box == "one":
            lo = (c >> 6) << 6
            hi = lo + 63
        elif box == "eight":
            lo = np.clip(((c + 32) >> 6) * 64 - 64, 0, 128)
            hi = lo + 127
        else:
            lo, hi = np.zeros(3, np.int64), np.full(3, 255, np.int64)
        ext = hi - lo + 1
        kw = dict(max_fall=4)
        if mode == "most":
            z1 = int(max(lo[2] + 8, min(c[2] - 8, hi[2] - 8)))
            ctx.edit_shapes([render.box_shape((lo[0], lo[1], z1 - 3), (hi[0], hi[1], z1), material=0, solid=0)])
        elif mode == "few":
            _, mine = ctx.read_box(lo, ext)
            z, y, x = np.nonzero(mine != 0)
            pick = np.random.default_rng(7).choice(len(z), size=1000, replace=False)
            ctx.edit_voxels(np.stack([x[pick], y[pick], z[pick]], axis=1) + lo, np.full(1000, WORD, np.uint32), np.ones(1000, bool))
            kw = dict(max_fall=4, loose_mask=0xFFFFFFFF, loose_value=WORD)
        else:
            ctx.settle_voxels(abi.make_voxel_settle(lo, hi))
        p = abi.make_voxel_settle(lo, hi, **kw)
        t_c = torch.zeros(4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        undo = ctx.stamp_capture(lo, ext)
        for _ in range(REPS):
            ctx.settle_voxels_async(p, t_c)
            ctx.edit_stamps([render.stamp_place(undo, lo)])
            ctx.sync()
        shape = render.box_shape(lo, hi, material=0, solid=0, where=abi.RT_WHERE_AIR)
        for _ in range(REPS):
            ctx.edit_shapes([shape])
        ctx.sync()
        cnt = t_c.cpu().numpy().view(np.uint32)
    print("done box %s mode %s: lo %s, texels %d, chunks %d, moved %d, falling %d, distance %d, dirty %d" % (
        box, mode, lo.tolist(), int(np.prod(ext)), int(np.prod((hi >> 6) - (lo >> 6) + 1)), int(cnt[0]) // REPS, int(cnt[1]) // REPS, int(cnt[2]) // REPS,
        int(cnt[3]) // REPS))


def profile_all(out_path):
    rows = ["# rocprofv3 --kernel-trace --stats, MI355X: %d x rt_settle_voxels_async and %d x rt_edit_shapes of the same box, one process per" % (REPS, REPS),
            "# configuration (tools/settle_voxels_profile.py).  Mean durations in us; settle = fill + columns + chunks + maps; maps is the mean",
            "# over the settles', the shapes' and the undo's launches of k_rebuild_chunk_maps (the same chunk list).  stream_us: the column",
            "# pass's 1 minefield byte per texel at %.1f TB/s." % STREAM_TBS,
            "%6s %8s %9s %6s %8s %8s %8s %8s %9s %8s %9s  %s" % ("box", "mode", "moved", "dirty", "fill", "columns", "chunks", "maps", "settle", "shapes", "stream_us", "")]
    for (box, mode) in CONFIGS:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), box, mode]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
            if r.returncode != 0:
                sys.exit("box %s %s: rocprofv3 exited with %d\n%s" % (box, mode, r.returncode, r.stderr[-2000:]))
            done = [l for l in r.stdout.splitlines() if l.startswith("done")]
            stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if not stats or not done:
                sys.exit("box %s %s: no kernel_stats.csv or no result line" % (box, mode))
            avg = dict.fromkeys(KERNELS, float("nan"))
            for rec in csv.DictReader(open(stats[0])):
                col = lambda key: next(v for k, v in rec.items() if k.lower().startswith(key))   # Name, Calls, AverageNs, MinNs, MaxNs
                for k in KERNELS:
                    if k in col("name"):
                        avg[k] = float(col("average")) / 1e3
            words = done[-1].replace(",", "").split()
            texels, moved, dirty = (int(words[words.index(k) + 1]) for k in ("texels", "moved", "dirty"))
            settle = avg["fillBuffer"] + avg["k_settle_columns"] + avg["k_settle_chunks"] + avg["k_rebuild_chunk_maps"]
            rows.append("%6s %8s %9d %6d %8.2f %8.2f %8.2f %8.2f %9.2f %8.2f %9.2f  %s" % (
                box, mode, moved, dirty, avg["fillBuffer"], avg["k_settle_columns"], avg["k_settle_chunks"], avg["k_rebuild_chunk_maps"], settle,
                avg["k_shape_chunks"] + avg["k_rebuild_chunk_maps"], texels / (STREAM_TBS * 1e6), done[-1]))
            print(rows[-1], flush=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    if len(sys.argv) >= 3:
        one(sys.argv[1], sys.argv[2])
    else:
        out = sys.argv[1] if len(sys.argv) == 2 else os.path.join(ROOT, "profiles", "settle_voxels_bench.txt")
        profile_all(out)
