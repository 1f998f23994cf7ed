"""What rt_detach_voxels costs beside its floor (profiles/detach_voxels_bench.txt, DESIGN.md "Voxel detachment").

    python tools/detach_voxels_profile.py                  # every configuration, each under rocprofv3 in a process of its own
    python tools/detach_voxels_profile.py BOX MODE         # one configuration (what the first form runs under the profiler)

One configuration: a box of the generated region — BOX = one (a chunk), eight (the eight chunks round the view's terrain) or limit
(the whole region, 256^3 texels) — with every face but the top anchoring.  MODE nothing: the terrain as generated; nothing detaches.
MODE small: a block of 12 x 12 texels' footprint under the view's terrain is cut loose by a slab and four trenches.  MODE half: a slab
four texels thick is carved through the whole region at the box's middle height and only the low z face anchors: what lies over it,
about half the box, detaches.  REPS times rt_detach_voxels_async with RT_DETACH_CARVE | RT_DETACH_CAPTURE and max_passes = PASSES, the
stamp destroyed and the box put back from a stamp between the calls.  The first form runs `rocprofv3 --kernel-trace --stats` (nothing
else traced; the program after `--`) and writes the mean duration of the seed, reach, apply, chunk and map launches, the reach
launches' sum per call (PASSES launches, those after the end included), and the time the call's bytes would take at 6.3 TB/s, the
chip's measured streaming rate: 1 minefield byte per texel for the seed, 5 stamp bytes per texel for the apply, and per chunk 64 KiB
written by the seed, 96 KiB moved by each reach pass that runs and 64 KiB read by the apply.  There is no pass/fail bar."""
import csv, glob, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 10
PASSES = 16
CONFIGS = tuple((box, mode) for box in ("one", "eight", "limit") for mode in ("nothing", "small", "half"))
KERNELS = ("k_detach_seed", "k_detach_reach", "k_detach_apply", "k_detach_chunks", "k_rebuild_chunk_maps")
STREAM_TBS = 6.3


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
        faces = 0x1F
        if mode == "small":
            f0 = np.clip(c[:2] - 6, lo[:2] + 4, hi[:2] - 16)
            f1 = f0 + 11
            z0, z1 = int(max(c[2] - 12, lo[2] + 4)), int(hi[2])
            cut = lambda a, b: render.box_shape((a[0], a[1], z0 - 3), (b[0], b[1], z1), material=0, solid=0)
            ctx.edit_shapes([render.box_shape((f0[0] - 2, f0[1] - 2, z0 - 3), (f1[0] + 2, f1[1] + 2, z0), material=0, solid=0),
                             cut((f0[0] - 2, f0[1] - 2), (f0[0] - 1, f1[1] + 2)), cut((f1[0] + 1, f0[1] - 2), (f1[0] + 2, f1[1] + 2)),
                             cut((f0[0] - 2, f0[1] - 2), (f1[0] + 2, f0[1] - 1)), cut((f0[0] - 2, f1[1] + 1), (f1[0] + 2, f1[1] + 2))])
        elif mode == "half":
            z1 = int((lo[2] + hi[2]) // 2)
            ctx.edit_shapes([render.box_shape((0, 0, z1 - 3), (255, 255, z1), material=0, solid=0)])
            faces = 0x10
        p = abi.make_voxel_detach(lo, hi, anchor_faces=faces, max_passes=PASSES)
        res0 = render.detach_result()
        t_r = torch.from_numpy(res0.view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        undo = ctx.stamp_capture(lo, ext)
        for _ in range(REPS):
            body = ctx.detach_voxels_async(p, t_r)
            ctx.stamp_destroy(body)
            ctx.edit_stamps([render.stamp_place(undo, lo)])
            ctx.sync()
        res = t_r.cpu().numpy().view(abi.DETACH_RESULT_DTYPE)[0]
    print("done box %s mode %s: lo %s, texels %d, chunks %d, detached %d, supported %d, passes %d, unconverged %d, dirty %d" % (
        box, mode, lo.tolist(), int(np.prod(ext)), int(np.prod((hi >> 6) - (lo >> 6) + 1)), int(res["detached"]) // REPS, int(res["supported"]) // REPS,
        int(res["passes"]) // REPS, int(res["unconverged"]), int(res["chunks"]) // REPS))


def profile_all(out_path):
    rows = ["# rocprofv3 --kernel-trace --stats, MI355X: %d x rt_detach_voxels_async (carve and capture, max_passes %d), one process per" % (REPS, PASSES),
            "# configuration (tools/detach_voxels_profile.py).  Mean durations in us; reach is the mean over all %d launches of a call, those" % PASSES,
            "# after the end included, reach_sum their sum per call; detach = seed + reach_sum + apply + chunks + maps; maps is the mean over the",
            "# detaches' and the undo's launches of k_rebuild_chunk_maps (the same chunk list).  stream_us: the call's bytes at %.1f TB/s." % STREAM_TBS,
            "%6s %8s %9s %6s %6s %8s %8s %9s %8s %8s %8s %9s %9s  %s" % ("box", "mode", "detached", "passes", "dirty", "seed", "reach", "reach_sum", "apply",
                                                                      "chunks", "maps", "detach", "stream_us", "")]
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
            texels, chunks, detached, passes, dirty = (int(words[words.index(k) + 1]) for k in ("texels", "chunks", "detached", "passes", "dirty"))
            reach_sum = avg["k_detach_reach"] * PASSES
            detach = avg["k_detach_seed"] + reach_sum + avg["k_detach_apply"] + avg["k_detach_chunks"] + avg["k_rebuild_chunk_maps"]
            moved = 6 * texels + chunks * (65536 + passes * 98304 + 65536)
            rows.append("%6s %8s %9d %6d %6d %8.2f %8.2f %9.2f %8.2f %8.2f %8.2f %9.2f %9.2f  %s" % (
                box, mode, detached, passes, dirty, avg["k_detach_seed"], avg["k_detach_reach"], reach_sum, avg["k_detach_apply"], avg["k_detach_chunks"],
                avg["k_rebuild_chunk_maps"], detach, moved / (STREAM_TBS * 1e6), done[-1]))
            print(rows[-1], flush=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    if len(sys.argv) >= 3:
        one(sys.argv[1], sys.argv[2])
    else:
        out = sys.argv[1] if len(sys.argv) == 2 else os.path.join(ROOT, "profiles", "detach_voxels_bench.txt")
        profile_all(out)
