"""What rt_flow_voxels costs, kernel by kernel and for 1, 2, 4 and 8 ticks per launch (profiles/flow_voxels_bench.txt, DESIGN.md "Fluid
flow").

    python tools/flow_voxels_profile.py                    # every configuration, each under rocprofv3 in a process of its own
    python tools/flow_voxels_profile.py BOX SCENE G        # one configuration (what the first form runs under the profiler)

One configuration: a box of the generated region round the view's terrain, its top layer eight texels over the highest voxel of its
footprint — BOX = one (64^3), eight (128^3) or limit (256 x 256 x 128, half the region) —, a SCENE and G, the ticks per launch
(RT_FLOW_TICKS, read when the context first plans a flow call).  dry: no voxel passes the fluid test, so every tile is copied through.
front: a row of sources along one top edge of the box (rt_edit_voxels); the timed calls are the REPS calls of TICKS ticks behind one
warm-up call, while the front falls and spreads.  fixed: the same, advanced until a call adds 0 to `active`; the timed calls change nothing, so a call's
first tick launch runs and the workgroups of the others return at once.  The process generates the world, prepares the scene and makes
a warm-up call and REPS calls of rt_flow_voxels_async.  The first form runs `rocprofv3 --kernel-trace --stats` (nothing else traced, no counters; the
program after `--`), every configuration in a process of its own so that none runs behind another's warm-up, takes the timed calls'
dispatches out of the trace by their order (the scene's preparation launches the same kernels, so the means of --stats would mix them
in), and writes per call the mean duration of the seed launch, of all tick launches together, of the apply launch, the chunk pass and
the map rebuild, beside the time one tick launch's state bytes (1 read and 1 written per cell) would take at 6.3 TB/s, the chip's
measured streaming rate.  There is no pass/fail bar."""
import csv, glob, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, TICKS = 10, 8
GROUPS = (1, 2, 4, 8)
CONFIGS = tuple((box, scene, g) for box in ("one", "eight", "limit") for scene in ("dry", "front", "fixed") for g in GROUPS)
STREAM_TBS = 6.3
WORD, MASK = 0x40A0E0C0, 0xFFFFFFF0


def one(box, scene, g):
    import numpy as np
    import torch
    from raytrace_amd import abi, render, world
    os.environ["RT_FLOW_TICKS"] = str(g)
    with render.Context(render.make_config(256, 144, spp=1, depth=2)) as ctx:
        ctx.generate_world(world.DEFAULT_SEED)
        u = render.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 5)
        hit = ctx.pick_pixels(u, np.array([[128, 72]], dtype=np.int32))[0]
        c = np.array(hit["texel"] if hit["kind"] == abi.RT_HIT_SOLID else (128, 128, 128), dtype=np.int64)
        e = {"one": (64, 64, 64), "eight": (128, 128, 128), "limit": (256, 256, 128)}[box]
        lo = np.array([min(max(int(c[0]) - e[0] // 2, 0), 256 - e[0]), min(max(int(c[1]) - e[1] // 2, 0), 256 - e[1]), 0], dtype=np.int64)
        _, column = ctx.read_box((lo[0], lo[1], 0), (e[0], e[1], 256))
        top = int(np.nonzero((column == 0).any(axis=(1, 2)))[0].max())              # the springs stand eight texels over the highest voxel
        lo[2] = min(max(top + 8 - (e[2] - 1), 0), 256 - e[2])
        hi = lo + np.array(e) - 1
        ext = hi - lo + 1
        pre = 0
        if scene != "dry":
            n = int(ext[1])
            xyz = np.stack([np.full(n, lo[0]), lo[1] + np.arange(n), np.full(n, hi[2])], axis=1)
            ctx.edit_voxels(xyz, np.full(n, WORD | 0xF, np.uint32), np.ones(n, bool))
        if scene == "fixed":
            p256 = abi.make_voxel_flow(lo, hi, MASK, WORD, ticks=256)
            while pre < 16:
                pre += 1
                if int(ctx.flow_voxels(p256)["active"]) == 0:
                    break
        pre_launches = pre * -(-256 // g)
        p = abi.make_voxel_flow(lo, hi, MASK, WORD, ticks=TICKS)
        ctx.flow_voxels(p)                                                          # the warm-up call: not timed
        pre, pre_launches = pre + 1, pre_launches + -(-TICKS // g)
        t_c = torch.zeros(8, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(REPS):
            ctx.flow_voxels_async(p, t_c)
        ctx.sync()
        cnt = t_c.cpu().numpy().view(np.uint32)
    print("done G %d box %s scene %s: lo %s, cells %d, chunks %d, pre %d, pre_launches %d, edits %d, wetted %d, changed %d, active %d, dirty %d" % (
        g, box, scene, lo.tolist(), int(np.prod(ext)), int(np.prod((hi >> 6) - (lo >> 6) + 1)), pre, pre_launches, int(scene != "dry"), int(cnt[0]), int(cnt[2]),
        int(cnt[3]), int(cnt[4])), flush=True)


def timed(rows, name, skip, take, per_call=1):
    """Mean microseconds per call of kernel `name` over the `take` calls behind the first `skip` (per_call dispatches each), and the
    dispatches left."""
    mine = [r for r in rows if name in r[0]]
    sel = mine[skip * per_call:(skip + take) * per_call]
    return (sum(r[2] - r[1] for r in sel) / 1e3 / take if len(sel) == take * per_call else float("nan")), mine[(skip + take) * per_call:]


def profile_all(out_path):
    out = ["# rocprofv3 --kernel-trace --stats, MI355X: a warm-up call, then %d x rt_flow_voxels_async of %d ticks; one process per box, scene and G" % (REPS, TICKS),
           "# (tools/flow_voxels_profile.py).  Mean durations in us per call; ticks = all of a call's tick launches together, launches =",
           "# how many; call = seed + ticks + apply + chunks + maps.  stream_us: one tick launch's state bytes (2 per cell) at %.1f TB/s." % STREAM_TBS,
           "%6s %6s %2s %9s %8s %8s %9s %8s %8s %8s %9s %9s  %s" % ("box", "scene", "G", "cells", "seed", "launches", "ticks", "apply", "chunks", "maps", "call", "stream_us", "")]
    for (box, scene, g) in CONFIGS:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), box, scene, str(g)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
            if r.returncode != 0:
                sys.exit("box %s %s G %d: rocprofv3 exited with %d\n%s" % (box, scene, g, r.returncode, r.stderr[-2000:]))
            done = [l for l in r.stdout.splitlines() if l.startswith("done")]
            trace = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
            if not trace or not done:
                sys.exit("box %s %s G %d: no kernel_trace.csv or no result line" % (box, scene, g))
            rows = []
            for rec in csv.DictReader(open(trace[0])):
                col = lambda key: next(v for k, v in rec.items() if key in k.lower())
                rows.append((col("kernel_name"), int(col("start")), int(col("end"))))
            rows.sort(key=lambda t: t[1])
            line = done[-1]
            words = line.replace(",", "").split()
            cells, pre, pre_launches, edits = (int(words[words.index(k) + 1]) for k in ("cells", "pre", "pre_launches", "edits"))
            launches = -(-TICKS // g)
            us = {k: timed(rows, k, pre + (edits if k == "k_rebuild_chunk_maps" else 0), REPS)[0]
                  for k in ("k_flow_seed", "k_flow_apply", "k_flow_chunks", "k_rebuild_chunk_maps")}
            mine = [t for t in rows if "k_flow_ticks<%d>" % g in t[0]][pre_launches:]
            ticks = sum(t[2] - t[1] for t in mine) / 1e3 / REPS if len(mine) == launches * REPS else float("nan")
            call = us["k_flow_seed"] + ticks + us["k_flow_apply"] + us["k_flow_chunks"] + us["k_rebuild_chunk_maps"]
            out.append("%6s %6s %2d %9d %8.2f %8d %9.2f %8.2f %8.2f %8.2f %9.2f %9.2f  %s" % (
                box, scene, g, cells, us["k_flow_seed"], launches, ticks, us["k_flow_apply"], us["k_flow_chunks"], us["k_rebuild_chunk_maps"], call,
                2 * cells / (STREAM_TBS * 1e6), line))
            print(out[-1], flush=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    if len(sys.argv) >= 4:
        one(sys.argv[1], sys.argv[2], int(sys.argv[3]))
    else:
        out = sys.argv[1] if len(sys.argv) == 2 else os.path.join(ROOT, "profiles", "flow_voxels_bench.txt")
        profile_all(out)
