"""What a navigation field's build and sample cost per kernel (profiles/nav_field_bench.txt, DESIGN.md "Navigation fields").

    python tools/nav_field_profile.py                  # every configuration, each under rocprofv3 in a process of its own
    python tools/nav_field_profile.py EXTENT LEVELS    # one configuration (what the first form runs under the profiler)

One configuration: a field of EXTENT x EXTENT x 128 cells of the generated region round the terrain the view looks at, that texel's
column the goal, max_dist 2 EXTENT, built REPS times with LEVELS levels per launch (RT_NAV_LEVELS: 1, 4 or 8), and AGENTS agents
sampled after every build.  The first form runs `rocprofv3 --kernel-trace --stats` (nothing else traced; the program after `--`)
and writes the mean duration of the seed, stand, goals, level, moves and sample launches, the level launches per build and their
sum, and the time the build's bytes would take at 6.3 TB/s, the chip's measured streaming rate: per cell one minefield byte read
and three field bytes written by the fill, per level launch that runs three bitmaps read and two written.  There is no pass/fail
bar."""
import csv, glob, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 10
AGENTS = 100000
CONFIGS = tuple((extent, levels) for extent in (64, 192) for levels in (1, 4, 8))
KERNELS = ("k_nav_seed", "k_nav_stand", "k_nav_goals", "k_nav_levels", "k_nav_moves", "k_nav_sample")
STREAM_TBS = 6.3


def one(extent, levels):
    os.environ["RT_NAV_LEVELS"] = str(levels)
    import numpy as np
    import torch
    from raytrace_amd import abi, render, world
    with render.Context(render.make_config(256, 144, spp=1, depth=2)) as ctx:
        ctx.generate_world(world.DEFAULT_SEED)
        u = render.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 5)
        hit = ctx.pick_pixels(u, np.array([[128, 72]], dtype=np.int32))[0]
        c = np.array(hit["texel"] if hit["kind"] == abi.RT_HIT_SOLID else (128, 128, 128), dtype=np.int64)
        ext = np.array((extent, extent, 128))
        lo = np.clip(c - ext // 2, 0, 256 - ext)
        p = abi.make_nav_build(lo, 2 * extent, goal_snap=8)
        goals = abi.make_nav_goals([(c[0], c[1], lo[2] + min(z, 127)) for z in range(8, 136, 9)])
        rng = np.random.default_rng(1)
        agents = abi.make_nav_agents(lo + rng.random((AGENTS, 3)) * ext, 8, 2)
        t_g, t_a = (torch.from_numpy(a.view(np.uint8).copy()).cuda() for a in (goals, agents))
        t_r = torch.zeros(32, dtype=torch.uint8, device="cuda")
        t_s = torch.zeros((AGENTS, 32), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        f = ctx.nav_create(ext)
        for _ in range(REPS):
            ctx.nav_build_async(f, p, t_g, t_r)
            ctx.nav_sample_async(f, t_a, t_s)
            ctx.sync()
        res = t_r.cpu().numpy().view(abi.NAV_RESULT_DTYPE)[0]
        found = int((t_s.cpu().numpy().view(abi.NAV_STEP_DTYPE)["dist"] != 0xFFFFFFFF).sum())
        ctx.nav_destroy(f)
    print("done extent %d levels %d: lo %s, cells %d, standable %d, reached %d, depth %d, truncated %d, agents %d, found %d" % (
        extent, levels, lo.tolist(), int(np.prod(ext)), int(res["standable"]) // REPS, int(res["reached"]) // REPS, int(res["levels"]),
        int(res["truncated"]) // REPS, AGENTS, found))


def profile_all(out_path):
    rows = ["# rocprofv3 --kernel-trace --stats, MI355X: %d x (rt_nav_build_async, rt_nav_sample_async of %d agents), one process per" % (REPS, AGENTS),
            "# configuration (tools/nav_field_profile.py).  Mean durations in us; levels is the mean over all launches of a build, those after",
            "# the frontier's end included, launches their number per build, levels_sum their sum; build = seed + stand + goals + levels_sum +",
            "# moves.  stream_us: the build's bytes at %.1f TB/s." % STREAM_TBS,
            "%6s %2s %9s %6s %8s %8s %8s %8s %8s %10s %8s %9s %8s %9s  %s" % ("extent", "G", "reached", "depth", "seed", "stand", "goals", "levels", "launches",
                                                                         "levels_sum", "moves", "build", "sample", "stream_us", "")]
    for (extent, levels) in CONFIGS:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), str(extent),
                   str(levels)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
            if r.returncode != 0:
                sys.exit("extent %d levels %d: rocprofv3 exited with %d\n%s" % (extent, levels, r.returncode, r.stderr[-2000:]))
            done = [l for l in r.stdout.splitlines() if l.startswith("done")]
            stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if not stats or not done:
                sys.exit("extent %d levels %d: no kernel_stats.csv or no result line" % (extent, levels))
            avg = dict.fromkeys(KERNELS, float("nan"))
            for rec in csv.DictReader(open(stats[0])):
                col = lambda key: next(v for k, v in rec.items() if k.lower().startswith(key))   # Name, Calls, AverageNs, MinNs, MaxNs
                for k in KERNELS:
                    if k in col("name"):
                        avg[k] = float(col("average")) / 1e3
            words = done[-1].replace(",", "").split()
            cells, reached, depth = (int(words[words.index(k) + 1]) for k in ("cells", "reached", "depth"))
            launches = -(-(2 * extent + 1) // levels)
            ran = min(launches, depth // levels + 1)
            bitmap = extent * 128 * 2 * ((-(-extent // 16) + 1) // 2 * 2)
            moved = 4 * cells + ran * 5 * bitmap
            levels_sum = avg["k_nav_levels"] * launches
            build = avg["k_nav_seed"] + avg["k_nav_stand"] + avg["k_nav_goals"] + levels_sum + avg["k_nav_moves"]
            rows.append("%6d %2d %9d %6d %8.2f %8.2f %8.2f %8.2f %8d %10.2f %8.2f %9.2f %8.2f %9.2f  %s" % (
                extent, levels, reached, depth, avg["k_nav_seed"], avg["k_nav_stand"], avg["k_nav_goals"], avg["k_nav_levels"], launches, levels_sum,
                avg["k_nav_moves"], build, avg["k_nav_sample"], moved / (STREAM_TBS * 1e6), done[-1]))
            print(rows[-1], flush=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    if len(sys.argv) >= 3:
        one(int(sys.argv[1]), int(sys.argv[2]))
    else:
        out = sys.argv[1] if len(sys.argv) == 2 else os.path.join(ROOT, "profiles", "nav_field_bench.txt")
        profile_all(out)
