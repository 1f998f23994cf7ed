"""What rt_emit_particles costs beside a read of the same voxels (profiles/emit_particles_bench.txt, DESIGN.md "Particle emitters").

    python tools/emit_particles_profile.py                  # every configuration, each under rocprofv3 in a process of its own
    python tools/emit_particles_profile.py RADIUS DENSITY   # one configuration (what the first form runs under the profiler)

One configuration: a sphere of RADIUS round the voxel the view's centre pixel shows in the generated region, DENSITY of 256 of its
occupied voxels kept.  REPS times rt_emit_particles_async into a device ring of 2^20 slots, and REPS times rt_stamp_capture of the
sphere's bounding box — the yardstick: k_stamp_capture reads the same voxels (minefield byte and material word of every voxel of the
box) and is therefore a floor for the read side — in the same process.  The first form runs `rocprofv3 --kernel-trace --stats`
(nothing else traced; the program after `--`) over radii 4, 16 and 64 at densities 256 and 64 and writes the mean duration of the
three emit kernels, their sum, k_stamp_capture's, the ratio, and the time the emit's bytes (64 per brick read, 12 per brick of
scratch written and read, 68 per particle) would take at 6.3 TB/s, the chip's measured streaming rate.  There is no pass/fail bar."""
import csv, glob, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 20
CONFIGS = tuple((r, d) for r in (4, 16, 64) for d in (256, 64))
KERNELS = ("k_emit_count", "k_emit_scan", "k_emit_write", "k_stamp_capture")
STREAM_TBS = 6.3
CAPACITY = 1 << 20


def one(radius, density):
    import numpy as np
    import torch
    from raytrace_amd import abi, render, world
    with render.Context(render.make_config(256, 144, spp=1, depth=2)) as ctx:
        ctx.generate_world(world.DEFAULT_SEED)
        u = render.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 5)
        hit = ctx.pick_pixels(u, np.array([[128, 72]], dtype=np.int32))[0]
        c = np.array(hit["texel"] if hit["kind"] == abi.RT_HIT_SOLID else (128, 128, 128), dtype=np.int64)
        e = render.make_particle_emitters([render.sphere_shape(c + 0.5, radius)], [c + 0.5 - 128.0], speeds=12.0, drifts=(0, 0, 4.0), spreads=3.0,
                                          life_mins=1.0, life_spans=2.0, densities=density, responses=abi.RT_PARTICLE_BOUNCE, seeds=0x5EED)
        lo, hi = np.maximum(c - radius, 0), np.minimum(c + radius, 255)
        ring = torch.zeros((CAPACITY, 64), dtype=torch.uint8, device="cuda")
        cursor = torch.zeros(4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(REPS):
            ctx.emit_particles_async(e, (0, 0, 0), ring, CAPACITY, cursor)
        ctx.sync()
        for _ in range(REPS):
            ctx.stamp_destroy(ctx.stamp_capture(lo, hi - lo + 1))
        ctx.sync()
        cur = cursor.cpu().numpy().view(np.uint32)
    n = (int(cur[1]) + int(cur[2])) // REPS
    bricks = int(np.prod((hi >> 2) - (lo >> 2) + 1))
    print("done radius %d density %d: centre %s, box %s, bricks %d, selected %d" % (radius, density, c.tolist(), (hi - lo + 1).tolist(), bricks, n))


def profile_all(out_path):
    rows = ["# rocprofv3 --kernel-trace --stats, MI355X: %d x rt_emit_particles_async of one sphere and %d x rt_stamp_capture of its bounding" % (REPS, REPS),
            "# box, one process per configuration (tools/emit_particles_profile.py).  Mean durations in us; emit = count + scan + write.",
            "# stream_us: 76 bytes per brick and 68 per particle at %.1f TB/s." % STREAM_TBS,
            "%6s %7s %8s %8s %8s %8s %10s %8s %7s %9s  %s" % ("radius", "density", "selected", "count", "scan", "write", "emit", "capture", "ratio", "stream_us", "")]
    for (radius, density) in CONFIGS:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                   str(radius), str(density)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
            if r.returncode != 0:
                sys.exit("radius %d density %d: rocprofv3 exited with %d\n%s" % (radius, density, r.returncode, r.stderr[-2000:]))
            done = [l for l in r.stdout.splitlines() if l.startswith("done")]
            stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if not stats or not done:
                sys.exit("radius %d density %d: no kernel_stats.csv or no result line" % (radius, density))
            avg = {}
            for rec in csv.DictReader(open(stats[0])):
                col = lambda key: next(v for k, v in rec.items() if k.lower().startswith(key))   # Name, Calls, AverageNs, MinNs, MaxNs
                for k in KERNELS:
                    if k in col("name"):
                        assert int(col("calls")) == REPS, (col("name"), col("calls"))
                        avg[k] = float(col("average")) / 1e3
            words = done[-1].replace(",", "").split()
            bricks, n = int(words[words.index("bricks") + 1]), int(words[words.index("selected") + 1])
            emit = avg["k_emit_count"] + avg["k_emit_scan"] + avg["k_emit_write"]
            rows.append("%6d %7d %8d %8.2f %8.2f %8.2f %10.2f %8.2f %7.2f %9.2f  %s" % (
                radius, density, n, avg["k_emit_count"], avg["k_emit_scan"], avg["k_emit_write"], emit, avg["k_stamp_capture"],
                emit / avg["k_stamp_capture"], (76 * bricks + 68 * n) / (STREAM_TBS * 1e6), done[-1]))
            print(rows[-1], flush=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    if len(sys.argv) >= 3:
        one(int(sys.argv[1]), int(sys.argv[2]))
    else:
        out = sys.argv[1] if len(sys.argv) == 2 else os.path.join(ROOT, "profiles", "emit_particles_bench.txt")
        profile_all(out)
