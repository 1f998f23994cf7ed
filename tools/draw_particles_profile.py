"""What rt_draw_particles costs, launch by launch (profiles/draw_particles_kernel_stats.txt, DESIGN.md "Particles").

    python tools/draw_particles_profile.py                          # every configuration, each under rocprofv3 in a process of its own
    python tools/draw_particles_profile.py WIDTH HEIGHT COUNT HALF  # one configuration (what the first form runs under the profiler)

One configuration: FRAMES one-sample frames, each followed by rt_draw_particles_async of COUNT cubes of half edge HALF scattered 10 to
200 units in front of the camera (HALF >= 100: 400 to 8000 units away, so that every cube covers more than 16 tiles and goes to the
wide list), sharing 64 light records.  The first form runs `rocprofv3 --kernel-trace --stats` over 1920x1080 with 4096, 16384, 100000
and 2^20 small cubes and 1000 wide ones and writes, per configuration, the average, minimum and maximum duration of the four particle
kernels.  There is no pass/fail bar."""
import csv, glob, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 20
CONFIGS = ((1920, 1080, 4096, 0.0625), (1920, 1080, 16384, 0.0625), (1920, 1080, 100000, 0.0625), (1920, 1080, 1 << 20, 0.0625),
           (1920, 1080, 1000, 300.0))
KERNELS = ("k_particles_bin", "k_particles_offsets", "k_particles_fill", "k_draw_particles")


def scatter(u, n, half, seed=1, nlights=64):
    """n cubes of half edge `half` over the view at log-uniform distances."""
    import numpy as np
    from raytrace_amd import render
    rng = np.random.default_rng(seed)
    o, f, r, up = (np.array(v[:], dtype=np.float64) for v in (u.origin, u.forward, u.right, u.up))
    near = 400.0 if half >= 100.0 else 10.0
    sx, sy = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    v = f[None] + r[None] * sx[:, None] + up[None] * sy[:, None]
    c = o[None] + v / np.linalg.norm(v, axis=1, keepdims=True) * np.exp(rng.uniform(np.log(near), np.log(20.0 * near), n))[:, None]
    return render.make_particles(c, half, rng.integers(0, 1 << 21, n), np.arange(n) % nlights)


def one(width, height, count, half):
    import numpy as np
    import torch
    from raytrace_amd import abi, render, world
    noise = np.fromfile(os.path.join(ROOT, "tests", "golden", "blue_noise_512.rgba"), dtype=np.uint8)
    with render.Context(render.make_config(width, height, spp=1, depth=2, flags=abi.RT_FLAG_CACHE_PRIMARY)) as ctx:
        ctx.generate_world(world.DEFAULT_SEED)
        ctx.upload_noise(noise)
        u = render.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 5)
        particles = scatter(u, count, half)
        lights = ctx.probe_light(u, particles["center"][:64], np.full(64, abi.RT_PROBE_SPHERE), np.stack([np.arange(64) % 16, np.arange(64) // 16], axis=-1), 4, 2)
        d_particles = torch.from_numpy(particles.view(np.uint8).reshape(len(particles), -1).copy()).cuda()
        d_lights = torch.from_numpy(lights.view(np.uint8).reshape(len(lights), -1).copy()).cuda()
        torch.cuda.synchronize()
        ctx.draw_frame(u)
        before = ctx.readback(abi.RT_BUF_DEPTH_F32)
        for k in range(FRAMES):
            u.seed = 5 + k
            ctx.draw_frame(u)
            ctx.draw_particles_async(u, d_particles, d_lights)
            if k == 0:
                drawn = int(np.count_nonzero(ctx.readback(abi.RT_BUF_DEPTH_F32) != before))
        ctx.sync()
    print("done %dx%d %d particles of half %g, %d pixels drawn" % (width, height, count, half, drawn))


def profile_all(out_path):
    rows = ["# rocprofv3 --kernel-trace --stats, MI355X: %d one-sample frames, each followed by rt_draw_particles_async" % FRAMES,
            "# (tools/draw_particles_profile.py; one process per configuration).  Cubes of the given half edge scattered over the view 10 to 200",
            "# units away (half 300: 400 to 8000 units away, every one on the wide list)."]
    for (w, h, n, half) in CONFIGS:
        tag = "%dx%d_%d_%g" % (w, h, n, half)
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                   str(w), str(h), str(n), str(half)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
            if r.returncode != 0:
                sys.exit("%s: rocprofv3 exited with %d\n%s" % (tag, r.returncode, r.stderr[-2000:]))
            done = [l for l in r.stdout.splitlines() if l.startswith("done")]
            stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if not stats:
                sys.exit("%s: no kernel_stats.csv" % tag)
            total = 0.0
            for rec in csv.DictReader(open(stats[0])):
                col = lambda key: next(v for k, v in rec.items() if k.lower().startswith(key))   # Name, Calls, AverageNs, MinNs, MaxNs
                name = col("name")
                if not any(k in name for k in KERNELS):
                    continue
                calls, avg = int(col("calls")), float(col("average")) / 1e3
                rows.append("%-24s %-48s calls %4d avg_us %9.2f min_us %9.2f max_us %9.2f" % (
                    tag, name[:48], calls, avg, float(col("min")) / 1e3, float(col("max")) / 1e3))
                total += calls * avg / FRAMES
            rows.append("%-24s the four kernels per call (%d calls): %.2f us; %s" % (tag, FRAMES, total, done[-1] if done else ""))
            print(rows[-1], flush=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    if len(sys.argv) >= 5:
        one(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4]))
    else:
        out = sys.argv[1] if len(sys.argv) == 2 else os.path.join(ROOT, "profiles", "draw_particles_kernel_stats.txt")
        profile_all(out)
