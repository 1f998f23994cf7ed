"""What rt_step_particles costs beside the sweep it is built on (profiles/step_particles_bench.txt, DESIGN.md "Particle simulation").

    python tools/step_particles_profile.py                 # every configuration, each under rocprofv3 in a process of its own
    python tools/step_particles_profile.py COUNT SWEEPS    # one configuration (what the first form runs under the profiler)

One configuration: COUNT debris particles (cubes of half edge 1/16 scattered 10 to 200 units in front of the camera, a seeded velocity
up to 12 units per second per axis, RT_PARTICLE_BOUNCE, gravity 32, dt 1/60, restitution 1/2, friction 3/4) in device buffers.  REPS
times rt_step_particles_async with SWEEPS sub-sweeps from those states into a second buffer and a draw buffer, and REPS times
rt_sweep_boxes_async — the yardstick: k_sweep, which the parent has — on the same boxes with the tick's motions, in the same process.
The first form runs `rocprofv3 --kernel-trace --stats` (nothing else traced; the program after `--`) over 4096, 100 000 and 2^20
particles at 1 and 3 sub-sweeps and writes the mean duration of k_step_particles and of k_sweep, their ratio, and the time the step's
record bytes (64 read, 96 written per particle) would take at 6.3 TB/s, the chip's measured streaming rate.  There is no pass/fail bar."""
import csv, glob, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 20
CONFIGS = tuple((n, s) for n in (4096, 100000, 1 << 20) for s in (1, 3))
KERNELS = ("k_step_particles", "k_sweep")
STREAM_TBS = 6.3
DT, GRAVITY = 1.0 / 60.0, (0.0, 0.0, -32.0)


def debris(u, n, seed=1):
    """(states, sweeps): n debris particles over the view at log-uniform distances, and their boxes with the first tick's motions."""
    import numpy as np
    from raytrace_amd import abi, render
    rng = np.random.default_rng(seed)
    o, f, r, up = (np.array(v[:], dtype=np.float64) for v in (u.origin, u.forward, u.right, u.up))
    sx, sy = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    v = f[None] + r[None] * sx[:, None] + up[None] * sy[:, None]
    c = (o[None] + v / np.linalg.norm(v, axis=1, keepdims=True) * np.exp(rng.uniform(np.log(10.0), np.log(200.0), n))[:, None]).astype(np.float32)
    half = np.float32(0.0625)
    vel = rng.uniform(-12.0, 12.0, (n, 3)).astype(np.float32)
    states = render.make_particle_states(c - half, c + half, vel, half, abi.RT_PARTICLE_BOUNCE, np.inf, rng.integers(0, 1 << 21, n), np.arange(n) % 64)
    motion = ((vel + np.float32(GRAVITY) * np.float32(DT)) * np.float32(DT)).astype(np.float32)
    return states, render.make_sweeps(np.stack([states["lo"], states["hi"], motion], axis=1))


def one(count, sweeps):
    import numpy as np
    import torch
    from raytrace_amd import abi, render, world
    dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(len(a), -1).copy()).cuda()
    with render.Context(render.make_config(256, 144, spp=1, depth=2)) as ctx:
        ctx.generate_world(world.DEFAULT_SEED)
        u = render.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 5)
        states, as_sweeps = debris(u, count)
        params = render.make_particle_step(DT, GRAVITY, 1.0, 0.5, 0.75, 0.5, (0, 0, 0), sweeps)
        d_in, d_sweeps = dev(states), dev(as_sweeps)
        d_out = torch.zeros((count, 64), dtype=torch.uint8, device="cuda")
        d_draw = torch.zeros((count, 32), dtype=torch.uint8, device="cuda")
        d_hits = torch.zeros((count, 64), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for _ in range(REPS):
            ctx.step_particles_async(params, d_in, d_out, d_draw)
        for _ in range(REPS):
            ctx.sweep_boxes_async(d_sweeps, d_hits)
        ctx.sync()
        out = d_out.cpu().numpy().view(abi.PARTICLE_STATE_DTYPE).reshape(-1)
        hits = d_hits.cpu().numpy().view(render.SWEEP_HIT_DTYPE).reshape(-1)
    print("done %d particles, %d sub-sweeps: %d in contact after the tick, %d of the plain sweeps blocked" % (
        count, sweeps, int(np.count_nonzero(out["flags"] & abi.RT_PSTATE_CONTACT)), int(np.count_nonzero(hits["kind"] == abi.RT_SWEEP_BLOCKED))))


def profile_all(out_path):
    rows = ["# rocprofv3 --kernel-trace --stats, MI355X: %d x rt_step_particles_async on debris (half 1/16, gravity, BOUNCE) and %d x" % (REPS, REPS),
            "# rt_sweep_boxes_async on the same boxes and the tick's motions, one process per configuration (tools/step_particles_profile.py).",
            "# stream_us: the step's record bytes (64 read + 96 written per particle) at %.1f TB/s." % STREAM_TBS,
            "%9s %6s %16s %12s %7s %10s  %s" % ("particles", "sweeps", "k_step_particles", "k_sweep", "ratio", "stream_us", "")]
    for (n, s) in CONFIGS:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), str(n), str(s)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
            if r.returncode != 0:
                sys.exit("%d x %d: rocprofv3 exited with %d\n%s" % (n, s, r.returncode, r.stderr[-2000:]))
            done = [l for l in r.stdout.splitlines() if l.startswith("done")]
            stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if not stats:
                sys.exit("%d x %d: no kernel_stats.csv" % (n, s))
            avg = {}
            for rec in csv.DictReader(open(stats[0])):
                col = lambda key: next(v for k, v in rec.items() if k.lower().startswith(key))   # Name, Calls, AverageNs, MinNs, MaxNs
                for k in KERNELS:
                    if k in col("name"):
                        assert int(col("calls")) == REPS, (col("name"), col("calls"))
                        avg[k] = float(col("average")) / 1e3
            rows.append("%9d %6d %13.2f us %9.2f us %7.2f %10.2f  %s" % (n, s, avg["k_step_particles"], avg["k_sweep"], avg["k_step_particles"] / avg["k_sweep"],
                                                                        n * 160 / (STREAM_TBS * 1e6), done[-1] if done else ""))
            print(rows[-1], flush=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    if len(sys.argv) >= 3:
        one(int(sys.argv[1]), int(sys.argv[2]))
    else:
        out = sys.argv[1] if len(sys.argv) == 2 else os.path.join(ROOT, "profiles", "step_particles_bench.txt")
        profile_all(out)
