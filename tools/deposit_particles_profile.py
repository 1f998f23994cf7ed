"""What rt_deposit_particles costs beside its two floors (profiles/deposit_particles_bench.txt, DESIGN.md "Particle deposits").

    python tools/deposit_particles_profile.py                    # every configuration, each under rocprofv3 in a process of its own
    python tools/deposit_particles_profile.py COUNT BOX MODE     # one configuration (what the first form runs under the profiler)

One configuration: COUNT particles whose centres lie on seeded random unoccupied texels of a box of the generated region — BOX = one
(a chunk), eight (the eight chunks round the view's terrain) or limit (the whole region, 2^24 texels) — all of them candidates (MODE
deposit) or none of them (MODE nothing: no contact bit).  REPS times rt_deposit_particles_async, the region's box put back from a
stamp and the states restored between the calls; and in the same process the two yardsticks: REPS times rt_edit_shapes of one box
shape equal to the deposit box (k_shape_chunks + k_rebuild_chunk_maps: the floor for the world side) and REPS times
rt_step_particles_async on the same states (k_step_particles: the floor for the particle side).  The first form runs `rocprofv3
--kernel-trace --stats` (nothing else traced; the program after `--`) and writes the mean duration of the scratch fill, the claim
pass, the chunk pass and the map rebuild, the yardsticks, and the time the fill's bytes (4 per texel) would take at 6.3 TB/s, the
chip's measured streaming rate.  There is no pass/fail bar."""
import csv, glob, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 10
CONFIGS = ((4096, "one", "deposit"), (4096, "eight", "deposit"), (100000, "one", "deposit"), (100000, "eight", "deposit"), (100000, "limit", "deposit"),
           (1 << 20, "one", "deposit"), (1 << 20, "eight", "deposit"), (1 << 20, "limit", "deposit"), (100000, "eight", "nothing"),
           (1 << 20, "limit", "nothing"))
KERNELS = ("fillBuffer", "k_deposit_claim", "k_deposit_chunks", "k_rebuild_chunk_maps", "k_shape_chunks", "k_step_particles")
STREAM_TBS = 6.3


def one(count, box, mode):
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
        _, mine = ctx.read_box(lo, ext)
        z, y, x = np.nonzero(mine != 0)
        pick = np.random.default_rng(count).integers(0, len(z), size=count)
        v = np.stack([x[pick], y[pick], z[pick]], axis=1) + lo - 128                       # world voxels under lr = 0
        states = np.zeros(count, dtype=abi.PARTICLE_STATE_DTYPE)
        states["lo"], states["hi"] = v + np.float32(0.375), v + np.float32(0.625)
        states["flags"] = abi.RT_PARTICLE_STICK | (0x40000 if mode == "deposit" else 0)
        states["life"], states["half"], states["material"] = 30.0, 0.125, np.arange(count)
        first = torch.from_numpy(states.view(np.uint8).reshape(count, 64).copy()).cuda()
        t_s, t_d, t_c = first.clone(), torch.zeros((count, 32), dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        undo = ctx.stamp_capture(lo, ext)
        p = abi.make_particle_deposit(lo, hi)
        for _ in range(REPS):
            ctx.deposit_particles_async(p, t_s, t_d, t_c)
            ctx.edit_stamps([render.stamp_place(undo, lo)])
            ctx.sync()
            t_s.copy_(first)
            torch.cuda.synchronize()
        shape = render.box_shape(lo, hi, material=0, solid=0, where=abi.RT_WHERE_AIR)
        for _ in range(REPS):
            ctx.edit_shapes([shape])
        step = render.make_particle_step(1.0 / 60.0, accel=(0.0, 0.0, -32.0), sweeps=1)
        for _ in range(REPS):
            ctx.step_particles_async(step, first, t_s, None)
        ctx.sync()
        cnt = t_c.cpu().numpy().view(np.uint32)
    print("done count %d box %s mode %s: lo %s, texels %d, chunks %d, deposited %d, voxels %d" % (
        count, box, mode, lo.tolist(), int(np.prod(ext)), int(np.prod((hi >> 6) - (lo >> 6) + 1)), int(cnt[0]) // REPS, int(cnt[1]) // REPS))


def profile_all(out_path):
    rows = ["# rocprofv3 --kernel-trace --stats, MI355X: %d x rt_deposit_particles_async, %d x rt_edit_shapes of the same box and %d x" % (REPS, REPS, REPS),
            "# rt_step_particles_async on the same states, one process per configuration (tools/deposit_particles_profile.py).  Mean durations",
            "# in us; deposit = fill + claim + chunks + maps; maps is the mean over the deposits', the shapes' and the undo's launches of",
            "# k_rebuild_chunk_maps (the same chunk list).  stream_us: the fill's 4 bytes per texel at %.1f TB/s." % STREAM_TBS,
            "%8s %6s %8s %9s %8s %8s %8s %8s %9s %8s %8s %9s  %s" % ("count", "box", "mode", "voxels", "fill", "claim", "chunks", "maps", "deposit", "shapes",
                                                                "step", "stream_us", "")]
    for (count, box, mode) in CONFIGS:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                   str(count), box, mode]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
            if r.returncode != 0:
                sys.exit("count %d box %s %s: rocprofv3 exited with %d\n%s" % (count, box, mode, r.returncode, r.stderr[-2000:]))
            done = [l for l in r.stdout.splitlines() if l.startswith("done")]
            stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if not stats or not done:
                sys.exit("count %d box %s %s: no kernel_stats.csv or no result line" % (count, box, mode))
            avg = dict.fromkeys(KERNELS, float("nan"))
            for rec in csv.DictReader(open(stats[0])):
                col = lambda key: next(v for k, v in rec.items() if k.lower().startswith(key))   # Name, Calls, AverageNs, MinNs, MaxNs
                for k in KERNELS:
                    if k in col("name"):
                        if k.startswith("k_deposit"):
                            assert int(col("calls")) == REPS, (col("name"), col("calls"))
                        avg[k] = float(col("average")) / 1e3
            words = done[-1].replace(",", "").split()
            texels, voxels = int(words[words.index("texels") + 1]), int(words[words.index("voxels") + 1])
            deposit = avg["fillBuffer"] + avg["k_deposit_claim"] + avg["k_deposit_chunks"] + avg["k_rebuild_chunk_maps"]
            rows.append("%8d %6s %8s %9d %8.2f %8.2f %8.2f %8.2f %9.2f %8.2f %8.2f %9.2f  %s" % (
                count, box, mode, voxels, avg["fillBuffer"], avg["k_deposit_claim"], avg["k_deposit_chunks"], avg["k_rebuild_chunk_maps"], deposit,
                avg["k_shape_chunks"] + avg["k_rebuild_chunk_maps"], avg["k_step_particles"], 4 * texels / (STREAM_TBS * 1e6), done[-1]))
            print(rows[-1], flush=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    if len(sys.argv) >= 4:
        one(int(sys.argv[1]), sys.argv[2], sys.argv[3])
    else:
        out = sys.argv[1] if len(sys.argv) == 2 else os.path.join(ROOT, "profiles", "deposit_particles_bench.txt")
        profile_all(out)
