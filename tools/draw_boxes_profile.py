"""What rt_draw_boxes costs beside the post passes of the same frame (profiles/draw_boxes_kernel_stats.txt, DESIGN.md "Entity boxes").

    python tools/draw_boxes_profile.py                      # every configuration, each under rocprofv3 in a process of its own
    python tools/draw_boxes_profile.py WIDTH HEIGHT COUNT   # one configuration (what the first form runs under the profiler)

One configuration: FRAMES one-sample frames, each followed by rt_draw_boxes_async of COUNT scattered entity-sized boxes (0 = one box
hidden behind the camera, so that the launch still happens), rt_denoise and rt_finalize.  The first form runs `rocprofv3 --kernel-trace
--stats` over each of 1920x1080 and 1024x1024 with 0, 64, 256, 1024 and 4096 boxes and writes, per configuration, the average, minimum
and maximum duration of k_draw_boxes, of the seven denoise launches and of k_finalize.  There is no pass/fail bar."""
import csv, glob, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 40
SHAPES = ((1920, 1080), (1024, 1024))
COUNTS = (0, 64, 256, 1024, 4096)


def scatter(u, n, seed=1):
    """n player-sized boxes (0.6 x 0.6 x 1.8) over the view, 20 to 400 units away (log-uniform)."""
    import numpy as np
    from raytrace_amd import render
    rng = np.random.default_rng(seed)
    o, f, r, up = (np.array(v[:], dtype=np.float64) for v in (u.origin, u.forward, u.right, u.up))
    if n == 0:
        c = (o - 50.0 * f)[None]
    else:
        sx, sy = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
        v = f[None] + r[None] * sx[:, None] + up[None] * sy[:, None]
        c = o[None] + v / np.linalg.norm(v, axis=1, keepdims=True) * np.exp(rng.uniform(np.log(20.0), np.log(400.0), n))[:, None]
    half = np.array([0.3, 0.3, 0.9])
    return render.make_draw_boxes(c - half, c + half, rng.integers(0, 1 << 21, len(c)))


def one(width, height, count):
    import numpy as np
    import torch
    from raytrace_amd import abi, render, world
    noise = np.fromfile(os.path.join(ROOT, "tests", "golden", "blue_noise_512.rgba"), dtype=np.uint8)
    with render.Context(render.make_config(width, height, spp=1, depth=2, flags=abi.RT_FLAG_CACHE_PRIMARY)) as ctx:
        ctx.generate_world(world.DEFAULT_SEED)
        ctx.upload_noise(noise)
        u = render.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 5)
        boxes = scatter(u, count)
        lights = ctx.probe_records(u, render.face_probes(boxes), 4, 2)
        d_boxes = torch.from_numpy(boxes.view(np.uint8).reshape(len(boxes), -1).copy()).cuda()
        d_lights = torch.from_numpy(lights.view(np.uint8).reshape(len(lights), -1).copy()).cuda()
        torch.cuda.synchronize()
        ctx.draw_frame(u)
        before = ctx.readback(abi.RT_BUF_DEPTH_F32)
        for k in range(FRAMES):
            u.seed = 5 + k
            ctx.draw_frame(u)
            ctx.draw_boxes_async(u, d_boxes, d_lights)
            if k == 0:
                drawn = int(np.count_nonzero(ctx.readback(abi.RT_BUF_DEPTH_F32) != before))
            ctx.denoise(True)
            ctx.finalize()
        ctx.sync()
    print("done %dx%d %d boxes, %d pixels drawn" % (width, height, count, drawn))


def profile_all(out_path):
    rows = ["# rocprofv3 --kernel-trace --stats, MI355X: %d one-sample frames, each followed by rt_draw_boxes_async, rt_denoise and rt_finalize" % FRAMES,
            "# (tools/draw_boxes_profile.py; one process per configuration).  Boxes: player-sized (0.6 x 0.6 x 1.8), scattered over the view 20 to 400",
            "# units away; \"0\" launches with one box hidden behind the camera."]
    for (w, h) in SHAPES:
        for n in COUNTS:
            tag = "%dx%d_%d" % (w, h, n)
            with tempfile.TemporaryDirectory() as tmp:
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                       str(w), str(h), str(n)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
                if r.returncode != 0:
                    sys.exit("%s: rocprofv3 exited with %d\n%s" % (tag, r.returncode, r.stderr[-2000:]))
                done = [l for l in r.stdout.splitlines() if l.startswith("done")]
                stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
                if not stats:
                    sys.exit("%s: no kernel_stats.csv" % tag)
                post = 0.0
                for rec in csv.DictReader(open(stats[0])):
                    col = lambda key: next(v for k, v in rec.items() if k.lower().startswith(key))   # Name, Calls, AverageNs, MinNs, MaxNs
                    name = col("name")
                    if not any(k in name for k in ("k_draw_boxes", "k_denoise", "k_finalize")):
                        continue
                    calls, avg = int(col("calls")), float(col("average")) / 1e3
                    rows.append("%-16s %-64s calls %4d avg_us %8.2f min_us %8.2f max_us %8.2f" % (
                        tag, name[:64], calls, avg, float(col("min")) / 1e3, float(col("max")) / 1e3))
                    if "k_denoise" in name:
                        post += calls * avg / FRAMES
                rows.append("%-16s denoise total per frame (%d frames): %.2f us; %s" % (tag, FRAMES, post, done[-1] if done else ""))
                print(rows[-1], flush=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    if len(sys.argv) >= 4:
        one(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]))
    else:
        out = sys.argv[1] if len(sys.argv) == 2 else os.path.join(ROOT, "profiles", "draw_boxes_kernel_stats.txt")
        profile_all(out)
