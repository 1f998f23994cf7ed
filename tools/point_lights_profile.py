"""What rt_add_lights costs beside the entity boxes and the post passes of the same frame (profiles/point_lights_kernel_stats.txt,
DESIGN.md "Point lights").

    python tools/point_lights_profile.py                      # every configuration, each under rocprofv3 in a process of its own
    python tools/point_lights_profile.py WIDTH HEIGHT COUNT   # one configuration (what the first form runs under the profiler)

One configuration: FRAMES one-sample frames, each followed by rt_draw_boxes_async of 256 scattered entity-sized boxes,
rt_add_lights_async of COUNT lights of radius 8 scattered just off the visible surfaces (0 = one light behind the camera that reaches
nothing, so that the launch still happens), rt_denoise and rt_finalize.  The first form runs `rocprofv3 --kernel-trace --stats` over
each of 1920x1080 and 1024x1024 with 0, 16, 256 and 1024 lights and writes, per configuration, the average, minimum and maximum
duration of k_add_lights, k_draw_boxes, the seven denoise launches and k_finalize.  Each configuration also restates the kernel's cull
on the host (float64: a statistic, not a check) and reports the mean number of candidates per tile that has a surface pixel and, over
the first 64 lights, the mean number of lanes that pass the exact test (and so trace) per candidate.  There is no pass/fail bar."""
import csv, glob, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 40
SHAPES = ((1920, 1080), (1024, 1024))
COUNTS = (0, 16, 256, 1024)
RADIUS = 8.0


def surface_points(planes, u, width, height):
    """(surface[H, W], P'[H, W, 3], axis, sign) in float64."""
    import numpy as np
    o, f, r, up = (np.array(v[:], dtype=np.float64) for v in (u.origin, u.forward, u.right, u.up))
    sx = np.arange(width) / width * 2.0 - 1.0
    sy = np.arange(height) / height * 2.0 - 1.0
    v = f[None, None] + r[None, None] * sx[None, :, None] + up[None, None] * sy[:, None, None]
    d = v / np.linalg.norm(v, axis=-1, keepdims=True)
    normal, depth = planes["normal_r8"].astype(np.int64), planes["depth_f32"].astype(np.float64)
    surface = (normal < 6) & (depth < 65535.0)
    P = o[None, None] + d * (depth / 32.0)[..., None]
    axis, sign = np.where(surface, normal >> 1, 0), np.where(normal & 1, -1.0, 1.0)
    np.put_along_axis(P, axis[..., None], np.take_along_axis(P, axis[..., None], -1) + (sign / 32.0)[..., None], -1)
    return surface, P, axis, sign, d


def scatter(planes, u, width, height, n, seed=1):
    """n lights of radius RADIUS: random pixels of the view, each light 1 to 4 units off the pixel's surface along its normal (30 units
    along the ray where the pixel shows sky)."""
    import numpy as np
    from raytrace_amd import render
    rng = np.random.default_rng(seed)
    o, f = (np.array(v[:], dtype=np.float64) for v in (u.origin, u.forward))
    if n == 0:
        return render.make_point_lights((o - 50.0 * f)[None], RADIUS, (30.0, 20.0, 10.0))
    surface, P, axis, sign, d = surface_points(planes, u, width, height)
    ys, xs = rng.integers(0, height, n), rng.integers(0, width, n)
    pos = np.where(surface[ys, xs][:, None], P[ys, xs], o[None] + 30.0 * d[ys, xs])
    off = rng.uniform(1.0, 4.0, n) * sign[ys, xs] * surface[ys, xs]
    pos[np.arange(n), axis[ys, xs]] += off
    return render.make_point_lights(pos, RADIUS, rng.uniform(5.0, 40.0, (n, 3)))


def cull_statistics(planes, u, width, height, lights):
    """(tiles with a surface pixel, mean candidates per such tile, mean lanes passing the exact test per candidate over the first 64 lights)."""
    import numpy as np
    surface, P, axis, sign, _ = surface_points(planes, u, width, height)
    ty, tx = (height + 7) // 8, (width + 7) // 8
    pad = lambda a, fill: np.pad(a, ((0, ty * 8 - height), (0, tx * 8 - width)) + ((0, 0),) * (a.ndim - 2), constant_values=fill)
    surf = pad(surface, False).reshape(ty, 8, tx, 8)
    Pp = pad(P, 0.0).reshape(ty, 8, tx, 8, 3)
    lo = np.where(surf[..., None], Pp, np.inf).min(axis=(1, 3)).reshape(-1, 3)
    hi = np.where(surf[..., None], Pp, -np.inf).max(axis=(1, 3)).reshape(-1, 3)
    live = surf.any(axis=(1, 3)).reshape(-1)
    pos, r2 = lights["position"].astype(np.float64), lights["radius"].astype(np.float64) ** 2
    cand = np.zeros((len(lights), lo.shape[0]), dtype=bool)
    for i in range(len(lights)):
        g = np.maximum(np.maximum(pos[i][None] - hi, lo - pos[i][None]), 0.0)
        cand[i] = live & ((g * g).sum(axis=-1) < r2[i])
    lanes = cands = 0
    for i in range(min(len(lights), 64)):
        v = pos[i][None, None] - P
        c = np.take_along_axis(v, axis[..., None], -1)[..., 0] * sign
        d2 = (v * v).sum(axis=-1)
        passes = pad(surface & (d2 > 0) & (d2 < r2[i]) & (c > 0), False).reshape(ty, 8, tx, 8).sum(axis=(1, 3)).reshape(-1)
        lanes += int(passes[cand[i]].sum())
        cands += int(cand[i].sum())
    return int(live.sum()), cand.sum() / max(int(live.sum()), 1), lanes / max(cands, 1)


def one(width, height, count):
    import numpy as np
    import torch
    from raytrace_amd import abi, render, world
    from tools.draw_boxes_profile import scatter as scatter_boxes
    noise = np.fromfile(os.path.join(ROOT, "tests", "golden", "blue_noise_512.rgba"), dtype=np.uint8)
    with render.Context(render.make_config(width, height, spp=1, depth=2, flags=abi.RT_FLAG_CACHE_PRIMARY)) as ctx:
        ctx.generate_world(world.DEFAULT_SEED)
        ctx.upload_noise(noise)
        u = render.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 5)
        boxes = scatter_boxes(u, 256)
        face = ctx.probe_records(u, render.face_probes(boxes), 4, 2)
        ctx.draw_frame(u)
        planes = {n: ctx.readback(b) for b, n in ((abi.RT_BUF_NORMAL_R8UI, "normal_r8"), (abi.RT_BUF_DEPTH_F32, "depth_f32"))}
        lights = scatter(planes, u, width, height, count)
        dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(len(a), -1).copy()).cuda()
        d_boxes, d_face, d_lights = dev(boxes), dev(face), dev(lights)
        torch.cuda.synchronize()
        before = ctx.readback(abi.RT_BUF_LIGHTING_F32)
        for k in range(FRAMES):
            u.seed = 5 + k
            ctx.draw_frame(u)
            ctx.draw_boxes_async(u, d_boxes, d_face)
            if k == 0:
                lit_before = ctx.readback(abi.RT_BUF_LIGHTING_F32)
            ctx.add_lights_async(u, d_lights)
            if k == 0:
                lit = int(np.count_nonzero((ctx.readback(abi.RT_BUF_LIGHTING_F32) != lit_before).any(axis=-1)))
            ctx.denoise(True)
            ctx.finalize()
        ctx.sync()
    del before
    tiles, cands, lanes = cull_statistics(planes, u, width, height, lights)
    print("done %dx%d %d lights, %d pixels lit; %d tiles with a surface pixel, %.3f candidates per tile, %.2f lanes tracing per candidate" % (
        width, height, count, lit, tiles, cands, lanes))


def profile_all(out_path):
    rows = ["# rocprofv3 --kernel-trace --stats, MI355X: %d one-sample frames, each followed by rt_draw_boxes_async (256 boxes), rt_add_lights_async," % FRAMES,
            "# rt_denoise and rt_finalize (tools/point_lights_profile.py; one process per configuration).  Lights: radius 8, 1 to 4 units off the surface",
            "# of random pixels of the view; \"0\" launches with one light behind the camera that reaches nothing.  The cull statistics restate the",
            "# kernel's cull on the host in float64; lanes per candidate over the first 64 lights."]
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
                    if not any(k in name for k in ("k_add_lights", "k_draw_boxes", "k_denoise", "k_finalize")):
                        continue
                    calls, avg = int(col("calls")), float(col("average")) / 1e3
                    rows.append("%-16s %-64s calls %4d avg_us %8.2f min_us %8.2f max_us %8.2f" % (
                        tag, name[:64], calls, avg, float(col("min")) / 1e3, float(col("max")) / 1e3))
                    if "k_denoise" in name:
                        post += calls * avg / FRAMES
                rows.append("%-16s denoise total per frame (%d frames): %.2f us; %s" % (tag, FRAMES, post, done[-1] if done else ""))
                print(rows[-1], flush=True)
            with open(out_path, "w") as fh:      # (kept after every configuration: a run cut short leaves what it measured)
                fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    if len(sys.argv) >= 4:
        one(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]))
    else:
        out = sys.argv[1] if len(sys.argv) == 2 else os.path.join(ROOT, "profiles", "point_lights_kernel_stats.txt")
        profile_all(out)
