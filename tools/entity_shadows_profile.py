"""What rt_shadow_entities costs beside the entity boxes, the point lights and the post passes of the same frame
(profiles/entity_shadows_kernel_stats.txt, DESIGN.md "Entity shadows").

    python tools/entity_shadows_profile.py [OUT [WIDTH HEIGHT]]         # every configuration (of one frame size), each under rocprofv3
    python tools/entity_shadows_profile.py WIDTH HEIGHT KIND COUNT      # one configuration (what the first form runs under the profiler)

One configuration: FRAMES one-sample frames, each followed by rt_draw_boxes_async of the occluders' boxes (for models: their bounding
boxes), rt_shadow_entities_async of COUNT occluders, rt_add_lights_async of as many lights of radius 8 at the occluders' centres (at
most 1024) and rt_denoise.  KIND is `boxes` (player-sized, 0.6 x 0.6 x 1.8), `models8` or `models1` (a 9 x 9 x 12 stamp, four
voxels in ten solid, at scale 1/8 or 1, the 48 orientations in turn); the occluders stand 0.5 to 6 units above what random pixels of the view show.
COUNT 0 enqueues no shadow launch at all (the call returns before it).  The first form runs `rocprofv3 --kernel-trace --stats` over
1920x1080 and 1024x1024 with 0, 64, 256, 1024 and 4096 occluders of each kind and writes, per configuration, the average, minimum and
maximum duration of k_shadow_entities, k_add_lights, k_draw_boxes and the denoise launches.  Each configuration also restates the
kernel's cull on the host (float64: a statistic, not a check) — the mean number of candidates per tile that has a surface pixel — and
gives the share of surface pixels some occluder shades (the pixels that go on to the world's ray), from tests/entity_shadow_ref.py on
every eighth pixel of every eighth row.  There is no pass/fail bar."""
import csv, glob, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 20
SHAPES = ((1920, 1080), (1024, 1024))
COUNTS = (0, 64, 256, 1024, 4096)
KINDS = ("boxes", "models8", "models1")
EXTENT = (9, 9, 12)


def occluders(planes, u, width, height, kind, n, stamp, seed=1):
    """(boxes, models or None, centres)."""
    import numpy as np
    from raytrace_amd import render
    from tests import stamp_edits as se
    from tests.point_light_ref import surface_points
    rng = np.random.default_rng(seed)
    surface, P, _, _ = surface_points(planes, u, width, height)
    pts = P[surface].astype(np.float64)
    c = pts[rng.integers(0, len(pts), n)]
    c[:, 2] += rng.uniform(0.5, 6.0, n)
    if kind == "boxes":
        half = np.array([0.3, 0.3, 0.9])
        return render.make_draw_boxes(c - half, c + half, 0x1FFFFF, 0xFF000000), None, c
    scale = 0.125 if kind == "models8" else 1.0
    orient = np.arange(n) % 48
    ext = np.array([se.placed_extent(EXTENT, int(o)) for o in orient], dtype=np.float64).reshape(n, 3)
    models = render.make_draw_stamps(stamp, c - 0.5 * ext * scale, scale, orient)
    lo = models["origin"].astype(np.float32)
    hi = (ext.astype(np.float32) * np.float32(scale) + lo).astype(np.float32)
    return render.make_draw_boxes(lo, hi, 0x1FFFFF, 0xFF000000), models, c


def cull_statistics(planes, u, width, height, boxes):
    """(tiles with a surface pixel, mean candidates per such tile): the kernel's cull restated in float64."""
    import numpy as np
    from oracle import pyoracle as po
    from tests.point_light_ref import surface_points
    surface, P, _, _ = surface_points(planes, u, width, height)
    s = po.sun(u.sun_angle)[0].astype(np.float64)
    ty, tx = (height + 7) // 8, (width + 7) // 8
    pad = lambda a, fill: np.pad(a, ((0, ty * 8 - height), (0, tx * 8 - width)) + ((0, 0),) * (a.ndim - 2), constant_values=fill)
    surf = pad(surface, False).reshape(ty, 8, tx, 8)
    Pp = pad(P.astype(np.float64), 0.0).reshape(ty, 8, tx, 8, 3)
    live = surf.any(axis=(1, 3)).reshape(-1)
    blo = np.where(surf[..., None], Pp, np.inf).min(axis=(1, 3)).reshape(-1, 3)[live]
    bhi = np.where(surf[..., None], Pp, -np.inf).max(axis=(1, 3)).reshape(-1, 3)[live]
    total = 0
    for b in boxes:
        lo, hi = b["lo"].astype(np.float64), b["hi"].astype(np.float64)
        tn = np.max([((lo[k] - bhi[:, k]) if s[k] > 0 else (hi[k] - blo[:, k])) / s[k] for k in range(3)], axis=0)
        tf = np.min([((hi[k] - blo[:, k]) if s[k] > 0 else (lo[k] - bhi[:, k])) / s[k] for k in range(3)], axis=0)
        total += int(((tn < tf) & (tf > 0)).sum())
    return int(live.sum()), total / max(int(live.sum()), 1)


def one(width, height, kind, count):
    import numpy as np
    import torch
    from raytrace_amd import abi, render, world
    from tests import entity_shadow_ref as ref
    noise = np.fromfile(os.path.join(ROOT, "tests", "golden", "blue_noise_512.rgba"), dtype=np.uint8)
    with render.Context(render.make_config(width, height, spp=1, depth=2, flags=abi.RT_FLAG_CACHE_PRIMARY)) as ctx:
        ctx.generate_world(world.DEFAULT_SEED)
        ctx.upload_noise(noise)
        u = render.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 5)
        mats, state = ref.small_stamp(seed=7, extent=EXTENT)
        stamp = ctx.stamp_create(mats, state)
        ctx.draw_frame(u)
        planes = {n: ctx.readback(b) for b, n in ((abi.RT_BUF_NORMAL_R8UI, "normal_r8"), (abi.RT_BUF_DEPTH_F32, "depth_f32"))}
        boxes, models, centres = occluders(planes, u, width, height, kind, max(count, 1), stamp)
        if count == 0:
            boxes, models, centres = boxes[:0], (None if models is None else models[:0]), centres[:0]
        nl = min(count, 1024)
        lights = render.make_point_lights(centres[:nl] if nl else (np.array(u.origin[:]) - 50.0 * np.array(u.forward[:]))[None], 8.0, (30.0, 20.0, 10.0))
        face = np.zeros(6 * max(len(boxes), 1), dtype=render.PROBE_LIGHT_DTYPE)
        face["light"] = 8.0
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).cuda()
        d_boxes = dev(boxes) if len(boxes) else None
        d_face, d_lights = dev(face), dev(lights)
        torch.cuda.synchronize()
        changed = 0
        for k in range(FRAMES):
            u.seed = 5 + k
            ctx.draw_frame(u)
            if d_boxes is not None:
                ctx.draw_boxes_async(u, d_boxes, d_face[:6 * len(boxes)])
            if k == 0:
                before = ctx.readback(abi.RT_BUF_LIGHTING_F32)
            ctx.shadow_entities_async(u, d_boxes if models is None else None, models)
            if k == 0:
                ctx.sync()      # (a launch still in flight when the host starts a readback into fresh memory is stretched by milliseconds)
                changed = int(np.count_nonzero((ctx.readback(abi.RT_BUF_LIGHTING_F32) != before).any(axis=-1)))
            ctx.add_lights_async(u, d_lights)
            ctx.denoise(True)
        ctx.sync()
        after_draw = {n: ctx.readback(b) for b, n in ((abi.RT_BUF_NORMAL_R8UI, "normal_r8"), (abi.RT_BUF_DEPTH_F32, "depth_f32"))}
    tiles, cands = cull_statistics(after_draw, u, width, height, boxes)
    # the share of surface pixels some occluder shades, on every eighth pixel of every eighth row
    surface, P, _, _ = ref.surface_points(after_draw, u, width, height)
    pts = P[::8, ::8][surface[::8, ::8]].astype(np.float32)
    s = ref.sun_of(u)[0]
    shaded = ref.boxes_shade(boxes, pts, s) if models is None else ref.models_shade(models, {stamp: (mats, state)}, pts, s)
    print("done %dx%d %s %d, %d pixels changed; %d tiles with a surface pixel, %.3f candidates per tile, %.4f of the surface pixels shaded" % (
        width, height, kind, count, changed, tiles, cands, float(shaded.mean()) if len(pts) else 0.0))


def profile_all(out_path, shapes):
    rows = ["# rocprofv3 --kernel-trace --stats, MI355X: %d one-sample frames, each followed by rt_draw_boxes_async (the occluders' boxes)," % FRAMES,
            "# rt_shadow_entities_async, rt_add_lights_async (as many lights of radius 8, at most 1024) and rt_denoise (tools/entity_shadows_profile.py;",
            "# one process per configuration).  Occluders 0.5 to 6 units above what random pixels show: player-sized boxes, or a 9 x 9 x 12 stamp",
            "# (four voxels in ten solid) at scale 1/8 (models8) or 1 (models1).  The cull statistic restates the kernel's cull on the host in float64."]
    if os.path.exists(out_path):
        rows = open(out_path).read().splitlines()
    for (w, h) in shapes:
        for kind in KINDS:
            for n in COUNTS:
                if n == 0 and kind != "boxes":
                    continue
                tag = "%dx%d_%s_%d" % (w, h, kind, n)
                with tempfile.TemporaryDirectory() as tmp:
                    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                           str(w), str(h), kind, str(n)]
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=200)
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
                        if not any(k in name for k in ("k_shadow_entities", "k_add_lights", "k_draw_boxes", "k_denoise")):
                            continue
                        calls, avg = int(col("calls")), float(col("average")) / 1e3
                        rows.append("%-28s %-64s calls %4d avg_us %8.2f min_us %8.2f max_us %8.2f" % (
                            tag, name[:64], calls, avg, float(col("min")) / 1e3, float(col("max")) / 1e3))
                        if "k_denoise" in name:
                            post += calls * avg / FRAMES
                    rows.append("%-28s denoise total per frame (%d frames): %.2f us; %s" % (tag, FRAMES, post, done[-1] if done else ""))
                    print(rows[-1], flush=True)
                with open(out_path, "w") as fh:      # (kept after every configuration: a run cut short leaves what it measured)
                    fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 5:
        one(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]))
    else:
        out = sys.argv[1] if len(sys.argv) >= 2 else os.path.join(ROOT, "profiles", "entity_shadows_kernel_stats.txt")
        profile_all(out, ((int(sys.argv[2]), int(sys.argv[3])),) if len(sys.argv) == 4 else SHAPES)
