"""What rt_add_lights_occluded costs beside rt_add_lights for the same lights on the same frame
(profiles/light_shadows_kernel_stats.txt, DESIGN.md "Point-light shadows of entities").

    python tools/light_shadows_profile.py                     # every configuration, each under rocprofv3 in a process of its own
    python tools/light_shadows_profile.py WIDTH HEIGHT CASE   # one configuration (what the first form runs under the profiler)

One configuration: FRAMES times a one-sample frame followed by rt_add_lights_async, then a fresh frame followed by
rt_add_lights_occluded_async, both with the same 64 lights of radius 8 scattered just off the visible surfaces
(tools/point_lights_profile.scatter).  The cases differ in the occluders:
    far        256 boxes + 64 models 400 units above the lights: no occluder near any light, so every tile's list is empty and the
               difference to k_add_lights is what the per-tile cull itself costs;
    scattered  256 boxes + 64 models, each within 3 units of a light, in turn;
    overflow   4096 boxes + 64 models within 3 units of the lights: 64 boxes round every light, so the tiles a light reaches list more
               than 64 and scan every record per candidate light.
The first form runs `rocprofv3 --kernel-trace --stats` over each case at 1920x1080 and writes the average, minimum and maximum
duration of k_add_lights and k_add_lights_occluded, and the pixels the entities changed.  There is no pass/fail bar."""
import csv, glob, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 40
SHAPES = ((1920, 1080),)
CASES = {"far": (256, 64, True), "scattered": (256, 64, False), "overflow": (4096, 64, False)}
LIGHTS, SPREAD, EXTENT, SCALE = 64, 3.0, (5, 4, 6), 0.125


def occluders(lights, nboxes, nmodels, far, sid, seed=2):
    """Player-sized boxes and models of the EXTENT stamp at SCALE, each within SPREAD units of a light, in turn (`far`: 400 units above it)."""
    import numpy as np
    from raytrace_amd import render
    rng = np.random.default_rng(seed)
    pos = lights["position"].astype(np.float64)
    lift = np.array([0.0, 0.0, 400.0 if far else 0.0])
    c = pos[np.arange(nboxes) % len(pos)] + rng.uniform(-SPREAD, SPREAD, (nboxes, 3)) + lift
    half = np.array([0.3, 0.3, 0.9])
    boxes = render.make_draw_boxes(c - half, c + half, 0x1FFFFF, 0xFF000000)
    c = pos[np.arange(nmodels) % len(pos)] + rng.uniform(-SPREAD, SPREAD, (nmodels, 3)) + lift
    orient = np.arange(nmodels) % 48
    placed = np.array(EXTENT)[np.array(render.STAMP_PERMS)[orient >> 3]]
    models = render.make_draw_stamps(sid, c - 0.5 * placed * SCALE, SCALE, orient)
    return boxes, models


def one(width, height, case):
    import numpy as np
    import torch
    from raytrace_amd import abi, render, world
    from tools.point_lights_profile import scatter
    nboxes, nmodels, far = CASES[case]
    noise = np.fromfile(os.path.join(ROOT, "tests", "golden", "blue_noise_512.rgba"), dtype=np.uint8)
    with render.Context(render.make_config(width, height, spp=1, depth=2, flags=abi.RT_FLAG_CACHE_PRIMARY)) as ctx:
        ctx.generate_world(world.DEFAULT_SEED)
        ctx.upload_noise(noise)
        u = render.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 5)
        rng = np.random.default_rng(3)
        state = np.where(rng.random(EXTENT[::-1]) < 0.3333, abi.RT_STAMP_SOLID,
                         np.where(rng.random(EXTENT[::-1]) < 0.5, abi.RT_STAMP_AIR, abi.RT_STAMP_ABSENT)).astype(np.uint8)
        sid = ctx.stamp_create(np.where(state == abi.RT_STAMP_SOLID, 0x1FFFFF, 0).astype(np.uint32), state)
        ctx.draw_frame(u)
        planes = {n: ctx.readback(b) for b, n in ((abi.RT_BUF_NORMAL_R8UI, "normal_r8"), (abi.RT_BUF_DEPTH_F32, "depth_f32"))}
        lights = scatter(planes, u, width, height, LIGHTS)
        boxes, models = occluders(lights, nboxes, nmodels, far, sid)
        dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(len(a), -1).copy()).cuda()
        d_boxes, d_lights = dev(boxes), dev(lights)
        torch.cuda.synchronize()
        for k in range(FRAMES):
            u.seed = 5 + k
            ctx.draw_frame(u)
            ctx.add_lights_async(u, d_lights)
            if k == 0:
                plain = ctx.readback(abi.RT_BUF_LIGHTING_F32)
            ctx.draw_frame(u)
            ctx.add_lights_occluded_async(u, d_lights, d_boxes, models)
            if k == 0:
                shadowed = int(np.count_nonzero((ctx.readback(abi.RT_BUF_LIGHTING_F32) != plain).any(axis=-1)))
        ctx.sync()
    print("done %dx%d %s: %d lights, %d boxes, %d models; %d pixels differ from rt_add_lights" % (width, height, case, LIGHTS, nboxes, nmodels, shadowed))


def profile_all(out_path):
    rows = ["# rocprofv3 --kernel-trace --stats, MI355X: %d times a one-sample frame + rt_add_lights_async, then a fresh frame + rt_add_lights_occluded_async," % FRAMES,
            "# the same %d lights of radius 8 (tools/light_shadows_profile.py; one process per case).  far: 256 boxes + 64 models 400 units above" % LIGHTS,
            "# the lights; scattered: the same within 3 units of a light, in turn; overflow: 4096 boxes + 64 models within 3 units of the lights."]
    for (w, h) in SHAPES:
        for case in CASES:
            tag = "%dx%d_%s" % (w, h, case)
            with tempfile.TemporaryDirectory() as tmp:
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                       str(w), str(h), case]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
                if r.returncode != 0:
                    sys.exit("%s: rocprofv3 exited with %d\n%s" % (tag, r.returncode, r.stderr[-2000:]))
                done = [l for l in r.stdout.splitlines() if l.startswith("done")]
                stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
                if not stats:
                    sys.exit("%s: no kernel_stats.csv" % tag)
                for rec in csv.DictReader(open(stats[0])):
                    col = lambda key: next(v for k, v in rec.items() if k.lower().startswith(key))   # Name, Calls, AverageNs, MinNs, MaxNs
                    name = col("name")
                    if "k_add_lights" not in name:
                        continue
                    rows.append("%-20s %-72s calls %4d avg_us %8.2f min_us %8.2f max_us %8.2f" % (
                        tag, name[:72], int(col("calls")), float(col("average")) / 1e3, float(col("min")) / 1e3, float(col("max")) / 1e3))
                    print(rows[-1], flush=True)
                rows.append("%-20s %s" % (tag, done[-1] if done else ""))
                print(rows[-1], flush=True)
            with open(out_path, "w") as fh:      # (kept after every configuration: a run cut short leaves what it measured)
                fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    if len(sys.argv) >= 4:
        one(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3])
    else:
        out = sys.argv[1] if len(sys.argv) == 2 else os.path.join(ROOT, "profiles", "light_shadows_kernel_stats.txt")
        profile_all(out)
