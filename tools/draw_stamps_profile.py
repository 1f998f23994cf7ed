"""What rt_draw_stamps costs beside rt_draw_boxes on the bounding boxes of the same records (profiles/draw_stamps_kernel_stats.txt,
DESIGN.md "Voxel-model entities").

    python tools/draw_stamps_profile.py [OUT]          # every configuration, each under rocprofv3 in a process of its own
    python tools/draw_stamps_profile.py --host [OUT]   # appends the host-side restatement of where the time goes (no GPU, minutes of CPU)

One configuration is `rt_bench --models N --model-scale S --width W --height H`: N copies of a 9 x 9 x 12 sparse stamp scattered over
the view 20 to 400 units away, drawn 21 times by rt_draw_stamps and then, as the yardstick, their bounding boxes 21 times by
rt_draw_boxes.  The first form runs `rocprofv3 --kernel-trace --stats` (no counters; the program after `--`) over 1920x1080 and
1024x1024 with 0, 64, 256, 1024 and 4096 models at scales 1/8 and 1 and writes, per configuration, the average, minimum and maximum
duration of k_draw_stamps and k_draw_boxes, their ratio and rt_bench's own line.  With 0 models neither call launches anything.

Where the time goes is restated on the host for the same distribution of models (not the same records: rt_bench seeds its own): the
bounding boxes whose projection meets an 8x8 tile (what the cull keeps, from below), and — from tests/draw_stamps_ref.py on a frame of
a quarter of the width and height — the bounding boxes a pixel's ray enters and the cells it steps through.  There is no pass/fail
bar."""
import csv, glob, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1920, 1080), (1024, 1024))
COUNTS = (0, 64, 256, 1024, 4096)
SCALES = (0.125, 1.0)
EXTENT = (9, 9, 12)


def host_stats(width, height, n, scale, seed=1):
    """(candidates per tile, boxes entered per pixel, steps per pixel, steps per entered box, share of pixels drawn over sky)."""
    import numpy as np
    from raytrace_amd import render
    from tests import draw_stamps_ref as ref
    from tests import stamp_edits as se
    rng = np.random.default_rng(seed)
    u = render.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, 0.0, 0.0, 5)
    o, f, r, up = (np.array(v[:], dtype=np.float64) for v in (u.origin, u.forward, u.right, u.up))
    state = np.where(rng.random(EXTENT[::-1]) < 1.0 / 3.0, se.SOLID, se.AIR).astype(np.uint8)
    stamps = {1: (np.ones(EXTENT[::-1], dtype=np.uint32), state)}
    sx, sy = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    v = f[None] + r[None] * sx[:, None] + up[None] * sy[:, None]
    c = o[None] + v / np.linalg.norm(v, axis=1, keepdims=True) * np.exp(rng.uniform(np.log(20.0), np.log(400.0), n))[:, None]
    orient = np.arange(n) % 48
    models = render.make_draw_stamps(1, c, scale, orient)
    lo, hi = render.stamp_bounding_boxes(models, EXTENT)
    models["origin"] = lo - (hi - lo) / 2
    lo, hi = render.stamp_bounding_boxes(models, EXTENT)
    # candidates per tile: the pixel rectangle of the eight projected corners (models in front of the camera plane only)
    tiles = np.zeros(((height + 7) // 8, (width + 7) // 8), dtype=np.int64)
    for i in range(n):
        corners = np.array([[(lo[i], hi[i])[b][k] for k, b in enumerate(bits)] for bits in np.ndindex(2, 2, 2)], dtype=np.float64) - o
        z = corners @ f
        if (z <= 1e-3).any():
            tiles += 1                                                   # straddles the camera plane: every tile keeps it
            continue
        px = ((corners @ r) / (r @ r) / z + 1.0) * 0.5 * width
        py = ((corners @ up) / (up @ up) / z + 1.0) * 0.5 * height
        x0, x1, y0, y1 = int(np.floor(px.min())) // 8, int(np.floor(px.max())) // 8, int(np.floor(py.min())) // 8, int(np.floor(py.max())) // 8
        if x1 < 0 or y1 < 0 or x0 >= tiles.shape[1] or y0 >= tiles.shape[0]:
            continue
        tiles[max(y0, 0):y1 + 1, max(x0, 0):x1 + 1] += 1
    w4, h4 = width // 4, height // 4
    _, idx, _, _, _ = ref.winners(u, models, stamps, w4, h4)
    st = ref.walk_stats()
    pix = float(w4 * h4)
    return tiles.mean(), st["pairs"] / pix, st["steps"] / pix, st["steps"] / max(st["pairs"], 1), np.count_nonzero(idx >= 0) / pix


def host_rows():
    rows = ["# where the time goes, restated on the host (the same distribution of models; a pixel's figures from a frame of a quarter of the",
            "# width and height): bounding boxes whose projection meets an 8x8 tile, bounding boxes a pixel's ray enters, cells it steps"
            " through", "%-22s %10s %12s %12s %12s %8s" % ("configuration", "cand/tile", "entered/pix", "steps/pix", "steps/entry", "covered")]
    for (w, h) in SHAPES:
        for scale in SCALES:
            for n in COUNTS[1:]:
                rows.append("%-22s %10.2f %12.3f %12.3f %12.2f %7.1f%%" % (("%dx%d_%d_s%g" % (w, h, n, scale),) + tuple(
                    x * (100.0 if k == 4 else 1.0) for k, x in enumerate(host_stats(w, h, n, scale)))))
                print(rows[-1], flush=True)
    return rows


def profile_all(out_path):
    rows = ["# rocprofv3 --kernel-trace --stats, MI355X: rt_bench --models N --model-scale S (tools/draw_stamps_profile.py; one process per",
            "# configuration): 21 rt_draw_stamps of N copies of a 9 x 9 x 12 stamp, a third solid, scattered over the view 20 to 400 units away,",
            "# then 21 rt_draw_boxes of the bounding boxes of the same records.  0 models: neither call launches."]
    bench = os.path.join(ROOT, "raytrace_amd", "rt_bench")
    for (w, h) in SHAPES:
        for scale in SCALES:
            for n in COUNTS:
                if n == 0 and scale != SCALES[0]:
                    continue
                tag = "%dx%d_%d_s%g" % (w, h, n, scale)
                with tempfile.TemporaryDirectory() as tmp:
                    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", bench, "--models", str(n),
                           "--model-scale", str(scale), "--width", str(w), "--height", str(h)]
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=200, cwd=ROOT)
                    if r.returncode != 0:
                        sys.exit("%s: rocprofv3 exited with %d\n%s" % (tag, r.returncode, r.stderr[-2000:]))
                    line = [l for l in r.stdout.splitlines() if l.startswith("{\"models\"")]
                    stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
                    if not stats:
                        sys.exit("%s: no kernel_stats.csv" % tag)
                    avg = {}
                    for rec in csv.DictReader(open(stats[0])):
                        col = lambda key: next(v for k, v in rec.items() if k.lower().startswith(key))   # Name, Calls, AverageNs, MinNs, MaxNs
                        name = col("name")
                        for kernel in ("k_draw_stamps", "k_draw_boxes"):
                            if kernel in name:
                                avg[kernel] = float(col("average")) / 1e3
                                rows.append("%-22s %-16s calls %4d avg_us %9.2f min_us %9.2f max_us %9.2f" % (
                                    tag, kernel, int(col("calls")), avg[kernel], float(col("min")) / 1e3, float(col("max")) / 1e3))
                    if len(avg) == 2:
                        rows.append("%-22s k_draw_stamps / k_draw_boxes = %.2f" % (tag, avg["k_draw_stamps"] / avg["k_draw_boxes"]))
                    elif n:
                        sys.exit("%s: a kernel is missing from the trace" % tag)
                    if line:
                        j = json.loads(line[-1])
                        rows.append("%-22s rt_bench: events %.4f / %.4f ms, %d pixels drawn (bounding boxes: %d)" % (
                            tag, j["draw_stamps_device_ms"], j["bounding_boxes_device_ms"], j["pixels_drawn"], j["bounding_box_pixels"]))
                    print("\n".join(r for r in rows if r.startswith(tag)), flush=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--host"]
    out = args[0] if args else os.path.join(ROOT, "profiles", "draw_stamps_kernel_stats.txt")
    if "--host" in sys.argv[1:]:
        with open(out, "a") as fh:
            fh.write("\n".join(host_rows()) + "\n")
    else:
        profile_all(out)
