"""Ray-query throughput and pick latency on the MI355X (DESIGN.md "Ray queries").

    python tools/ray_query_bench.py [--sizes 1048576,16777216] [--sweep]

For each size and ray distribution — incoherent (seeded origins in the region, random directions) and coherent (a 1920x1080
camera's primary rays handed over as arbitrary rays) — rt_trace_rays_async runs on device tensors on a caller's stream; G rays/s
comes from torch.cuda events round the calls.  --sweep adds smaller sizes.  Then the latency of one-pixel rt_pick_pixels calls (call to return), idle and right after a 1920x1080 spp 64 depth 4
frame was submitted.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raytrace_amd import abi, render, world  # noqa: E402


def _ctx(mats, mine, W=1920, H=1080, **kw):
    ctx = render.Context(render.make_config(W, H, **kw))
    ctx.upload_world(mats, mine)
    return ctx


def _rays(kind, n, rng):
    r = np.zeros((n, 8), np.float32)
    if kind == "incoherent":
        r[:, 0:3] = rng.uniform(-127.0, 127.0, (n, 3))
        r[:, 4:7] = rng.normal(size=(n, 3))
    else:
        u = render.camera_uniforms(render.DEFAULT_POSE["origin"], render.DEFAULT_POSE["heading"], render.DEFAULT_POSE["pitch"])
        W, H = 1920, 1080
        i = np.arange(n) % (W * H)
        sx = (i % W).astype(np.float32) / np.float32(W) * np.float32(2) - np.float32(1)
        sy = (i // W).astype(np.float32) / np.float32(H) * np.float32(2) - np.float32(1)
        d = np.float32(u.forward[:]) + np.float32(u.right[:]) * sx[:, None] + np.float32(u.up[:]) * sy[:, None]
        r[:, 0:3] = np.float32(u.origin[:])
        r[:, 4:7] = d
    return r


def grays(ctx, rays_t, hits_t, stream, reps):
    with torch.cuda.stream(stream):
        ctx.trace_rays_async(rays_t, hits_t)   # warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            ctx.trace_rays_async(rays_t, hits_t)
        e1.record(stream)
    stream.synchronize()
    ms = e0.elapsed_time(e1) / reps
    return rays_t.shape[0] / (ms * 1e-3) / 1e9, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1048576,16777216")
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    if a.sweep:
        sizes = [1 << k for k in (10, 12, 14, 16, 17, 18, 19)] + sizes
    mats, mine = world.generate_region(world.DEFAULT_SEED)
    rng = np.random.default_rng(1)
    out = {"throughput": []}
    stream = torch.cuda.Stream()
    ctx = _ctx(mats, mine, 64, 64)
    ctx.set_stream(stream.cuda_stream)
    for kind in ("incoherent", "coherent"):
        for n in sizes:
            rays_t = torch.from_numpy(_rays(kind, n, rng)).cuda()
            hits_t = torch.empty((n, 48), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            g, ms = grays(ctx, rays_t, hits_t, stream, 5 if n >= (1 << 20) else 20)
            row = {"rays": kind, "n": n, "grays": round(g, 3), "ms": round(ms, 4)}
            out["throughput"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del rays_t, hits_t
    ctx.set_stream(None)
    ctx.destroy()

    # pick latency: one pixel, call to return
    noise = np.fromfile(os.path.join(ROOT, "tests", "golden", "blue_noise_512.rgba"), dtype=np.uint8)
    u = render.camera_uniforms(render.DEFAULT_POSE["origin"], render.DEFAULT_POSE["heading"], render.DEFAULT_POSE["pitch"])
    ctx = _ctx(mats, mine, 1920, 1080, spp=64, depth=4, flags=abi.RT_FLAG_CACHE_PRIMARY)
    ctx.upload_noise(noise)
    for _ in range(20):
        ctx.pick_pixels(u, [(960, 540)])
    idle = []
    for _ in range(200):
        t = time.perf_counter()
        ctx.pick_pixels(u, [(960, 540)])
        idle.append((time.perf_counter() - t) * 1e3)
    ctx.draw_frame(u)
    ctx.sync()
    t = time.perf_counter()
    ctx.draw_frame(u)
    ctx.sync()
    frame_ms = (time.perf_counter() - t) * 1e3
    busy = []
    for _ in range(20):
        ctx.draw_frame(u)
        t = time.perf_counter()
        ctx.pick_pixels(u, [(960, 540)])
        busy.append((time.perf_counter() - t) * 1e3)
        ctx.sync()
    ctx.destroy()
    out["pick_ms_idle_median"] = round(float(np.median(idle)), 4)
    out["pick_ms_idle_p90"] = round(float(np.percentile(idle, 90)), 4)
    out["pick_ms_frame_in_flight_median"] = round(float(np.median(busy)), 4)
    out["pick_ms_frame_in_flight_max"] = round(float(np.max(busy)), 4)
    out["frame_ms"] = round(frame_ms, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
