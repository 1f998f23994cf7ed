"""Light-probe throughput on the MI355X (DESIGN.md "Light probes").

    python tools/probe_bench.py [--shapes 65536x16x2,1x4096x2,4096x1x2] [--reps 20] [--pair 0,1] [--no-frame]

For each shape count x samples x depth, rt_probe_light_async runs on device tensors on a caller's stream; the time per call comes
from torch.cuda events round `reps` calls after a warm-up call, repeated three times (all three are printed: the spread).  The probes
are the primary hits of a 256 x 256 frame of the default camera on the procedural 256 region (rt_pick_pixels), repeated to `count`.
--pair runs every shape on both forms of k_probe in turn, in the same process (RT_PROBE_PAIR: 1 = the shadow and the diffuse ray of
a level stepped together, the shipped form; 0 = one after the other).  Unless --no-frame, the yardstick is timed too: the 256 x 256,
spp 16, depth 2, RT_FLAG_CACHE_PRIMARY frame on the default kernel — as many paths as 65536 probes x 16 samples, plus the primary
prepass.  Prints one JSON line."""
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

FRAME = 256


def _uniforms(seed=1):
    p = render.DEFAULT_POSE
    return render.camera_uniforms(p["origin"], p["heading"], -0.2, 0.3, seed)


def _frame_probes(ctx, u):
    xy = np.stack(np.meshgrid(np.arange(FRAME), np.arange(FRAME)), axis=-1).reshape(-1, 2)
    hits = ctx.pick_pixels(u, xy)
    keep = hits["kind"] != abi.RT_HIT_AIR
    xy, hits = xy[keep], hits[keep]
    cells = np.stack([render.workgroup_of(xy[:, 0]), render.workgroup_of(xy[:, 1])], axis=-1)
    return render.make_probes(hits["position"], hits["normal"], cells)


def _timed(fn, stream, reps):
    """ms per call: three windows of `reps` calls between events, after one warm-up call."""
    out = []
    with torch.cuda.stream(stream):
        fn()
        stream.synchronize()
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            stream.synchronize()
            out.append(round(e0.elapsed_time(e1) / reps, 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x16x2,1x4096x2,4096x1x2")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pair", default="1")
    ap.add_argument("--no-frame", action="store_true")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    mats, mine = world.generate_region(world.DEFAULT_SEED)
    noise = np.fromfile(os.path.join(ROOT, "tests", "golden", "blue_noise_512.rgba"), dtype=np.uint8)
    u = _uniforms()
    stream = torch.cuda.Stream()
    out = {"probes": []}
    base = None
    for pair in [int(v) for v in a.pair.split(",")]:
        os.environ["RT_PROBE_PAIR"] = str(pair)          # read by rt_create
        ctx = render.Context(render.make_config(FRAME, FRAME))
        ctx.upload_world(mats, mine)
        ctx.upload_noise(noise)
        if base is None:
            base = _frame_probes(ctx, u)
            out["surface_fraction"] = round(len(base) / float(FRAME * FRAME), 3)
        ctx.set_stream(stream.cuda_stream)
        for count, samples, depth in shapes:
            probes_t = torch.from_numpy(np.resize(base, count).view(np.uint8).reshape(-1, 32).copy()).cuda()
            out_t = torch.empty((count, 4), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ms = _timed(lambda: ctx.probe_light_async(u, probes_t, out_t, samples, depth), stream, a.reps)
            row = {"pair": pair, "count": count, "samples": samples, "depth": depth, "ms": ms,
                   "mpaths_per_s": round(count * samples / (min(ms) * 1e-3) / 1e6, 1)}
            out["probes"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del probes_t, out_t
        ctx.set_stream(None)
        ctx.destroy()
    os.environ.pop("RT_PROBE_PAIR", None)
    if not a.no_frame:
        ctx = render.Context(render.make_config(FRAME, FRAME, spp=16, depth=2, flags=abi.RT_FLAG_CACHE_PRIMARY))
        ctx.upload_world(mats, mine)
        ctx.upload_noise(noise)
        ctx.set_stream(stream.cuda_stream)
        seeds = iter(range(2, 1 << 20))

        def frame():
            u.seed = next(seeds)      # (the seed advances per frame, as a host drives it)
            ctx.draw_frame(u)
        out["frame_256x256_spp16_depth2_ms"] = _timed(frame, stream, a.reps)
        out["frame_kernel"] = ctx.kernel_in_use()
        ctx.set_stream(None)
        # ... and on the context's own streams (host clock round `reps` frames and the wait for them)
        wall = []
        for _ in range(3):
            ctx.sync()
            t = time.perf_counter()
            for _ in range(a.reps):
                frame()
            ctx.sync()
            wall.append(round((time.perf_counter() - t) * 1e3 / a.reps, 4))
        out["frame_own_stream_wall_ms"] = wall
        ctx.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
