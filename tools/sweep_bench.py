"""Box-sweep throughput on the MI355X beside ray queries from the same points (DESIGN.md "Box sweeps").

    python tools/sweep_bench.py [--n 1048576] [--reps 100] [--rounds 5]

n player-sized boxes (0.6 x 0.6 x 1.8) that start just above the terrain surface of the procedural region and move by a vector of
length 1 in a random direction run through rt_sweep_boxes_async, and n rays from the boxes' centres along the same vectors through
rt_trace_rays_async, on device tensors on a caller's stream.  The two alternate for `rounds` rounds in one run; each round times
`reps` back-to-back calls with torch.cuda events after a warm-up call.  Prints one JSON line per round to stderr and one JSON
summary line (medians over the rounds, and the ratio) to stdout."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raytrace_amd import render, world  # noqa: E402


def surface_boxes(mine, n, rng, R=256):
    """float32[n, 3, 3] (lo, hi, motion): a player-sized box 0.05 .. 0.5 above the highest occupied voxel of a random column."""
    solid = mine.reshape(R, R, R) == 0
    top = R - np.argmax(solid[::-1], axis=0) - R // 2       # world z of the surface per [y][x] column
    ix, iy = rng.integers(8, R - 8, n), rng.integers(8, R - 8, n)
    lo = np.stack([ix - R // 2 + rng.random(n) * 0.4, iy - R // 2 + rng.random(n) * 0.4, top[iy, ix] + rng.uniform(0.05, 0.5, n)], 1)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = np.zeros((n, 3, 3), np.float32)
    out[:, 0] = lo
    out[:, 1] = out[:, 0] + np.float32([0.6, 0.6, 1.8])
    out[:, 2] = d
    return out


def timed(call, stream, reps):
    with torch.cuda.stream(stream):
        call()   # warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            call()
        e1.record(stream)
    stream.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    mats, mine = world.generate_region(world.DEFAULT_SEED)
    boxes = surface_boxes(mine, a.n, np.random.default_rng(1))
    recs = render.make_sweeps(boxes)
    rays = np.zeros((a.n, 8), np.float32)
    rays[:, 0:3] = (boxes[:, 0] + boxes[:, 1]) * np.float32(0.5)
    rays[:, 4:7] = boxes[:, 2]
    stream = torch.cuda.Stream()
    ctx = render.Context(render.make_config(64, 64))
    ctx.upload_world(mats, mine)
    ctx.set_stream(stream.cuda_stream)
    sweeps_t = torch.from_numpy(recs.view(np.uint8).reshape(-1, 48).copy()).cuda()
    sweep_hits_t = torch.empty((a.n, 64), dtype=torch.uint8, device="cuda")
    rays_t = torch.from_numpy(rays).cuda()
    ray_hits_t = torch.empty((a.n, 48), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rows = []
    for k in range(a.rounds):
        sweep_ms = timed(lambda: ctx.sweep_boxes_async(sweeps_t, sweep_hits_t), stream, a.reps)
        ray_ms = timed(lambda: ctx.trace_rays_async(rays_t, ray_hits_t), stream, a.reps)
        rows.append((sweep_ms, ray_ms))
        print(json.dumps({"round": k, "n": a.n, "reps": a.reps, "sweep_ms": round(sweep_ms, 4), "ray_ms": round(ray_ms, 4)}), file=sys.stderr, flush=True)
    hits = sweep_hits_t.cpu().numpy().view(render.SWEEP_HIT_DTYPE).reshape(-1)
    ray_hits = ray_hits_t.cpu().numpy().view(render.HIT_DTYPE).reshape(-1)
    ctx.set_stream(None)
    ctx.destroy()
    sweep_ms, ray_ms = (float(np.median([r[i] for r in rows])) for i in (0, 1))
    kinds = np.bincount(hits["kind"], minlength=4)
    print(json.dumps({
        "n": a.n, "reps": a.reps, "rounds": a.rounds,
        "sweep_ms": round(sweep_ms, 4), "sweep_ms_min_max": [round(min(r[0] for r in rows), 4), round(max(r[0] for r in rows), 4)],
        "ray_ms": round(ray_ms, 4), "ray_ms_min_max": [round(min(r[1] for r in rows), 4), round(max(r[1] for r in rows), 4)],
        "sweep_over_ray": round(sweep_ms / ray_ms, 3), "msweeps_per_s": round(a.n / sweep_ms / 1e3, 1), "mrays_per_s": round(a.n / ray_ms / 1e3, 1),
        "sweeps_free_blocked_embedded_invalid": [int(v) for v in kinds],
        "rays_air_solid_limit": [int(v) for v in np.bincount(ray_hits["kind"], minlength=3)],
        "mean_ray_iterations": round(float(ray_hits["iterations"].mean()), 2)}))


if __name__ == "__main__":
    main()
