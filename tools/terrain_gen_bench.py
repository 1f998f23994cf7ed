"""Device time of rt_generate_world and rt_generate_slice at R = 256, 512 and 1024 (HIP events on the context's stream, through
torch), next to the host path they replace: world.generate_region (one core) + rt_upload_world, wall time.

    python tools/terrain_gen_bench.py [--regions 256 512 1024] [--reps 5] [--no-host] [--out FILE.jsonl]

One JSON line per (R, what).  Needs a GPU."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from raytrace_amd import render, world  # noqa: E402


def device_ms(ctx, stream, fn, reps):
    """Median device time of fn() over reps calls, each bracketed by events on the context's (caller-given) stream."""
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []
    s = torch.cuda.Stream(device=0)
    for R in args.regions:
        with render.Context(render.make_config(64, 64, region=R)) as ctx:
            ctx.set_stream(s.cuda_stream)
            seed = world.DEFAULT_SEED
            ctx.generate_world(seed)                       # warm-up: code objects, scratch allocation
            ctx.generate_slice(seed, 0, (R // 2, -R // 2, -R // 2))
            s.synchronize()
            med, lo = device_ms(ctx, s, lambda: ctx.generate_world(seed), args.reps)
            lines.append({"R": R, "what": "rt_generate_world", "device_ms_median": med, "device_ms_min": lo})
            for axis in range(3):
                win = [-R // 2] * 3
                k = [0]

                def one():
                    win[axis] = R // 2 + 16 * (k[0] % (R // 16))
                    k[0] += 1
                    ctx.generate_slice(seed, axis, tuple(win))
                med, lo = device_ms(ctx, s, one, max(args.reps, 8))
                lines.append({"R": R, "what": "rt_generate_slice", "axis": axis, "device_ms_median": med, "device_ms_min": lo})
            assert ctx.selftest(2) == 0
            ctx.set_stream(0)
            if not args.no_host:
                t0 = time.perf_counter()
                mats, mine = world.generate_region(seed, region=R)
                t1 = time.perf_counter()
                ctx.upload_world(mats, mine)
                ctx.sync()
                t2 = time.perf_counter()
                lines.append({"R": R, "what": "host generate_region + rt_upload_world", "generate_s": t1 - t0, "upload_s": t2 - t1})
                del mats, mine
        for ln in lines:
            if ln["R"] == R:
                print(json.dumps(ln), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
