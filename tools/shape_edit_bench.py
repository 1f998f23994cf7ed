"""Shape edits on the MI355X beside rt_edit_voxels fed with the same voxels enumerated (DESIGN.md "Shape edits").

    python tools/shape_edit_bench.py [--calls 40] [--rounds 3] [--voxels-only]

Four shapes round the centre of the procedural 256^3 region — a sphere of radius 8, one of radius 24, a box that is exactly one
64^3 chunk, a box that is the whole region — each applied `calls` times (4 for the whole region), alternately filled and carved, through rt_edit_shapes and,
as one 16-byte record per voxel of the shape, through rt_edit_voxels.  Per case and path: the host time inside the call, the device
time of the call's two launches (RT_FLAG_TIMING_ALL, rt_get_timing) and the wall time per call with one sync at the end; medians
over `rounds` rounds.  --voxels-only runs on a build that has no rt_edit_shapes (the baseline of an earlier commit: run this file
from that tree).  One JSON line per case on stdout."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raytrace_amd import abi, render, world  # noqa: E402

R = 256
WORD = (1 << 15) | (90 << 14) | (60 << 7) | 30
CASES = [("sphere r=8", "sphere", 8), ("sphere r=24", "sphere", 24), ("one chunk box", "box", 64), ("whole region box", "box", 256)]


def voxels_of(kind, n):
    """int[N, 3] (x, y, z) of the shape's voxels: a sphere of radius n round the centre of voxel (128, 128, 128), or the cube of
    edge n whose low corner is (64, 64, 64) (n = 64) or the origin (n = 256)."""
    if kind == "box":
        lo = 0 if n == R else 64
        z, y, x = np.mgrid[lo:lo + n, lo:lo + n, lo:lo + n]
        return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    z, y, x = np.mgrid[127 - n:130 + n, 127 - n:130 + n, 127 - n:130 + n]
    inside = (2 * x + 1 - 257) ** 2 + (2 * y + 1 - 257) ** 2 + (2 * z + 1 - 257) ** 2 <= (2 * n) ** 2
    return np.stack([x[inside], y[inside], z[inside]], axis=1)


def shape_rows(kind, n):
    """The same shape as RtShapeEdit rows, [fill, carve]."""
    if kind == "box":
        lo = 0 if n == R else 64
        return [render.box_shape((lo,) * 3, (lo + n - 1,) * 3, WORD, solid) for solid in (True, False)]
    return [render.sphere_shape((128.5,) * 3, n, WORD, solid) for solid in (True, False)]


def record_rows(xyz):
    recs = np.zeros(len(xyz), dtype=[("x", "<u2"), ("y", "<u2"), ("z", "<u2"), ("solid", "<u2"), ("material", "<u4"), ("reserved", "<u4")])
    recs["x"], recs["y"], recs["z"], recs["material"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], WORD
    out = []
    for solid in (1, 0):
        r = recs.copy()
        r["solid"] = solid
        out.append(r)
    return out


def one_round(ctx, call, calls):
    """(host ms, device ms, wall ms) per call."""
    call(0)
    call(1)
    ctx.sync()
    ctx.timing()                                   # drains the launch timers
    host = 0.0
    w0 = time.perf_counter()
    for i in range(calls):
        h0 = time.perf_counter()
        call(i & 1)
        host += time.perf_counter() - h0
    ctx.sync()
    wall = time.perf_counter() - w0
    tm = ctx.timing()
    assert tm.other_launches == 2 * calls, tm.other_launches
    return 1e3 * host / calls, tm.shade_ms / calls, 1e3 * wall / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--voxels-only", action="store_true")
    a = ap.parse_args()
    mats, mine = world.generate_region(world.DEFAULT_SEED)
    with render.Context(render.make_config(64, 64, flags=abi.RT_FLAG_TIMING_ALL)) as ctx:
        ctx.upload_world(mats, mine)
        ctx.upload_noise(np.fromfile(os.path.join(ROOT, "tests", "golden", "blue_noise_512.rgba"), dtype=np.uint8))
        ctx.draw_frame(render.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, 0.0))   # (rt_get_timing asks for a frame)
        lib, h = ctx._lib, ctx.handle
        for name, kind, n in CASES:
            xyz = voxels_of(kind, n)
            recs = record_rows(xyz)
            ptrs = [r.ctypes.data_as(C.POINTER(abi.RtVoxelEdit)) for r in recs]
            paths = {"voxels": lambda i: ctx._check(lib.rt_edit_voxels(h, ptrs[i], len(xyz)))}
            if not a.voxels_only:
                rows = [np.ascontiguousarray(s).reshape(1) for s in shape_rows(kind, n)]
                sptr = [r.ctypes.data_as(C.POINTER(abi.RtShapeEdit)) for r in rows]
                paths["shapes"] = lambda i: ctx._check(lib.rt_edit_shapes(h, sptr[i], 1))
            calls = a.calls if len(xyz) < (1 << 20) else 4           # (a whole region of records takes a good part of a second per call)
            out = {"case": name, "voxel_count": int(len(xyz)), "calls": calls, "rounds": a.rounds}
            for path, call in paths.items():
                rounds = np.array([one_round(ctx, call, calls) for _ in range(a.rounds)])
                med = np.median(rounds, axis=0)
                out[path] = {"host_ms": round(float(med[0]), 4), "device_ms": round(float(med[1]), 4), "wall_ms": round(float(med[2]), 4),
                             "wall_ms_rounds": [round(float(v), 4) for v in rounds[:, 2]]}
            if "shapes" in out:
                out["voxels_over_shapes"] = {k: round(out["voxels"][k] / out["shapes"][k], 1) for k in ("host_ms", "device_ms", "wall_ms")}
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
