"""Voxel stamps on the MI355X beside rt_edit_voxels fed with the same voxels enumerated (DESIGN.md "Voxel stamps").

    python tools/stamp_bench.py [--calls 24] [--warmup 3] [--rounds 3] [--out profiles/stamps_bench.txt]

64 copies of a 9 x 9 x 12 stamp (a third of its voxels ABSENT, the rest SOLID or AIR), each turned by its index, in an 8 x 8 grid over
the generated 256^3 world — through rt_edit_stamps (64 placements of 32 bytes) and, as one 16-byte record per selected voxel in
placement order, through rt_edit_voxels.  The records are made before the clock starts: the host's expansion of the stamp is not
counted against rt_edit_voxels.  Calls alternate between the stamp and its complement (SOLID and AIR swapped), so that every call
changes the world.  Per call: wall time from the call to rt_sync's return, and the device time of the call's two launches
(RT_FLAG_TIMING_ALL, rt_get_timing).  Per round and path the median over `calls` calls after `warmup` calls; the two paths alternate
round by round in one process; the spread is that of the rounds' medians.  Both paths leave the same region (checked once)."""
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
E = (9, 9, 12)
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


def stamp_pair():
    """(materials, state) and the complement's state."""
    rng = np.random.default_rng(9)
    r = rng.random((E[2], E[1], E[0]))
    state = np.where(r < 1 / 3, abi.RT_STAMP_ABSENT, np.where(r < 2 / 3, abi.RT_STAMP_AIR, abi.RT_STAMP_SOLID)).astype(np.uint8)
    other = np.where(state == abi.RT_STAMP_AIR, abi.RT_STAMP_SOLID, np.where(state == abi.RT_STAMP_SOLID, abi.RT_STAMP_AIR, state)).astype(np.uint8)
    mats = rng.integers(1, 2 ** 32, size=state.shape, dtype=np.uint64).astype(np.uint32)
    return mats, state, other


def oriented(arr, orient):
    """include/rt_abi.h's orientation rule with np.flip / np.transpose."""
    perm, f = PERMS[orient >> 3], orient & 7
    for j in range(3):
        if (f >> j) & 1:
            arr = np.flip(arr, axis=2 - j)
    axes = [0, 0, 0]
    for k in range(3):
        axes[2 - k] = 2 - perm[k]
    return np.transpose(arr, axes)


def placements():
    """(at, orient) of the 64 copies: 30 texels apart, round the terrain's surface."""
    return [((8 + 30 * (i % 8), 8 + 30 * (i // 8), 120 + 3 * (i % 5)), i % 48) for i in range(64)]


def records(mats, state):
    """RtVoxelEdit rows of the 64 placements' selected voxels (where = ALL: every voxel that is not ABSENT), in placement order."""
    rows = []
    for at, orient in placements():
        s, m = oriented(state, orient), oriented(mats, orient)
        z, y, x = np.nonzero(s != abi.RT_STAMP_ABSENT)
        r = np.zeros(len(x), dtype=[("x", "<u2"), ("y", "<u2"), ("z", "<u2"), ("solid", "<u2"), ("material", "<u4"), ("reserved", "<u4")])
        r["x"], r["y"], r["z"] = x + at[0], y + at[1], z + at[2]
        r["solid"], r["material"] = s[z, y, x] == abi.RT_STAMP_SOLID, m[z, y, x]
        rows.append(r)
    return np.concatenate(rows)


def one_round(ctx, call, calls, warmup):
    """(wall ms, device ms) medians over `calls` calls, each synchronised."""
    for i in range(warmup):
        call(i & 1)
        ctx.sync()
    ctx.timing()                                   # drains the launch timers
    wall, dev = [], []
    for i in range(calls):
        t0 = time.perf_counter()
        call((warmup + i) & 1)
        ctx.sync()
        wall.append(1e3 * (time.perf_counter() - t0))
        tm = ctx.timing()
        assert tm.other_launches == 2, tm.other_launches
        dev.append(tm.shade_ms)
    return float(np.median(wall)), float(np.median(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mats, state, other = stamp_pair()
    recs = [records(mats, state), records(mats, other)]
    region = world.generate_region(world.DEFAULT_SEED)
    noise = np.fromfile(os.path.join(ROOT, "tests", "golden", "blue_noise_512.rgba"), dtype=np.uint8)
    results = {"stamps": [], "voxels": []}
    with render.Context(render.make_config(64, 64, flags=abi.RT_FLAG_TIMING_ALL)) as ctx, \
            render.Context(render.make_config(64, 64, flags=abi.RT_FLAG_TIMING_ALL)) as ref:
        for c in (ctx, ref):
            c.upload_world(*region)
            c.upload_noise(noise)
            c.draw_frame(render.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, 0.0))   # (rt_get_timing asks for a frame)
            c.sync()
        ids = [ctx.stamp_create(mats, state), ctx.stamp_create(mats, other)]
        rows = [np.array([render.stamp_place(sid, at, orient) for at, orient in placements()], dtype=render.STAMP_PLACE_DTYPE) for sid in ids]
        sptr = [r.ctypes.data_as(C.POINTER(abi.RtStampPlace)) for r in rows]
        vptr = [r.ctypes.data_as(C.POINTER(abi.RtVoxelEdit)) for r in recs]
        paths = {"stamps": (ctx, lambda i: ctx._check(ctx._lib.rt_edit_stamps(ctx.handle, sptr[i], 64))),
                 "voxels": (ref, lambda i: ref._check(ref._lib.rt_edit_voxels(ref.handle, vptr[i], len(recs[i]))))}
        # the two paths compute the same region
        for c, call in paths.values():
            call(0)
        a_m, a_f = ctx.read_box((0, 0, 0), (R, R, R))
        b_m, b_f = ref.read_box((0, 0, 0), (R, R, R))
        same = bool(np.array_equal(a_f, b_f) and np.array_equal(a_m, b_m) and not np.array_equal(a_f, region[1]))
        for _ in range(a.rounds):
            for name, (c, call) in paths.items():
                results[name].append(one_round(c, call, a.calls, a.warmup))
    lines = ["# tools/stamp_bench.py: 64 placements of a 9 x 9 x 12 stamp (%d of its %d voxels ABSENT) over the generated 256^3 world, through" % (
                 int(np.count_nonzero(state == 0)), state.size),
             "# rt_edit_stamps (64 x 32 bytes) and through rt_edit_voxels (%d records x 16 bytes, made before the clock starts)." % len(recs[0]),
             "# Per round: the median over %d calls after %d warm-up calls, each call timed from the call to rt_sync's return (wall) and by" % (a.calls, a.warmup),
             "# the events round its two launches (device); %d rounds per path, alternating, in one process.  Same region from both paths: %s." % (a.rounds, same),
             "path     figure      median_ms  rounds_ms                      spread_ms"]
    summary = {"same_region": same, "records": int(len(recs[0]))}
    for name in ("stamps", "voxels"):
        arr = np.array(results[name])
        for k, fig in enumerate(("wall", "device")):
            v = arr[:, k]
            lines.append("%-8s %-10s %10.4f  %-30s %.4f" % (name, fig, float(np.median(v)), " ".join("%.4f" % x for x in v), float(v.max() - v.min())))
            summary["%s_%s_ms" % (name, fig)] = round(float(np.median(v)), 4)
            summary["%s_%s_spread_ms" % (name, fig)] = round(float(v.max() - v.min()), 4)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
