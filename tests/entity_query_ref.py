"""numpy restatement of the entity part of rt_trace_entities / rt_pick_entities (include/rt_abi.h "Entity queries").  Test infrastructure.

Written from the header's words for arbitrary rays with per-ray origins: no cull, every entity against every ray — the slab tests in
blocks of records against every ray of the batch at once (for memory's sake only), the walks one model at a time.  Every operation is a float32 array operation rounded on its own; the fused ones (P = rtm_fma(d, t, o),
the planes rtm_fma(float(i), scale, origin_k), the two of rtm_length3) go through the exact fma emulation the drawing references use.
It shares the scalar helpers fma, length3 and directions with tests/draw_boxes_ref.py and the orientation with tests/stamp_edits.oriented;
the slab test, the first cell, the walk and the choice of the winner are restated here and owe nothing to draw_stamps_ref._walk or to
either winners(): tests/test_entity_query_contract.py holds the two restatements against each other.

The world part is an input: `world_hits` are HIT_DTYPE records from the device or from tests/ray_query_ref.py.

    trace(origins, directions, world_hits, boxes, models, stamps)       -> ENTITY_HIT_DTYPE[N]    (rt_trace_entities)
    pick(u, xy, width, height, world_hits, boxes, models, stamps)       -> ENTITY_HIT_DTYPE[N]    (rt_pick_entities)
    winners(o, d, boxes, models, stamps)                                -> the nearest entity per ray before the depth test

`stamps` maps a stamp id to (materials u32[ez, ey, ex], state u8[ez, ey, ex]); boxes are RtDrawBox records, models RtDrawStamp records."""
import numpy as np

from tests import stamp_edits as se
from tests.draw_boxes_ref import directions, fma, length3

f32 = np.float32
MAX_COORD = f32(4194304.0)
MIN_SCALE, MAX_SCALE = f32(1.0 / 256.0), f32(64.0)
NONE, BOX, MODEL = 0, 1, 2
HIT_AIR = 0
ENTITY_HIT_DTYPE = np.dtype([("position", "<f4", 3), ("t", "<f4"), ("kind", "<u4"), ("index", "<u4"), ("normal", "<u4"), ("material", "<u4"),
                             ("cell", "<i4", 3), ("voxel", "<u4")])
assert ENTITY_HIT_DTYPE.itemsize == 48


def normalize3(v):
    """rtm_normalize3 per row: v * (1.0f / rtm_length3(v))."""
    v = np.asarray(v, dtype=f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        r = (f32(1.0) / length3(v[:, 0], v[:, 1], v[:, 2])).astype(f32)
        return (v * r[:, None]).astype(f32)


def box_valid(lo, hi):
    """rt_draw_boxes' valid box."""
    with np.errstate(invalid="ignore"):
        return bool(((np.abs(lo) <= MAX_COORD) & (np.abs(hi) <= MAX_COORD) & (lo < hi)).all())


def model_valid(m, stamps):
    """rt_draw_stamps' valid record."""
    if int(m["stamp"]) not in stamps or m["orient"] >= 48 or m["reserved0"].any() or m["reserved"] != 0:
        return False
    with np.errstate(invalid="ignore"):
        if not (m["scale"] >= MIN_SCALE and m["scale"] <= MAX_SCALE):
            return False
        ext = np.array(se.placed_extent(se.extent_of(stamps[int(m["stamp"])][1]), int(m["orient"])), dtype=f32)
        hi = fma(ext, np.full(3, m["scale"], dtype=f32), m["origin"].astype(f32))
        return bool((np.abs(m["origin"]) <= MAX_COORD).all() and (np.abs(hi) <= MAX_COORD).all())


def slab(lo, hi, o, d, inv):
    """The slab test of B boxes (lo, hi [B, 3]) against N rays: (hit, t_in, t_out, axis), each [B, N]."""
    lo, hi = np.asarray(lo, dtype=f32).reshape(-1, 3), np.asarray(hi, dtype=f32).reshape(-1, 3)
    shape = (lo.shape[0], o.shape[0])
    bounded = np.zeros(shape, dtype=bool)
    miss = np.zeros(shape, dtype=bool)
    t_in = np.zeros(shape, dtype=f32)
    t_out = np.zeros(shape, dtype=f32)
    axis = np.zeros(shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        for k in range(3):
            nz = np.broadcast_to((d[:, k] != 0)[None, :], shape)
            ok, ik, lk, hk = o[None, :, k], inv[None, :, k], lo[:, None, k], hi[:, None, k]
            t0 = ((lk - ok).astype(f32) * ik).astype(f32)
            t1 = ((hk - ok).astype(f32) * ik).astype(f32)
            tn = np.where(t1 < t0, t1, t0)                                   # rtm_min(t0, t1) = t1 < t0 ? t1 : t0
            tf = np.where(t0 < t1, t1, t0)                                   # rtm_max(t0, t1) = t0 < t1 ? t1 : t0
            first = nz & ~bounded
            new_in = first | (nz & bounded & (tn > t_in))
            new_out = first | (nz & bounded & (tf < t_out))
            t_in = np.where(new_in, tn, t_in)
            axis = np.where(new_in, k, axis)
            t_out = np.where(new_out, tf, t_out)
            bounded = bounded | nz
            miss |= ~nz & ~((lk < ok) & (ok < hk))
        hit = bounded & ~miss & (t_in > 0) & (t_in < t_out)
    return hit, t_in, t_out, axis


def walk(o, d, inv, t_in, axis, origin, scale, ext, state):
    """First cell and walk of one model for the n rays that enter its bounding box: state is the placed array [z, y, x], ext = E'
    (x, y, z).  Returns (found[n], t[n], axis[n], cell[n, 3])."""
    n = t_in.shape[0]
    c = np.zeros((n, 3), dtype=np.int64)
    with np.errstate(all="ignore"):
        for k in range(3):
            p = np.where(d[:, k] == 0, o[:, k], fma(d[:, k], t_in, o[:, k]))
            q = np.floor(((p - origin[k]).astype(f32) / scale).astype(f32))
            q = np.where(q > 0, np.where(q > f32(ext[k] - 1), f32(ext[k] - 1), q), f32(0.0))    # clamp(int(.), 0, E'_k - 1)
            c[:, k] = np.where(axis == k, np.where(d[:, k] > 0, 0, ext[k] - 1), q.astype(np.int64))
    t = t_in.astype(f32).copy()
    axis = axis.copy()
    found = np.zeros(n, dtype=bool)
    live = np.arange(n)
    for _ in range(int(ext[0] + ext[1] + ext[2]) + 1):
        if not live.size:
            break
        cc = c[live]
        solid = state[cc[:, 2], cc[:, 1], cc[:, 0]] == se.SOLID                  # (1) AIR and ABSENT are see-through
        found[live[solid]] = True
        live = live[~solid]
        if not live.size:
            break
        cc, dd, oo, ii = c[live], d[live], o[live], inv[live]
        have = np.zeros(live.size, dtype=bool)
        tmin = np.zeros(live.size, dtype=f32)
        ax = np.zeros(live.size, dtype=np.int64)
        with np.errstate(all="ignore"):
            for k in range(3):                                                   # (2) the lowest axis wins ties
                nz = dd[:, k] != 0
                w = fma((cc[:, k] + (dd[:, k] > 0)).astype(f32), np.full(live.size, scale, dtype=f32), np.full(live.size, origin[k], dtype=f32))
                tk = ((w - oo[:, k]).astype(f32) * ii[:, k]).astype(f32)
                take = nz & (~have | (tk < tmin))
                tmin = np.where(take, tk, tmin)
                ax = np.where(take, k, ax)
                have |= nz
            rows = np.arange(live.size)
            cc[rows, ax] += np.where(dd[rows, ax] > 0, 1, -1)                    # (3)
            inside = have & (cc[rows, ax] >= 0) & (cc[rows, ax] < np.asarray(ext)[ax])
            keep = live[inside]
            c[keep] = cc[inside]
            t[keep] = np.where(t[keep] < tmin[inside], tmin[inside], t[keep])    # (4)
            axis[keep] = ax[inside]
        live = keep
    assert not live.size, "a walk passed E'x + E'y + E'z steps"
    return found, t, axis, c


def winners(o, d, boxes, models, stamps):
    """The nearest entity of every ray before the depth test: dict of t[N] float32, kind[N], index[N] (-1: none), axis[N], material[N],
    cell[N, 3], voxel[N].  The smallest t over boxes and models together; on equal t a box before a model, then the lowest index."""
    o = np.asarray(o, dtype=f32).reshape(-1, 3)
    d = np.asarray(d, dtype=f32).reshape(-1, 3)
    n = o.shape[0]
    boxes = np.asarray(boxes).reshape(-1) if boxes is not None else np.zeros(0)
    models = np.asarray(models).reshape(-1) if models is not None else np.zeros(0)
    w = {"t": np.full(n, np.inf, dtype=f32), "kind": np.zeros(n, dtype=np.uint32), "index": np.full(n, -1, dtype=np.int64),
         "axis": np.zeros(n, dtype=np.int64), "material": np.zeros(n, dtype=np.uint32), "cell": np.full((n, 3), -1, dtype=np.int64),
         "voxel": np.full(n, 0xFFFFFFFF, dtype=np.int64)}
    with np.errstate(all="ignore"):
        inv = (f32(1.0) / d).astype(f32)
    block = max(1, (1 << 21) // max(n, 1))                                  # boxes at a time, for memory's sake only
    for first in range(0, boxes.size, block):
        part = boxes[first:first + block]
        lo, hi = part["lo"].astype(f32), part["hi"].astype(f32)
        ok = np.array([box_valid(lo[j], hi[j]) for j in range(part.size)], dtype=bool)
        hit, t_in, _, axis = slab(lo, hi, o, d, inv)
        t_hit = np.where(hit & ok[:, None], t_in, f32(np.inf))
        j = np.argmin(t_hit, axis=0)                                         # the first of equal minima: the lowest index
        rays = np.arange(n)
        better = t_hit[j, rays] < w["t"]                                     # strict: a box of an earlier block keeps a tie
        w["t"][better], w["kind"][better], w["index"][better] = t_hit[j, rays][better], BOX, first + j[better]
        w["axis"][better], w["material"][better] = axis[j, rays][better], part["material"][j[better]]
    placed, exts = {}, {}
    for m in range(models.size):
        assert model_valid(models[m], stamps), "the calls refuse an invalid model on the host"
        key = (int(models["stamp"][m]), int(models["orient"][m]))
        if key not in placed:
            mats, state = stamps[key[0]]
            state = np.asarray(state, dtype=np.uint8)
            placed[key] = (se.oriented(state, key[1]), se.oriented(np.arange(state.size, dtype=np.int64).reshape(state.shape), key[1]),
                           np.asarray(mats, dtype=np.uint32).reshape(-1))
        exts[m] = se.extent_of(placed[key][0])
    for first in range(0, models.size, block):
        sel_m = np.arange(first, min(first + block, models.size))
        origin_all, scale_all = models["origin"][sel_m].astype(f32), models["scale"][sel_m].astype(f32)
        with np.errstate(all="ignore"):
            hi_all = fma(np.array([exts[m] for m in sel_m], dtype=f32), np.repeat(scale_all[:, None], 3, axis=1), origin_all)
        enters_all, t_in_all, _, axis_all = slab(origin_all, hi_all, o, d, inv)
        for j, m in enumerate(sel_m):                                        # in index order: on equal t the lowest index keeps the hit
            sel = np.nonzero(enters_all[j])[0]
            if not sel.size:
                continue
            state, voxel_of, mats = placed[(int(models["stamp"][m]), int(models["orient"][m]))]
            found, t, ax, c = walk(o[sel], d[sel], inv[sel], t_in_all[j, sel], axis_all[j, sel], origin_all[j], scale_all[j], exts[m], state)
            better = found & (t < w["t"][sel])
            s, c = sel[better], c[better]
            vox = voxel_of[c[:, 2], c[:, 1], c[:, 0]]
            w["t"][s], w["kind"][s], w["index"][s], w["axis"][s] = t[better], MODEL, m, ax[better]
            w["material"][s], w["cell"][s], w["voxel"][s] = mats[vox], c, vox
    return w


def world_depth(o, world_hits):
    """D per ray: 65535.0f under the sky, else rtm_length3(o - world position as returned) * 32.0f."""
    o = np.asarray(o, dtype=f32).reshape(-1, 3)
    p = world_hits["position"].astype(f32)
    with np.errstate(all="ignore"):
        diff = (o - p).astype(f32)
        D = (length3(diff[:, 0], diff[:, 1], diff[:, 2]) * f32(32.0)).astype(f32)
    return np.where(world_hits["kind"] == HIT_AIR, f32(65535.0), D).astype(f32)


def records(o, d, D, won):
    """The records of the call: the depth test of every ray's winner against D, then the reported or the empty record."""
    n = o.shape[0]
    out = np.zeros(n, dtype=ENTITY_HIT_DTYPE)
    out["index"], out["normal"], out["cell"], out["voxel"] = 0xFFFFFFFF, 6, -1, 0xFFFFFFFF
    has = won["index"] >= 0
    with np.errstate(all="ignore"):
        t = np.where(has, won["t"], f32(0.0)).astype(f32)
        P = np.stack([fma(d[:, k], t, o[:, k]) for k in range(3)], axis=-1)
        diff = (o - P).astype(f32)
        depth_f = (length3(diff[:, 0], diff[:, 1], diff[:, 2]) * f32(32.0)).astype(f32)
        shown = has & (depth_f < D)
    d_a = np.take_along_axis(d, won["axis"][:, None], axis=1)[:, 0]
    normal = 2 * won["axis"] + (d_a > 0)
    out["position"][shown], out["t"][shown] = P[shown], t[shown]
    out["kind"][shown], out["index"][shown], out["normal"][shown] = won["kind"][shown], won["index"][shown], normal[shown]
    out["material"][shown] = won["material"][shown]
    is_model = shown & (won["kind"] == MODEL)
    out["cell"][is_model], out["voxel"][is_model] = won["cell"][is_model], won["voxel"][is_model]
    return out, depth_f, has


def trace(origins, dirs, world_hits, boxes=None, models=None, stamps=None, details=False):
    """rt_trace_entities' entity_hits for rays (origins, dirs) whose world hits are `world_hits`."""
    o = np.ascontiguousarray(origins, dtype=f32).reshape(-1, 3)
    d = normalize3(dirs)
    return _answer(o, d, world_hits, boxes, models, stamps or {}, details)


def pick(u, xy, width, height, world_hits, boxes=None, models=None, stamps=None, details=False):
    """rt_pick_entities' entity_hits for the pixels xy of the camera in `u`: the ray of rt_draw_boxes, o = u.origin, no slide."""
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    d = directions(u, width, height)[xy[:, 1], xy[:, 0]]
    o = np.repeat(np.array([[u.origin[0], u.origin[1], u.origin[2]]], dtype=f32), xy.shape[0], axis=0)
    return _answer(o, d, world_hits, boxes, models, stamps or {}, details)


def _answer(o, d, world_hits, boxes, models, stamps, details):
    won = winners(o, d, boxes, models, stamps)
    D = world_depth(o, world_hits)
    out, depth_f, has = records(o, d, D, won)
    if details:   # what the tests assert about their own inputs: rays with a hit, occluded ones, reported ones under the sky
        shown = out["kind"] != NONE
        return out, {"hit": has, "occluded": has & ~shown, "under_sky": shown & (world_hits["kind"] == HIT_AIR), "D": D, "depth_f": depth_f}
    return out
