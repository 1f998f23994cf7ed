"""numpy restatement of rt_draw_stamps (include/rt_abi.h "Voxel-model entities").  Test infrastructure.

No cull: every model is tested against every pixel (in blocks of models, for memory's sake only), and every pixel whose ray enters a
model's bounding box walks that model's cells by the header's words, operation by operation in float32.  The direction, the slab test,
fma, length3, unorm, f2u16 and albedo_rgba8 are tests/draw_boxes_ref.py's; the orientation is tests/stamp_edits.oriented(), built from
np.transpose and np.flip alone — not from strides, as the library's is.

`stamps` maps a stamp id to (materials u32[ez, ey, ex], state u8[ez, ey, ex]); `models` holds MODEL_DTYPE records (RtDrawStamp's 32
bytes).  draw_stamps(planes, u, models, stamps, lights, width, height) takes the frame's planes as Context.readback_all /
pyoracle.render return them and returns new planes; planes it does not write are passed through as they are.  walk_stats() tells what
the last winners() call walked: pairs of (model, pixel) that entered a bounding box and the steps they took."""
import numpy as np

from tests import draw_boxes_ref as boxes_ref
from tests import stamp_edits as se
from tests.draw_boxes_ref import albedo_rgba8, f2u16, fma, length3, unorm

f32 = np.float32
MAX_COORD = f32(4194304.0)
MIN_SCALE, MAX_SCALE = f32(1.0 / 256.0), f32(64.0)
MAX_MODELS = 4096
MODEL_DTYPE = np.dtype([("origin", "<f4", 3), ("scale", "<f4"), ("stamp", "<u4"), ("orient", "u1"), ("reserved0", "u1", 3),
                        ("emission", "<u4"), ("reserved", "<u4")])
assert MODEL_DTYPE.itemsize == 32

_stats = {"pairs": 0, "steps": 0, "max_steps": 0, "bound_ok": True}


def walk_stats():
    return dict(_stats)


def model(stamp, origin, scale=1.0, orient=0, emission=0xFF000000):
    m = np.zeros((), MODEL_DTYPE)
    m["stamp"], m["origin"], m["scale"], m["orient"], m["emission"] = stamp, origin, scale, orient, emission
    return m


def batch(models):
    return np.array([np.asarray(m, dtype=MODEL_DTYPE) for m in models], dtype=MODEL_DTYPE).reshape(-1)


def placed_extents(models, stamps):
    """E'[N, 3] (x, y, z) of records that name a known stamp with orient < 48; 1 elsewhere."""
    out = np.ones((models.size, 3), dtype=np.int64)
    for i, m in enumerate(models):
        if int(m["stamp"]) in stamps and m["orient"] < 48:
            out[i] = se.placed_extent(se.extent_of(stamps[int(m["stamp"])][1]), int(m["orient"]))
    return out


def high_corners(models, ext):
    """hi_k = rtm_fma(float(E'_k), scale, origin_k)."""
    with np.errstate(all="ignore"):
        return fma(ext.astype(f32), np.repeat(models["scale"].astype(f32)[:, None], 3, axis=1), models["origin"].astype(f32))


def valid(models, stamps):
    """The header's valid record, per record."""
    models = np.asarray(models, dtype=MODEL_DTYPE).reshape(-1)
    ext = placed_extents(models, stamps)
    known = np.array([int(s) in stamps for s in models["stamp"]], dtype=bool).reshape(-1)
    with np.errstate(invalid="ignore"):
        ok = known & (models["orient"] < 48) & (models["reserved0"] == 0).all(axis=1) & (models["reserved"] == 0)
        ok &= (models["scale"] >= MIN_SCALE) & (models["scale"] <= MAX_SCALE)
        ok &= (np.abs(models["origin"]) <= MAX_COORD).all(axis=1)
        ok &= (np.abs(high_corners(models, ext)) <= MAX_COORD).all(axis=1)
    return ok


def _walk(o, d, inv, t_in, axis, origin, scale, ext, off, state_flat):
    """The header's first cell and walk for n (model, pixel) pairs at once: d, inv, origin [n, 3]; t_in, scale [n]; axis [n]; ext [n, 3]
    = E'; off [n] = where the pair's model starts in state_flat (its oriented state array, [z, y, x] flattened).  Returns
    (found[n], t[n], axis[n], cell index into state_flat [n], steps[n])."""
    n = t_in.shape[0]
    c = np.zeros((n, 3), dtype=np.int64)
    with np.errstate(all="ignore"):
        for k in range(3):
            p = np.where(d[:, k] == 0, o[k], fma(d[:, k], t_in, np.full(n, o[k], dtype=f32)))
            q = np.floor(((p - origin[:, k]).astype(f32) / scale).astype(f32))
            q = np.where(q > 0, np.minimum(q, (ext[:, k] - 1).astype(f32)), f32(0.0))         # clamp(int(.), 0, E' - 1)
            c[:, k] = np.where(axis == k, np.where(d[:, k] > 0, 0, ext[:, k] - 1), q.astype(np.int64))
    t = t_in.copy()
    axis = axis.astype(np.int64).copy()
    found = np.zeros(n, dtype=bool)
    steps = np.zeros(n, dtype=np.int64)
    cell = np.zeros(n, dtype=np.int64)
    live = np.arange(n)
    bound = ext.sum(axis=1)
    while live.size:
        e, cc = ext[live], c[live]
        idx = off[live] + (cc[:, 2] * e[:, 1] + cc[:, 1]) * e[:, 0] + cc[:, 0]
        solid = state_flat[idx] == se.SOLID
        found[live[solid]] = True
        cell[live[solid]] = idx[solid]
        live = live[~solid]
        if not live.size:
            break
        if (steps[live] >= bound[live]).any():
            _stats["bound_ok"] = False
            raise AssertionError("a walk passed E'x + E'y + E'z steps")
        steps[live] += 1
        cc, dd = c[live], d[live]
        have = np.zeros(live.size, dtype=bool)
        tmin = np.zeros(live.size, dtype=f32)
        ax = np.zeros(live.size, dtype=np.int64)
        with np.errstate(all="ignore"):
            for k in range(3):
                nz = dd[:, k] != 0
                i = (cc[:, k] + (dd[:, k] > 0)).astype(f32)
                w = fma(i, scale[live], origin[live, k])
                tk = ((w - o[k]).astype(f32) * inv[live, k]).astype(f32)
                take = nz & (~have | (tk < tmin))
                tmin = np.where(take, tk, tmin)
                ax = np.where(take, k, ax)
                have |= nz
        rows = np.arange(live.size)
        cc[rows, ax] += np.where(dd[rows, ax] > 0, 1, -1)
        inside = have & (cc[rows, ax] >= 0) & (cc[rows, ax] < ext[live][rows, ax])
        c[live] = cc
        with np.errstate(invalid="ignore"):
            t[live] = np.where(inside & (t[live] < tmin), tmin, t[live])
        axis[live] = np.where(inside, ax, axis[live])
        live = live[inside]
    return found, t, axis, cell, steps


def winners(u, models, stamps, width, height, block=32):
    """(t[H, W] float32, index[H, W] int64 (-1: none), axis[H, W] int64, material[H, W] uint32, d[H, W, 3]) of the model every pixel's
    ray hits first: the smallest t, on equal t the lowest index."""
    models = np.asarray(models, dtype=MODEL_DTYPE).reshape(-1)
    d = boxes_ref.directions(u, width, height)
    o = np.array([u.origin[0], u.origin[1], u.origin[2]], dtype=f32)
    ok = valid(models, stamps)
    ext_all = placed_extents(models, stamps)
    hi_all = high_corners(models, ext_all)
    best_t = np.full((height, width), np.inf, dtype=f32)
    best_i = np.full((height, width), -1, dtype=np.int64)
    best_a = np.zeros((height, width), dtype=np.int64)
    best_m = np.zeros((height, width), dtype=np.uint32)
    _stats.update(pairs=0, steps=0, max_steps=0, bound_ok=True)
    oriented = {}
    with np.errstate(all="ignore"):
        inv = (f32(1.0) / d).astype(f32)
        plain = bool((d != 0).all() and np.isfinite(inv).all() and np.isfinite(o).all())
        for first in range(0, models.size, block):
            sel = np.arange(first, min(first + block, models.size))
            lo, hi = models["origin"][sel].astype(f32), hi_all[sel]
            if plain and ok[sel].all():                                  # (draw_boxes_ref's shorter way through plain frames)
                t_in, t_out, axis, alive = boxes_ref._slab_plain(lo, hi, o, inv)
            else:
                t_in, t_out, axis, alive = boxes_ref._slab_general(lo, hi, o, d, inv, (sel.size, height, width))
            enters = (t_in > 0) & (t_in < t_out) & alive & ok[sel][:, None, None]
            mi, py, px = np.nonzero(enters)
            if not mi.size:
                continue
            # the oriented arrays of the block's models, one after the other
            offs, flat_state, flat_mats, at = np.zeros(sel.size, dtype=np.int64), [], [], 0
            for j, i in enumerate(sel):
                if not ok[i]:
                    continue
                key = (int(models["stamp"][i]), int(models["orient"][i]))
                if key not in oriented:
                    mats, state = stamps[key[0]]
                    oriented[key] = (np.ascontiguousarray(se.oriented(np.asarray(mats, dtype=np.uint32), key[1])).reshape(-1),
                                     np.ascontiguousarray(se.oriented(np.asarray(state, dtype=np.uint8), key[1])).reshape(-1))
                offs[j] = at
                flat_mats.append(oriented[key][0])
                flat_state.append(oriented[key][1])
                at += oriented[key][1].size
            flat_state, flat_mats = np.concatenate(flat_state), np.concatenate(flat_mats)
            found, t, ax, cell, steps = _walk(o, d[py, px], inv[py, px], t_in[mi, py, px], axis[mi, py, px], lo[mi],
                                              models["scale"][sel].astype(f32)[mi], ext_all[sel][mi], offs[mi], flat_state)
            _stats["pairs"] += int(mi.size)
            _stats["steps"] += int(steps.sum())
            _stats["max_steps"] = max(_stats["max_steps"], int(steps.max()))
            mi, py, px, t, ax, cell = mi[found], py[found], px[found], t[found], ax[found], cell[found]
            # per pixel the smallest t, then the lowest index; against earlier blocks strictly smaller
            order = np.lexsort((mi, t, py * width + px))
            pix = (py * width + px)[order]
            firsts = order[np.concatenate([[True], pix[1:] != pix[:-1]])] if order.size else order
            y, x = py[firsts], px[firsts]
            better = t[firsts] < best_t[y, x]
            y, x, f = y[better], x[better], firsts[better]
            best_t[y, x], best_i[y, x], best_a[y, x], best_m[y, x] = t[f], sel[mi[f]], ax[f], flat_mats[cell[f]]
    return best_t, best_i, best_a, best_m, d


def draw_stamps(planes, u, models, stamps, lights, width, height, won=None):
    """The planes after rt_draw_stamps(u, models, lights) on `planes` (`won`: what winners() returned for these arguments, if the
    caller has it already)."""
    out = {name: np.array(p, copy=True) for name, p in planes.items()}
    models = np.asarray(models, dtype=MODEL_DTYPE).reshape(-1)
    if models.size == 0:
        return out
    light = np.asarray(lights).reshape(-1)["light"].astype(f32).reshape(-1, 3)
    assert light.shape[0] == 6 * models.size
    t_hit, idx, axis, material, d = won if won is not None else winners(u, models, stamps, width, height)
    o = np.array([u.origin[0], u.origin[1], u.origin[2]], dtype=f32)
    with np.errstate(all="ignore"):
        t = np.where(idx >= 0, t_hit, f32(0.0)).astype(f32)
        P = [fma(d[..., k], t, np.full_like(t, o[k])) for k in range(3)]
        depth_f = (length3((o[0] - P[0]).astype(f32), (o[1] - P[1]).astype(f32), (o[2] - P[2]).astype(f32)) * f32(32.0)).astype(f32)
        drawn = (idx >= 0) & (depth_f < planes["depth_f32"])
    d_a = np.take_along_axis(d, axis[..., None], axis=-1)[..., 0]
    normal = 2 * axis + (d_a > 0)
    b = np.where(drawn, idx, 0)
    out["depth_f32"][drawn] = depth_f[drawn]
    out["depth_r16"][drawn] = f2u16(depth_f)[drawn]
    out["normal_r8"][drawn] = normal[drawn].astype(np.uint8)
    out["albedo_rgba8"][drawn] = albedo_rgba8(material)[drawn]
    em = models["emission"][b].astype(np.uint32)
    out["emission_rgba8"][drawn] = np.stack([(em >> s) & 0xFF for s in (0, 8, 16, 24)], axis=-1).astype(np.uint8)[drawn]
    # store_lighting(sum = light, spp = 1): (light / 1.0f) / 16 and 1 / 16, then UNORM16
    with np.errstate(all="ignore"):
        L = light[6 * b + normal]
        lv = np.concatenate([((L / f32(1.0)).astype(f32) / f32(16.0)).astype(f32), np.full(L.shape[:-1] + (1,), f32(1.0) / f32(16.0), dtype=f32)], axis=-1)
    out["lighting_f32"][drawn] = lv[drawn]
    out["lighting_rgba16"][drawn] = unorm(lv, 65535.0).astype(np.uint16)[drawn]
    return out


def bounding_boxes(models, stamps, materials=0):
    """The models' bounding boxes as rt_draw_boxes records (lo = origin, hi as the header gives it, the models' emission words)."""
    from raytrace_amd import render
    models = np.asarray(models, dtype=MODEL_DTYPE).reshape(-1)
    b = np.zeros(models.size, dtype=render.DRAW_BOX_DTYPE)
    b["lo"], b["hi"] = models["origin"], high_corners(models, placed_extents(models, stamps))
    b["material"] = np.broadcast_to(np.asarray(materials, dtype=np.uint32), (models.size,))
    b["emission"] = models["emission"]
    return b
