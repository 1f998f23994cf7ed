"""numpy restatement of rt_add_lights_occluded (include/rt_abi.h "Point-light shadows of entities").  Test infrastructure.

No cull: every valid box and every model is tested against every (pixel, light) pair that passed rt_add_lights' pair test (in blocks
of lights and of occluders, for memory's sake only); a pair no entity blocks gets the world's shadow ray.  Every operation is a
float32 array operation rounded on its own; the contract's fused operations go through the exact fma emulation of
tests/denoise_history_ref.py.

The pair test, the surface point, the world's shadow ray and the valid light are tests/point_light_ref's, unchanged; rtm_min / rtm_max,
the valid box and the placed extents are tests/entity_shadow_ref's, tests/draw_boxes_ref's and tests/draw_stamps_ref's.  The slab test
is restated here once more, because here both the origin and the direction differ per pair, and so are the first cell and the walk
with its added stop at the light.

add_lights_occluded(planes, u, lights, boxes, models, stamps, minefield, width, height) takes the frame's planes as
Context.readback_all returns them and returns new planes; planes it does not write are passed through as they are.  `stamps` maps a
stamp id to (materials, state[ez, ey, ex]) as for tests/draw_stamps_ref."""
import numpy as np

from tests import draw_boxes_ref as boxes_ref
from tests import draw_stamps_ref as stamps_ref
from tests import point_light_ref as pl
from tests import stamp_edits as se
from tests.denoise_history_ref import fma
from tests.draw_boxes_ref import length3, unorm
from tests.entity_shadow_ref import _rmax, _rmin

f32 = np.float32
WRITTEN = pl.WRITTEN
MODEL_DTYPE = stamps_ref.MODEL_DTYPE


def segments(v, dist2):
    """(d[n, 3], inv[n, 3], len[n]) of the pairs' segments: d = rtm_normalize3(v) as trace_visible computes it, inv_k = 1.0f / d_k,
    len = rtm_sqrt(dist2)."""
    with np.errstate(all="ignore"):
        rlen = (f32(1.0) / length3(v[:, 0], v[:, 1], v[:, 2])).astype(f32)
        d = (v * rlen[:, None]).astype(f32)
        inv = (f32(1.0) / d).astype(f32)
        ln = np.sqrt(dist2).astype(f32)
    return d, inv, ln


def slab(lo, hi, o, d, inv):
    """The slab test of the pairs (o[n, 3], d[n, 3], inv[n, 3]) against the boxes lo, hi [m, 3], operation by operation:
    (t_in[m, n], t_out[m, n], axis[m, n], some axis gave a bound & every zero-direction axis passes [m, n])."""
    m, n = lo.shape[0], o.shape[0]
    bounded = np.zeros((m, n), dtype=bool)
    miss = np.zeros((m, n), dtype=bool)
    t_in = np.zeros((m, n), dtype=f32)
    t_out = np.zeros((m, n), dtype=f32)
    axis = np.zeros((m, n), dtype=np.int8)
    with np.errstate(all="ignore"):
        for k in range(3):
            nz = np.broadcast_to((d[:, k] != 0)[None, :], (m, n))
            t0 = ((lo[:, k, None] - o[None, :, k]).astype(f32) * inv[None, :, k]).astype(f32)
            t1 = ((hi[:, k, None] - o[None, :, k]).astype(f32) * inv[None, :, k]).astype(f32)
            tn, tf = _rmin(t0, t1), _rmax(t0, t1)
            first = nz & ~bounded
            new_in = nz & bounded & (tn > t_in)
            new_out = nz & bounded & (tf < t_out)
            t_in = np.where(first | new_in, tn, t_in)
            axis = np.where(first | new_in, np.int8(k), axis)
            t_out = np.where(first | new_out, tf, t_out)
            bounded = bounded | nz
            miss |= ~nz & ~((lo[:, k, None] < o[None, :, k]) & (o[None, :, k] < hi[:, k, None]))
    return t_in, t_out, axis, bounded & ~miss


def crossed(lo, hi, o, d, inv, ln):
    """(blocks[m, n], t_in, axis): the box rule — some axis gave a bound, every zero axis passes, t_out > 0, t_in < t_out and
    t_in < len."""
    t_in, t_out, axis, ok = slab(lo, hi, o, d, inv)
    with np.errstate(invalid="ignore"):
        return ok & (t_out > 0) & (t_in < t_out) & (t_in < ln[None, :]), t_in, axis


def boxes_block(boxes, o, d, inv, ln, block=128):
    """blocked bool[n]: some valid box blocks the pair."""
    boxes = np.asarray(boxes).reshape(-1)
    out = np.zeros(o.shape[0], dtype=bool)
    ok = boxes_ref.valid(boxes) if boxes.size else np.zeros(0, dtype=bool)
    for first in range(0, boxes.size, block):
        sel = np.arange(first, min(first + block, boxes.size))[ok[first:first + block]]
        todo = np.nonzero(~out)[0]                      # (a boolean OR: a pair some box blocks needs no further box)
        if sel.size and todo.size:
            hit = crossed(boxes["lo"][sel].astype(f32), boxes["hi"][sel].astype(f32), o[todo], d[todo], inv[todo], ln[todo])[0].any(axis=0)
            out[todo[hit]] = True
    return out


def _walk(o, d, inv, ln, t_in, axis, origin, scale, ext, off, state_flat):
    """The first cell and the boolean walk for n (model, pair) pairs at once: o, d, inv, origin [n, 3]; ln, t_in, scale [n]; axis [n];
    ext [n, 3] = E'; off [n] = where the model starts in state_flat (its oriented state array, [z, y, x] flattened).  found[n]."""
    n = t_in.shape[0]
    c = np.zeros((n, 3), dtype=np.int64)
    with np.errstate(all="ignore"):
        outside = t_in > 0
        for k in range(3):
            entry = np.where(d[:, k] == 0, o[:, k], fma(d[:, k], t_in, o[:, k]))
            p = np.where(outside, entry, o[:, k]).astype(f32)
            q = np.floor(((p - origin[:, k]).astype(f32) / scale).astype(f32))
            q = np.where(q > 0, np.minimum(q, (ext[:, k] - 1).astype(f32)), f32(0.0))         # clamp(int(.), 0, E' - 1)
            c[:, k] = np.where(outside & (axis == k), np.where(d[:, k] > 0, 0, ext[:, k] - 1), q.astype(np.int64))
    found = np.zeros(n, dtype=bool)
    steps = np.zeros(n, dtype=np.int64)
    live = np.arange(n)
    bound = ext.sum(axis=1)
    while live.size:
        e, cc = ext[live], c[live]
        idx = off[live] + (cc[:, 2] * e[:, 1] + cc[:, 1]) * e[:, 0] + cc[:, 0]
        solid = state_flat[idx] == se.SOLID                                                   # (1)
        found[live[solid]] = True
        live = live[~solid]
        if not live.size:
            break
        if (steps[live] >= bound[live]).any():
            raise AssertionError("a walk passed E'x + E'y + E'z steps")
        steps[live] += 1
        cc, dd = c[live], d[live]
        have = np.zeros(live.size, dtype=bool)
        tmin = np.zeros(live.size, dtype=f32)
        ax = np.zeros(live.size, dtype=np.int64)
        with np.errstate(all="ignore"):
            for k in range(3):                                                                # (2)
                nz = dd[:, k] != 0
                i = (cc[:, k] + (dd[:, k] > 0)).astype(f32)
                w = fma(i, scale[live], origin[live, k])
                tk = ((w - o[live, k]).astype(f32) * inv[live, k]).astype(f32)
                take = nz & (~have | (tk < tmin))
                tmin = np.where(take, tk, tmin)
                ax = np.where(take, k, ax)
                have |= nz
            before = have & (tmin < ln[live])                                                 # the added stop: the light comes first
        rows = np.arange(live.size)
        cc[rows, ax] += np.where(dd[rows, ax] > 0, 1, -1)                                     # (3)
        inside = before & (cc[rows, ax] >= 0) & (cc[rows, ax] < ext[live][rows, ax])
        c[live] = cc
        live = live[inside]
    return found


def models_block(models, stamps, o, d, inv, ln, block=32):
    """blocked bool[n]: some model's walk along the pair's segment stops on a SOLID cell before the light.  Every record must be valid
    (the library rejects the call otherwise)."""
    models = np.asarray(models, dtype=MODEL_DTYPE).reshape(-1)
    out = np.zeros(o.shape[0], dtype=bool)
    if not models.size:
        return out
    assert stamps_ref.valid(models, stamps).all(), "an invalid model record: the library rejects the whole call"
    ext_all = stamps_ref.placed_extents(models, stamps)
    hi_all = stamps_ref.high_corners(models, ext_all)
    oriented = {}
    for first in range(0, models.size, block):
        sel = np.arange(first, min(first + block, models.size))
        todo = np.nonzero(~out)[0]
        if not todo.size:
            break
        lo, hi = models["origin"][sel].astype(f32), hi_all[sel]
        enters, t_in, axis = crossed(lo, hi, o[todo], d[todo], inv[todo], ln[todo])
        mi, pi = np.nonzero(enters)
        if not mi.size:
            continue
        offs, flat, at = np.zeros(sel.size, dtype=np.int64), [], 0
        for j, i in enumerate(sel):
            key = (int(models["stamp"][i]), int(models["orient"][i]))
            if key not in oriented:
                oriented[key] = np.ascontiguousarray(se.oriented(np.asarray(stamps[key[0]][1], dtype=np.uint8), key[1])).reshape(-1)
            offs[j] = at
            flat.append(oriented[key])
            at += oriented[key].size
        g = todo[pi]
        found = _walk(o[g], d[g], inv[g], ln[g], t_in[mi, pi], axis[mi, pi], lo[mi], models["scale"][sel].astype(f32)[mi], ext_all[sel][mi],
                      offs[mi], np.concatenate(flat))
        out[g[found]] = True
    return out


def entities_block(boxes, models, stamps, o, v, dist2):
    """blocked bool[n]: an entity blocks the pair whose segment runs from o[n, 3] along v[n, 3] to the light at squared distance
    dist2[n]."""
    o, v, dist2 = np.asarray(o, dtype=f32).reshape(-1, 3), np.asarray(v, dtype=f32).reshape(-1, 3), np.asarray(dist2, dtype=f32).reshape(-1)
    d, inv, ln = segments(v, dist2)
    out = np.zeros(o.shape[0], dtype=bool)
    if boxes is not None and len(boxes):
        out |= boxes_block(boxes, o, d, inv, ln)
    if models is not None and len(models):
        todo = np.nonzero(~out)[0]
        out[todo[models_block(models, stamps, o[todo], d[todo], inv[todo], ln[todo])]] = True
    return out


def weights(planes, u, lights, boxes, models, stamps, minefield, width, height, region=256, block=16, classes=None):
    """w float32[N, H, W]: the weight of every light at every pixel, +0 where the light is skipped or blocked, and seen bool[N, H, W].
    `classes`: a dict that receives how many pairs passed the pair test and ended `entity_only` (an entity blocks, the world's ray
    would not), `world_only`, `both` and `visible` — the world's ray is then traced for every pair, which the verdict does not need."""
    lights = np.asarray(lights).reshape(-1)
    surface, P, axis, even = pl.surface_points(planes, u, width, height)
    Pf, af, ef, sf = P.reshape(-1, 3), axis.reshape(-1), even.reshape(-1), surface.reshape(-1)
    ok = pl.valid(lights)
    w = np.zeros((lights.size, height * width), dtype=f32)
    seen = np.zeros((lights.size, height * width), dtype=bool)
    lr = tuple(int(x) for x in u.lr[:])
    if classes is not None:
        classes.update(entity_only=0, world_only=0, both=0, visible=0)
    for first in range(0, lights.size, block):
        L = lights[first:first + block]
        passes, v, dist2, r2, c = pl.pair_terms(Pf, af, ef, L["position"].astype(f32), L["radius"].astype(f32))
        passes &= sf[None, :] & ok[first:first + block, None]
        li, pi = np.nonzero(passes)
        blocked = entities_block(boxes, models, stamps, Pf[pi], v[li, pi], dist2[li, pi])
        if classes is not None:
            world = pl.trace_visible(minefield, region, lr, Pf[pi], v[li, pi], dist2[li, pi])
            classes["entity_only"] += int((blocked & world).sum())
            classes["world_only"] += int((~blocked & ~world).sum())
            classes["both"] += int((blocked & ~world).sum())
            classes["visible"] += int((~blocked & world).sum())
            vis = ~blocked & world
        else:
            vis = ~blocked
            vis[~blocked] = pl.trace_visible(minefield, region, lr, Pf[pi[~blocked]], v[li[~blocked], pi[~blocked]], dist2[li[~blocked], pi[~blocked]])
        li, pi = li[vis], pi[vis]
        with np.errstate(all="ignore"):
            d2, cc = dist2[li, pi], c[li, pi]
            ln = np.sqrt(d2).astype(f32)
            cosine = (cc / ln).astype(f32)
            x = (f32(1.0) - (d2 / r2[li]).astype(f32)).astype(f32)
            w[first + li, pi] = ((cosine * (x * x).astype(f32)).astype(f32) / (f32(1.0) + d2).astype(f32)).astype(f32)
        seen[first + li, pi] = True
    return w.reshape(-1, height, width), seen.reshape(-1, height, width)


def add_lights_occluded(planes, u, lights, boxes, models, stamps, minefield, width, height, region=256, classes=None):
    """The planes after rt_add_lights_occluded(u, lights, boxes, models) on `planes`, with `minefield` the resident region's bytes
    ([z][y][x])."""
    out = {name: np.array(p, copy=True) for name, p in planes.items()}
    lights = np.asarray(lights).reshape(-1)
    if lights.size == 0:
        return out
    w, seen = weights(planes, u, lights, boxes, models, stamps, minefield, width, height, region, classes=classes)
    color = lights["color"].astype(f32)
    add = np.zeros((height, width, 3), dtype=f32)
    with np.errstate(all="ignore"):
        for i in np.nonzero(seen.any(axis=(1, 2)))[0]:          # in index order; a light seen nowhere adds +0 everywhere
            add[seen[i]] = (add[seen[i]] + (color[i][None, :] * w[i][seen[i]][:, None]).astype(f32)).astype(f32)
        lit = seen.any(axis=0)
        s = (add / f32(16.0)).astype(f32)
        out["lighting_f32"][..., :3][lit] = (planes["lighting_f32"][..., :3] + s).astype(f32)[lit]
        q = (planes["lighting_rgba16"][..., :3].astype(f32) / f32(65535.0)).astype(f32)
        out["lighting_rgba16"][..., :3][lit] = unorm((q + s).astype(f32), 65535.0).astype(np.uint16)[lit]
    return out
