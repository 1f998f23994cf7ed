"""numpy restatement of rt_shadow_entities (include/rt_abi.h "Entity shadows").  Test infrastructure.

No cull: every box and every model is tested against every surface pixel (in blocks of occluders, for memory's sake only); every
pixel whose sun ray enters a model's bounding box walks that model's cells by the header's words; every pixel some occluder shades
gets the world's sun ray.  Every operation is a float32 array operation rounded on its own; the contract's fused operations go
through the exact fma emulation of tests/denoise_history_ref.py.

The surface point P' is tests/point_light_ref.surface_points (rt_add_lights' rule, word for word); the sun's direction and colour are
oracle/pyoracle.sun; record validity and the placed extents are tests/draw_boxes_ref.valid and tests/draw_stamps_ref's.  The slab
test is restated here (its origin differs per pixel and its direction does not, the other way round from rt_draw_boxes), and so are
the start-inside first cell and the boolean walk.  The world's ray is trace_ray (raytrace.comp:82-183) written from the shader's
lines, not from the kernels' DDA: the minefield is the linear [z][y][x] array the oracle reads, fetched with the sampler's wrap and
border; test_entity_shadow_contract.py holds it against the CPU oracle's trace_ray.

shadow_entities(planes, u, boxes, models, stamps, minefield, width, height) takes the frame's planes as Context.readback_all returns
them and returns new planes; planes it does not write are passed through as they are.  `stamps` maps a stamp id to (materials,
state[ez, ey, ex]) as for tests/draw_stamps_ref."""
import numpy as np

from oracle import pyoracle as po
from tests import draw_boxes_ref as boxes_ref
from tests import draw_stamps_ref as stamps_ref
from tests import stamp_edits as se
from tests.denoise_history_ref import fma
from tests.draw_boxes_ref import length3, unorm
from tests.point_light_ref import surface_points

f32 = np.float32
TRACE_LIMIT = 2048                       # RT_TRACE_LIMIT
WRITTEN = ("lighting_f32", "lighting_rgba16")
AIR, SOLID, LIMIT = 0, 1, 2              # how the world's ray ended (RT_HIT_AIR, RT_HIT_SOLID, RT_HIT_LIMIT)
MODEL_DTYPE = stamps_ref.MODEL_DTYPE


def sun_of(u):
    """(s float32[3], sunlight float32[3]): the frame's sun direction and colour."""
    return po.sun(u.sun_angle)


def _rmin(a, b):
    return np.where(b < a, b, a)         # rtm_min(a, b)


def _rmax(a, b):
    return np.where(a < b, b, a)         # rtm_max(a, b)


def slab(lo, hi, o, s):
    """rt_draw_boxes' slab test of the rays (o[n, 3], direction s[3]) against the boxes lo, hi [m, 3], operation by operation:
    (t_in[m, n], t_out[m, n], axis[m, n], bounded & every zero-direction axis passes [m, n])."""
    m, n = lo.shape[0], o.shape[0]
    bounded = np.zeros((m, n), dtype=bool)
    miss = np.zeros((m, n), dtype=bool)
    t_in = np.zeros((m, n), dtype=f32)
    t_out = np.zeros((m, n), dtype=f32)
    axis = np.zeros((m, n), dtype=np.int8)
    with np.errstate(all="ignore"):
        inv = (f32(1.0) / s).astype(f32)
        for k in range(3):
            if s[k] != 0:
                t0 = ((lo[:, k, None] - o[None, :, k]).astype(f32) * inv[k]).astype(f32)
                t1 = ((hi[:, k, None] - o[None, :, k]).astype(f32) * inv[k]).astype(f32)
                tn, tf = _rmin(t0, t1), _rmax(t0, t1)
                if not bounded.any():                       # (the same for every pair: the direction is one)
                    t_in, t_out, axis[:] = tn, tf, k
                    bounded[:] = True
                else:
                    new_in = tn > t_in
                    t_in = np.where(new_in, tn, t_in)
                    axis = np.where(new_in, np.int8(k), axis)
                    t_out = np.where(tf < t_out, tf, t_out)
            else:
                miss |= ~((lo[:, k, None] < o[None, :, k]) & (o[None, :, k] < hi[:, k, None]))
    return t_in, t_out, axis, bounded & ~miss


def crossed(lo, hi, o, s):
    """(shades[m, n], t_in, axis): the box rule — some axis gave a bound, every zero axis passes, t_out > 0 and t_in < t_out."""
    t_in, t_out, axis, ok = slab(lo, hi, o, s)
    with np.errstate(invalid="ignore"):
        return ok & (t_out > 0) & (t_in < t_out), t_in, axis


def boxes_shade(boxes, o, s, block=64):
    """shaded bool[n]: some valid box shades the point."""
    boxes = np.asarray(boxes).reshape(-1)
    out = np.zeros(o.shape[0], dtype=bool)
    ok = boxes_ref.valid(boxes) if boxes.size else np.zeros(0, dtype=bool)
    for first in range(0, boxes.size, block):
        sel = np.arange(first, min(first + block, boxes.size))[ok[first:first + block]]
        if sel.size:
            out |= crossed(boxes["lo"][sel].astype(f32), boxes["hi"][sel].astype(f32), o, s)[0].any(axis=0)
    return out


def _walk(o, s, t_in, axis, origin, scale, ext, off, state_flat):
    """The first cell and the boolean walk for n (model, pixel) pairs at once: o, origin [n, 3]; t_in, scale [n]; axis [n]; ext [n, 3] =
    E'; off [n] = where the pair's model starts in state_flat (its oriented state array, [z, y, x] flattened).  found[n]."""
    n = t_in.shape[0]
    c = np.zeros((n, 3), dtype=np.int64)
    with np.errstate(all="ignore"):
        inv = (f32(1.0) / s).astype(f32)
        outside = t_in > 0
        for k in range(3):
            entry = o[:, k] if s[k] == 0 else fma(np.full(n, s[k], dtype=f32), t_in, o[:, k])
            p = np.where(outside, entry, o[:, k]).astype(f32)
            q = np.floor(((p - origin[:, k]).astype(f32) / scale).astype(f32))
            q = np.where(q > 0, np.minimum(q, (ext[:, k] - 1).astype(f32)), f32(0.0))         # clamp(int(.), 0, E' - 1)
            c[:, k] = np.where(outside & (axis == k), 0 if s[k] > 0 else ext[:, k] - 1, q.astype(np.int64))
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
        cc = c[live]
        have = False
        tmin = np.zeros(live.size, dtype=f32)
        ax = np.zeros(live.size, dtype=np.int64)
        with np.errstate(all="ignore"):
            for k in range(3):                                                                # (2)
                if s[k] == 0:
                    continue
                i = (cc[:, k] + (1 if s[k] > 0 else 0)).astype(f32)
                w = fma(i, scale[live], origin[live, k])
                tk = ((w - o[live, k]).astype(f32) * inv[k]).astype(f32)
                take = (tk < tmin) if have else np.ones(live.size, dtype=bool)
                tmin = np.where(take, tk, tmin)
                ax = np.where(take, k, ax)
                have = True
        if not have:
            break
        rows = np.arange(live.size)
        step = np.array([1 if s[k] > 0 else -1 for k in range(3)], dtype=np.int64)
        cc[rows, ax] += step[ax]                                                              # (3)
        inside = (cc[rows, ax] >= 0) & (cc[rows, ax] < ext[live][rows, ax])
        c[live] = cc
        live = live[inside]
    return found


def models_shade(models, stamps, o, s, block=32):
    """shaded bool[n]: some model's walk from the point along s stops on a SOLID cell.  Every record must be valid (the library
    rejects the call otherwise)."""
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
        lo, hi = models["origin"][sel].astype(f32), hi_all[sel]
        enters, t_in, axis = crossed(lo, hi, o, s)
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
        found = _walk(o[pi], s, t_in[mi, pi], axis[mi, pi], lo[mi], models["scale"][sel].astype(f32)[mi], ext_all[sel][mi], offs[mi],
                      np.concatenate(flat))
        out[pi[found]] = True
    return out


# ---- inputs the tests share ---------------------------------------------------------------------------------------------------------------
def scatter_boxes(planes, u, width, height, n, seed, lift=(0.5, 6.0)):
    """n RtDrawBox records (raytrace_amd.render.DRAW_BOX_DTYPE) scattered 0.5 to 6 units above random surface pixels: half extents
    0.2 to 1.2, one box in sixteen sunk into its surface instead."""
    from raytrace_amd import render
    rng = np.random.default_rng(seed)
    surface, P, _, _ = surface_points(planes, u, width, height)
    pts = P[surface].astype(np.float64)
    assert len(pts) > 100
    c = pts[rng.integers(0, len(pts), n)] + rng.uniform(-0.5, 0.5, (n, 3))
    c[:, 2] += np.where(rng.random(n) < 1.0 / 16.0, -0.3, rng.uniform(lift[0], lift[1], n))
    half = rng.uniform(0.2, 1.2, (n, 3))
    b = np.zeros(n, dtype=render.DRAW_BOX_DTYPE)
    b["lo"], b["hi"] = (c - half).astype(f32), (c + half).astype(f32)
    b["material"], b["emission"] = 0x1FFFFF, 0xFF000000
    return b


def small_stamp(seed=1, extent=(3, 4, 5)):
    """(materials u32[ez, ey, ex], state u8[ez, ey, ex]) of a small sparse stamp: four voxels in ten solid, the rest air and absent."""
    rng = np.random.default_rng(seed)
    ex, ey, ez = extent
    r = rng.random((ez, ey, ex))
    state = np.where(r < 0.4, se.SOLID, np.where(r < 0.7, se.AIR, se.ABSENT)).astype(np.uint8)
    mats = np.where(state == se.SOLID, rng.integers(1, 1 << 21, (ez, ey, ex)), 0).astype(np.uint32)
    return mats, state


def scatter_models(planes, u, width, height, n, seed, stamp_id, extent, scales=(0.125, 1.0), lift=(0.5, 6.0)):
    """n RtDrawStamp records of stamp `stamp_id` (extent (ex, ey, ez)) scattered like the boxes, at the given scales in turn and with
    orientations spread over the 48."""
    rng = np.random.default_rng(seed)
    surface, P, _, _ = surface_points(planes, u, width, height)
    pts = P[surface].astype(np.float64)
    c = pts[rng.integers(0, len(pts), n)] + rng.uniform(-0.5, 0.5, (n, 3))
    c[:, 2] += rng.uniform(lift[0], lift[1], n)
    out = []
    for i in range(n):
        orient, scale = (7 * i + seed) % 48, scales[i % len(scales)]
        e = np.array(se.placed_extent(tuple(extent), orient), dtype=np.float64)
        out.append(stamps_ref.model(stamp_id, (c[i] - 0.5 * e * scale).astype(f32), scale, orient))
    return stamps_ref.batch(out)


def _mod(x, y):
    """rtm_mod: x - y * floor(x / y)."""
    return (x - (y * np.floor((x / y).astype(f32))).astype(f32)).astype(f32)


def _fetch(mine, R, pos):
    """The minefield sampler at `pos` [n, 3]: mod(pos + R/2, R) per axis, NEAREST, border value 0 (a NaN lands on the border)."""
    W = f32(R)
    c = _mod((pos + W / f32(2)).astype(f32), W)
    ok = ((c >= 0) & (c < W)).all(axis=1)
    i = np.where(ok[:, None], c, 0).astype(np.int64)
    return np.where(ok, mine[(i[:, 2] * R + i[:, 1]) * R + i[:, 0]], 0).astype(np.int64)


def trace_kind(minefield, region, lr, origin, direction):
    """kind int[n] (AIR, SOLID, LIMIT): trace_ray from origin[n, 3] along direction[3] (normalised here, as the shader does)."""
    mine = np.ascontiguousarray(minefield, dtype=np.uint8).reshape(-1)
    R = int(region)
    assert mine.size == R ** 3
    origin = np.asarray(origin, dtype=f32).reshape(-1, 3)
    n = origin.shape[0]
    kind = np.full(n, LIMIT, dtype=np.int64)
    if n == 0:
        return kind
    half = f32(R) / f32(2)
    lrf = np.array([lr[0], lr[1], lr[2]], dtype=f32)
    v = np.asarray(direction, dtype=f32).reshape(3)
    with np.errstate(all="ignore"):
        d = (v * (f32(1.0) / length3(v[0], v[1], v[2])).astype(f32)).astype(f32)   # :83
        ln = (f32(1.0) / np.abs(d)).astype(f32)                                     # :88
        muls = np.where(d > 0, f32(-1.0), f32(1.0)).astype(f32)
        pos = origin.copy()
        step = _fetch(mine, R, pos)                                                 # :106
        idx = np.arange(n)                                                          # the rays still alive
        for _ in range(TRACE_LIMIT):                                                # :109-113
            if idx.size == 0:
                break
            ss = ((1 << (step & 31)) // 2).astype(f32)[:, None]                     # :107, :161
            q = ((pos + half).astype(f32) * muls).astype(f32)
            l = ((f32(0.0001) + _mod(q, ss)).astype(f32) * ln).astype(f32)          # :119 (step 0: mod(x, 0) is NaN)
            lx, ly, lz = l[:, 0], l[:, 1], l[:, 2]
            t = np.where(lx < ly, np.where(lx < lz, lx, lz), np.where(ly < lz, ly, lz))   # :120-136
            pos = np.stack([fma(np.full(idx.size, d[k], dtype=f32), t, pos[:, k]) for k in range(3)], axis=-1)
            step = _fetch(mine, R, pos)                                             # :137
            sky = (np.abs((pos - lrf).astype(f32)) >= half).any(axis=1)             # :138-145
            hit = ~sky & (step == 0)                                                # :146
            kind[idx[sky]] = AIR
            kind[idx[hit]] = SOLID
            go = ~(sky | hit)
            idx, pos, step = idx[go], pos[go], step[go]
    return kind


def masks(planes, u, boxes, models, stamps, minefield, width, height, region=256):
    """The four classes of a frame's pixels, bool[H, W] each: `changed` (an entity shades the pixel and the world's sun ray leaves the
    window), `world` (an entity shades it but the world does already), `open` (a surface pixel no occluder shades) and `sky`."""
    surface, P, _, _ = surface_points(planes, u, width, height)
    s, _ = sun_of(u)
    o = P[surface].astype(f32)
    shaded = boxes_shade(boxes, o, s) if boxes is not None and len(boxes) else np.zeros(o.shape[0], dtype=bool)
    if models is not None and len(models):
        shaded |= models_shade(models, stamps, o, s)
    lit = np.zeros(o.shape[0], dtype=bool)
    lit[shaded] = trace_kind(minefield, region, tuple(int(x) for x in u.lr[:]), o[shaded], s) == AIR
    out = {}
    for name, m in (("changed", shaded & lit), ("world", shaded & ~lit), ("open", ~shaded)):
        out[name] = np.zeros((height, width), dtype=bool)
        out[name][surface] = m
    out["sky"] = ~surface
    return out


def shadow_entities(planes, u, boxes, models, stamps, minefield, width, height, region=256, strength=1.0, sunlight=None, classes=None):
    """The planes after rt_shadow_entities(u, boxes, models, strength) on `planes`, with `minefield` the resident region's bytes
    ([z][y][x]).  `sunlight` replaces the frame's sun colour (the contract's night, which no sun angle is known to give); `classes`
    is what masks() returned for these arguments, if the caller has it already."""
    out = {name: np.array(p, copy=True) for name, p in planes.items()}
    nb = 0 if boxes is None else len(boxes)
    nm = 0 if models is None else len(models)
    color = sun_of(u)[1] if sunlight is None else np.asarray(sunlight, dtype=f32)
    if nb + nm == 0 or (color == 0).all():
        return out
    changed = (classes or masks(planes, u, boxes, models, stamps, minefield, width, height, region))["changed"]
    with np.errstate(all="ignore"):
        sub = ((color * f32(strength)).astype(f32) / f32(16.0)).astype(f32)
        L = planes["lighting_f32"][..., :3].astype(f32)
        out["lighting_f32"][..., :3][changed] = _rmax((L - sub).astype(f32), f32(0.0))[changed]
        q = (planes["lighting_rgba16"][..., :3].astype(f32) / f32(65535.0)).astype(f32)
        out["lighting_rgba16"][..., :3][changed] = unorm(_rmax((q - sub).astype(f32), f32(0.0)), 65535.0).astype(np.uint16)[changed]
    return out
