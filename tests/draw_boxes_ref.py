"""numpy restatement of rt_draw_boxes (include/rt_abi.h "Entity boxes").  Test infrastructure.

No cull: every box is tested against every pixel (in blocks of boxes, for memory's sake only).  Every operation is a float32 array
operation rounded on its own; the contract's three fused operations (the two of rtm_length3, P = rtm_fma(d, t_in, o)) go through the
exact fma emulation of tests/denoise_history_ref.py.  The direction is tests/shader_formulas.primary_direction's expression restated in
float32 (that one is float64, for formulas that need no bits); test_draw_boxes_contract.py holds the two against each other.

draw_boxes(planes, u, boxes, lights, width, height) takes the frame's planes as Context.readback_all / pyoracle.render return them and
returns new planes; planes it does not write are passed through as they are."""
import numpy as np

from tests.denoise_history_ref import fma

f32 = np.float32
MAX_COORD = f32(4194304.0)
WRITTEN = ("depth_f32", "depth_r16", "normal_r8", "albedo_rgba8", "emission_rgba8", "lighting_f32", "lighting_rgba16")


def _vec(c):
    return np.array([c[0], c[1], c[2]], dtype=f32)


def length3(x, y, z):
    """rtm_length3."""
    return np.sqrt(fma(z, z, fma(y, y, (x * x).astype(f32)))).astype(f32)


def directions(u, width, height):
    """d[H, W, 3] float32: normalize(forward + right * sx + up * sy), each product and sum rounded, rtm_normalize3."""
    fwd, up, right = _vec(u.forward), _vec(u.up), _vec(u.right)
    sx = (np.arange(width, dtype=f32) / f32(width)) * f32(2.0) - f32(1.0)
    sy = (np.arange(height, dtype=f32) / f32(height)) * f32(2.0) - f32(1.0)
    v = [((fwd[k] + right[k] * sx)[None, :] + (up[k] * sy)[:, None]).astype(f32) for k in range(3)]
    r = (f32(1.0) / length3(v[0], v[1], v[2])).astype(f32)
    return np.stack([(v[k] * r).astype(f32) for k in range(3)], axis=-1)


def valid(boxes):
    """The contract's valid box, per record."""
    lo, hi = boxes["lo"].astype(f32), boxes["hi"].astype(f32)
    with np.errstate(invalid="ignore"):
        return ((np.abs(lo) <= MAX_COORD) & (np.abs(hi) <= MAX_COORD) & (lo < hi)).all(axis=1)


def unorm(x, maxv):
    """rtm_unorm."""
    x = np.asarray(x, dtype=f32)
    with np.errstate(invalid="ignore"):
        q = np.floor((np.minimum(x, f32(1.0)) * f32(maxv) + f32(0.5)).astype(f32))
        return np.where(x > 0, q, 0).astype(np.uint32)


def f2u16(x):
    """rtm_f2u16."""
    x = np.asarray(x, dtype=f32)
    with np.errstate(invalid="ignore"):
        inner = np.where((x > 0) & (x < f32(65535.0)), x, 0).astype(np.int64)   # truncates
        return np.where(x >= f32(65535.0), 65535, inner).astype(np.uint16)


def albedo_rgba8(material):
    """pack_rgba8(albedo_of(material), 1) as [.., 4] uint8."""
    m = np.asarray(material, dtype=np.uint32)
    ch = [unorm(((m >> s) & 0x7F).astype(f32) / f32(127.0), 255.0) for s in (14, 7, 0)]
    return np.stack(ch + [np.full(m.shape, 255, dtype=np.uint32)], axis=-1).astype(np.uint8)


def _slab_general(lo, hi, o, d, inv, shape):
    """(t_in, t_out, axis, bounded & every zero-component axis passes) of a block of boxes, the contract's words operation by operation."""
    bounded = np.zeros(shape, dtype=bool)
    miss = np.zeros(shape, dtype=bool)
    t_in = np.zeros(shape, dtype=f32)
    t_out = np.zeros(shape, dtype=f32)
    axis = np.zeros(shape, dtype=np.int8)
    for k in range(3):
        nz = np.broadcast_to((d[..., k] != 0)[None], shape)
        t0 = (lo[:, k] - o[k])[:, None, None] * inv[..., k][None]
        t1 = (hi[:, k] - o[k])[:, None, None] * inv[..., k][None]
        tn = np.where(t1 < t0, t1, t0)                       # rtm_min(t0, t1)
        tf = np.where(t0 < t1, t1, t0)                       # rtm_max(t0, t1)
        start = nz & ~bounded
        later = nz & bounded
        new_in = start | (later & (tn > t_in))
        new_out = start | (later & (tf < t_out))
        t_in = np.where(new_in, tn, t_in)
        axis = np.where(new_in, np.int8(k), axis)
        t_out = np.where(new_out, tf, t_out)
        bounded = bounded | nz
        passes = ((lo[:, k] < o[k]) & (o[k] < hi[:, k]))[:, None, None]
        miss = miss | (~nz & ~passes)
    return t_in, t_out, axis, bounded & ~miss


def _slab_plain(lo, hi, o, inv):
    """The same where every direction component of every pixel is non-zero and every product is a number: rtm_min / rtm_max are then
    the minimum and maximum, 'replace iff greater' is a running maximum, and no axis needs the zero-component rule.  (A zero of either
    sign compares alike, so which zero a minimum returns decides nothing.)"""
    t_in = t_out = axis = None
    for k in range(3):
        t0 = (lo[:, k] - o[k])[:, None, None] * inv[..., k][None]
        t1 = (hi[:, k] - o[k])[:, None, None] * inv[..., k][None]
        tn, tf = np.minimum(t0, t1), np.maximum(t0, t1)
        if k == 0:
            t_in, t_out, axis = tn, tf, np.zeros(tn.shape, dtype=np.int8)
            continue
        axis[tn > t_in] = k
        np.maximum(t_in, tn, out=t_in)
        np.minimum(t_out, tf, out=t_out)
    return t_in, t_out, axis, True


def winners(u, boxes, width, height, block=8):
    """(t_in[H, W] float32, index[H, W] int64 (-1: none), axis[H, W] int64, d[H, W, 3]) of the box every pixel's ray hits first."""
    d = directions(u, width, height)
    o = _vec(u.origin)
    ok = valid(boxes)
    best_t = np.full((height, width), np.inf, dtype=f32)
    best_i = np.full((height, width), -1, dtype=np.int64)
    best_a = np.zeros((height, width), dtype=np.int64)
    with np.errstate(all="ignore"):
        inv = (f32(1.0) / d).astype(f32)
        plain = bool((d != 0).all() and np.isfinite(inv).all() and np.isfinite(o).all())
        for first in range(0, boxes.size, block):
            lo = boxes["lo"][first:first + block].astype(f32)
            hi = boxes["hi"][first:first + block].astype(f32)
            n = lo.shape[0]
            fine = ok[first:first + n]
            if plain and fine.all():
                t_in, t_out, axis, alive = _slab_plain(lo, hi, o, inv)
            else:
                t_in, t_out, axis, alive = _slab_general(lo, hi, o, d, inv, (n, height, width))
            hit = (t_in > 0) & (t_in < t_out) & alive & fine[:, None, None]
            t_hit = np.where(hit, t_in, f32(np.inf))
            j = np.argmin(t_hit, axis=0)                             # the first of equal minima: the lowest index
            t_j = np.take_along_axis(t_hit, j[None], axis=0)[0]
            a_j = np.take_along_axis(axis, j[None], axis=0)[0]
            better = t_j < best_t                                    # strict: an earlier block's box wins a tie
            best_t = np.where(better, t_j, best_t)
            best_i = np.where(better, first + j, best_i)
            best_a = np.where(better, a_j, best_a)
    return best_t, best_i, best_a, d


def draw_boxes(planes, u, boxes, lights, width, height):
    """The planes after rt_draw_boxes(u, boxes, lights) on `planes`."""
    out = {name: np.array(p, copy=True) for name, p in planes.items()}
    boxes = np.asarray(boxes).reshape(-1)
    if boxes.size == 0:
        return out
    light = np.asarray(lights).reshape(-1)["light"].astype(f32).reshape(-1, 3)
    assert light.shape[0] == 6 * boxes.size
    t_in, idx, axis, d = winners(u, boxes, width, height)
    o = _vec(u.origin)
    with np.errstate(all="ignore"):
        t = np.where(idx >= 0, t_in, f32(0.0)).astype(f32)
        P = [fma(d[..., k], t, np.full_like(t, o[k])) for k in range(3)]
        depth_f = (length3((o[0] - P[0]).astype(f32), (o[1] - P[1]).astype(f32), (o[2] - P[2]).astype(f32)) * f32(32.0)).astype(f32)
        drawn = (idx >= 0) & (depth_f < planes["depth_f32"])
    d_a = np.take_along_axis(d, axis[..., None], axis=-1)[..., 0]
    normal = 2 * axis + (d_a > 0)
    b = np.where(drawn, idx, 0)
    out["depth_f32"][drawn] = depth_f[drawn]
    out["depth_r16"][drawn] = f2u16(depth_f)[drawn]
    out["normal_r8"][drawn] = normal[drawn].astype(np.uint8)
    out["albedo_rgba8"][drawn] = albedo_rgba8(boxes["material"][b])[drawn]
    em = boxes["emission"][b].astype(np.uint32)
    out["emission_rgba8"][drawn] = np.stack([(em >> s) & 0xFF for s in (0, 8, 16, 24)], axis=-1).astype(np.uint8)[drawn]
    # store_lighting(sum = light, spp = 1): (light / 1.0f) / 16 and 1 / 16, then UNORM16
    with np.errstate(all="ignore"):
        L = light[6 * b + normal]
        lv = np.concatenate([((L / f32(1.0)).astype(f32) / f32(16.0)).astype(f32), np.full(L.shape[:-1] + (1,), f32(1.0) / f32(16.0), dtype=f32)], axis=-1)
    out["lighting_f32"][drawn] = lv[drawn]
    out["lighting_rgba16"][drawn] = unorm(lv, 65535.0).astype(np.uint16)[drawn]
    return out
