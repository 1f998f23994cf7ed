"""numpy restatement of rt_add_lights (include/rt_abi.h "Point lights").  Test infrastructure.

No cull: every light is tested against every pixel (in blocks of lights, for memory's sake only), and every (pixel, light) pair that
passes the exact test gets its shadow ray.  The rays of a block are stepped together: one numpy step per loop iteration for all rays
still alive.  Every operation is a float32 array operation rounded on its own; the contract's fused operations (rtm_dot3, rtm_fma in P
and in the ray's position, the two of rtm_normalize3's length) go through the exact fma emulation of tests/denoise_history_ref.py.

The shadow ray is trace_ray (raytrace.comp:82-183) written from the shader's lines, not from the kernels' DDA: the minefield is the
linear [z][y][x] array the oracle reads, fetched with the sampler's wrap and border.

add_lights(planes, u, lights, minefield, width, height, region) takes the frame's planes as Context.readback_all returns them and
returns new planes; planes it does not write are passed through as they are."""
import numpy as np

from tests.denoise_history_ref import fma
from tests.draw_boxes_ref import directions, length3, unorm

f32 = np.float32
MAX_COORD, MAX_RADIUS, MAX_COLOR = f32(4194304.0), f32(1024.0), f32(1048576.0)
OFFSET = f32(0.03125)
TRACE_LIMIT = 2048                       # RT_TRACE_LIMIT
WRITTEN = ("lighting_f32", "lighting_rgba16")
END_REACHED, END_AIR, END_SOLID, END_LIMIT = 0, 1, 2, 3      # how a shadow ray ended (trace_visible's `ends`)


def dot3(a, b):
    """rtm_dot3 of [..., 3] arrays."""
    return fma(a[..., 2], b[..., 2], fma(a[..., 1], b[..., 1], (a[..., 0] * b[..., 0]).astype(f32)))


def valid(lights):
    """The contract's valid light, per record."""
    pos, rad, col = lights["position"].astype(f32), lights["radius"].astype(f32), lights["color"].astype(f32)
    with np.errstate(invalid="ignore"):
        return ((np.abs(pos) <= MAX_COORD).all(axis=1) & (rad > 0) & (rad <= MAX_RADIUS) & ((col >= 0) & (col <= MAX_COLOR)).all(axis=1)
                & (lights["reserved"] == 0))


def surface_points(planes, u, width, height):
    """(surface bool[H, W], P' float32[H, W, 3], axis int64[H, W], even bool[H, W]) of the frame's pixels."""
    normal = planes["normal_r8"].astype(np.int64)
    depth = planes["depth_f32"].astype(f32)
    with np.errstate(all="ignore"):
        surface = (normal < 6) & (depth < f32(65535.0))
        d = directions(u, width, height)
        t = (depth / f32(32.0)).astype(f32)
        o = np.array(u.origin[:], dtype=f32)
        P = np.stack([fma(d[..., k], t, np.full_like(t, o[k])) for k in range(3)], axis=-1)
        axis = np.where(surface, normal >> 1, 0)
        even = (normal & 1) == 0
        off = np.where(even, OFFSET, -OFFSET).astype(f32)
        moved = (np.take_along_axis(P, axis[..., None], axis=-1)[..., 0] + off).astype(f32)
        np.put_along_axis(P, axis[..., None], moved[..., None], axis=-1)
    return surface, P, axis, even


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


def trace_visible(minefield, region, lr, origin, v, dist2, ends=False):
    """visible bool[n]: the contract's shadow ray from origin[n, 3] in direction v[n, 3] (normalised here), ended as visible once
    rtm_dot3(pos - origin, pos - origin) >= dist2[n].  With `ends`: (visible, end int[n]) — how each ray ended, END_REACHED (as far from
    its origin as the light), END_AIR (left the window), END_SOLID or END_LIMIT (RT_TRACE_LIMIT steps: blocked)."""
    mine = np.ascontiguousarray(minefield, dtype=np.uint8).reshape(-1)
    R = int(region)
    assert mine.size == R ** 3
    origin, v, dist2 = np.asarray(origin, dtype=f32).reshape(-1, 3), np.asarray(v, dtype=f32).reshape(-1, 3), np.asarray(dist2, dtype=f32).reshape(-1)
    n = origin.shape[0]
    visible = np.zeros(n, dtype=bool)
    end = np.full(n, END_LIMIT, dtype=np.int64)
    if n == 0:
        return (visible, end) if ends else visible
    half = f32(R) / f32(2)
    lrf = np.array([lr[0], lr[1], lr[2]], dtype=f32)
    with np.errstate(all="ignore"):
        rlen = (f32(1.0) / length3(v[:, 0], v[:, 1], v[:, 2])).astype(f32)
        d = (v * rlen[:, None]).astype(f32)                                     # :83
        ln = (f32(1.0) / np.abs(d)).astype(f32)                                 # :88
        muls = np.where(d > 0, f32(-1.0), f32(1.0)).astype(f32)
        pos = origin.copy()
        step = _fetch(mine, R, pos)                                             # :106
        idx = np.arange(n)                                                      # the rays still alive
        for _ in range(TRACE_LIMIT):                                            # :109-113
            if idx.size == 0:
                break
            ss = ((1 << (step & 31)) // 2).astype(f32)[:, None]                 # :107, :161
            q = ((pos + half).astype(f32) * muls[idx]).astype(f32)
            l = ((f32(0.0001) + _mod(q, ss)).astype(f32) * ln[idx]).astype(f32)  # :119 (step 0: mod(x, 0) is NaN)
            lx, ly, lz = l[:, 0], l[:, 1], l[:, 2]
            t = np.where(lx < ly, np.where(lx < lz, lx, lz), np.where(ly < lz, ly, lz))   # :120-136
            pos = np.stack([fma(d[idx, k], t, pos[:, k]) for k in range(3)], axis=-1)
            step = _fetch(mine, R, pos)                                         # :137
            sky = (np.abs((pos - lrf).astype(f32)) >= half).any(axis=1)         # :138-145
            e = (pos - origin[idx]).astype(f32)
            reach = ~sky & (dot3(e, e) >= dist2[idx])                           # the added exit
            hit = ~sky & ~reach & (step == 0)                                   # :146
            visible[idx[sky | reach]] = True
            end[idx[sky]], end[idx[reach]], end[idx[hit]] = END_AIR, END_REACHED, END_SOLID
            go = ~(sky | reach | hit)
            idx, pos, step = idx[go], pos[go], step[go]
    return (visible, end) if ends else visible                                  # (the loop limit: blocked)


def pair_terms(P, axis, even, light_pos, light_radius):
    """The exact test of a block of lights [m] against points P[n, 3]: (passes bool[m, n], v[m, n, 3], dist2[m, n], r2[m], c[m, n])."""
    with np.errstate(all="ignore"):
        v = (light_pos[:, None, :] - P[None, :, :]).astype(f32)
        dist2 = dot3(v, v)
        r2 = (light_radius * light_radius).astype(f32)
        va = np.take_along_axis(v, np.broadcast_to(axis[None, :, None], v.shape[:2] + (1,)), axis=-1)[..., 0]
        c = np.where(even[None, :], va, -va).astype(f32)
        passes = (dist2 > 0) & (dist2 < r2[:, None]) & (c > 0)
    return passes, v, dist2, r2, c


def weights(planes, u, lights, minefield, width, height, region=256, block=16):
    """w float32[N, H, W]: the weight of every light at every pixel, +0 where the light is skipped or blocked, and seen bool[N, H, W]."""
    lights = np.asarray(lights).reshape(-1)
    surface, P, axis, even = surface_points(planes, u, width, height)
    Pf, af, ef, sf = P.reshape(-1, 3), axis.reshape(-1), even.reshape(-1), surface.reshape(-1)
    ok = valid(lights)
    w = np.zeros((lights.size, height * width), dtype=f32)
    seen = np.zeros((lights.size, height * width), dtype=bool)
    lr = tuple(int(x) for x in u.lr[:])
    for first in range(0, lights.size, block):
        L = lights[first:first + block]
        passes, v, dist2, r2, c = pair_terms(Pf, af, ef, L["position"].astype(f32), L["radius"].astype(f32))
        passes &= sf[None, :] & ok[first:first + block, None]
        li, pi = np.nonzero(passes)
        vis = trace_visible(minefield, region, lr, Pf[pi], v[li, pi], dist2[li, pi])
        li, pi = li[vis], pi[vis]
        with np.errstate(all="ignore"):
            d2, cc = dist2[li, pi], c[li, pi]
            ln = np.sqrt(d2).astype(f32)
            cosine = (cc / ln).astype(f32)
            x = (f32(1.0) - (d2 / r2[li]).astype(f32)).astype(f32)
            w[first + li, pi] = ((cosine * (x * x).astype(f32)).astype(f32) / (f32(1.0) + d2).astype(f32)).astype(f32)
        seen[first + li, pi] = True
    return w.reshape(-1, height, width), seen.reshape(-1, height, width)


def add_lights(planes, u, lights, minefield, width, height, region=256):
    """The planes after rt_add_lights(u, lights) on `planes`, with `minefield` the resident region's bytes ([z][y][x])."""
    out = {name: np.array(p, copy=True) for name, p in planes.items()}
    lights = np.asarray(lights).reshape(-1)
    if lights.size == 0:
        return out
    w, seen = weights(planes, u, lights, minefield, width, height, region)
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
