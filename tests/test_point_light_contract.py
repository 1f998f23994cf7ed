"""The rules of rt_add_lights on the CPU: tests/point_light_ref.py (the restatement the GPU tests compare with bit for bit) on hand-made
planes over tiny hand-made worlds — an open floor's closed-form weight, a one-voxel wall's shadow, the lights that change nothing, the
voxel beyond the light, the independence of the sum from skipped lights and of the two planes from each other — and its shadow ray held
against the CPU oracle's trace_ray on pairs taken from a rendered frame of the terrain fixture."""
import numpy as np
import pytest

from oracle import pyoracle as po
from raytrace_amd import abi, render
from tests import point_light_ref as ref
from tests import synthetic_planes

f32 = np.float32
W, H = 48, 32
R = 256
CAM_Z = 10.5


def same(a, b):
    return a.keys() == b.keys() and all(a[k].tobytes() == b[k].tobytes() for k in a)


def down_camera():
    """Looks straight down from (0.25, 0.25, CAM_Z) with right = +x and up = +y, scaled 0.5."""
    u = abi.RtUniforms()
    for k in range(3):
        u.origin[k] = (0.25, 0.25, CAM_Z)[k]
        u.forward[k], u.right[k], u.up[k] = (0.0, 0.0, -1.0)[k], (0.5, 0.0, 0.0)[k], (0.0, 0.5, 0.0)[k]
    return u


def floor_world(extra_solid=()):
    """Air (minefield value 1: one-voxel steps) over a floor one voxel thick under z = 0; `extra_solid` world voxels are solid too."""
    mine = np.ones((R, R, R), dtype=np.uint8)
    mine[R // 2 - 1] = 0
    for (x, y, z) in extra_solid:
        mine[z + R // 2, y + R // 2, x + R // 2] = 0
    return mine


def floor_planes(u, seed=1):
    """The planes of the floor seen by `u`: every pixel's depth puts its point on z = 0 with the +z face code; the lighting planes
    hold unrelated values in their two representations."""
    rng = np.random.default_rng(seed)
    d = ref.directions(u, W, H)
    t = (f32(CAM_Z) / -d[..., 2]).astype(f32)
    planes = dict(depth_f32=(t * f32(32.0)).astype(f32), normal_r8=np.full((H, W), 4, dtype=np.uint8),
                  lighting_f32=(rng.random((H, W, 4), dtype=f32) * f32(0.5)).astype(f32),
                  lighting_rgba16=rng.integers(0, 30000, size=(H, W, 4)).astype(np.uint16))
    planes["depth_r16"] = planes["depth_f32"].astype(np.uint16)
    return planes


def light(pos, radius=8.0, color=(16.0, 8.0, 4.0)):
    return render.make_point_lights([pos], radius, color)


def points(planes, u):
    return ref.surface_points(planes, u, W, H)[1].astype(np.float64)


def test_rebuilt_points_lie_a_32nd_over_the_floor():
    u = down_camera()
    surface, P, axis, even = ref.surface_points(floor_planes(u), u, W, H)
    assert surface.all() and (axis == 2).all() and even.all()
    assert np.abs(P[..., 2] - 0.03125).max() < 1e-5
    assert P[..., 0].min() < -4 and P[..., 0].max() > 4             # the view spans several voxels


def test_open_floor_gets_the_closed_form_weight():
    u = down_camera()
    planes, mine = floor_planes(u), floor_world()
    L = light((0.5, 0.5, 3.0), radius=6.0)
    w, seen = ref.weights(planes, u, L, mine, W, H)
    v = np.array([0.5, 0.5, 3.0]) - points(planes, u)
    d2 = (v * v).sum(axis=-1)
    inside = d2 < 36.0
    assert np.array_equal(seen[0], inside) and 100 < inside.sum() < W * H
    want = (v[..., 2] / np.sqrt(d2)) * (1 - d2 / 36.0) ** 2 / (1 + d2)
    assert np.allclose(w[0][inside], want[inside], rtol=2e-5, atol=1e-9) and not w[0][~inside].any()
    out = ref.add_lights(planes, u, L, mine, W, H)
    for k, c in enumerate((16.0, 8.0, 4.0)):
        assert np.allclose(out["lighting_f32"][..., k] - planes["lighting_f32"][..., k], np.where(inside, c * want / 16.0, 0), rtol=1e-4, atol=1e-6)
    assert np.array_equal(out["lighting_f32"][..., 3], planes["lighting_f32"][..., 3])
    assert np.array_equal(out["lighting_rgba16"][..., 3], planes["lighting_rgba16"][..., 3])
    assert np.array_equal(out["lighting_f32"][~inside], planes["lighting_f32"][~inside])


def _segment_meets_box(p, q, lo, hi, grow):
    """Does the segment p[n, 3] -> q[3] meet the box [lo - grow, hi + grow]?  float64 slab test."""
    lo, hi = np.asarray(lo, dtype=np.float64) - grow, np.asarray(hi, dtype=np.float64) + grow
    d = q[None] - p
    with np.errstate(all="ignore"):
        t0, t1 = (lo - p) / d, (hi - p) / d
    tn, tf = np.minimum(t0, t1).max(axis=-1), np.maximum(t0, t1).min(axis=-1)
    return (tn <= tf) & (tf >= 0) & (tn <= 1)


def test_a_one_voxel_wall_blocks_exactly_the_pixels_behind_it():
    u = down_camera()
    planes = floor_planes(u)
    pos = np.array([0.5, 0.5, 4.0])
    L = light(pos, radius=12.0)
    open_seen = ref.weights(planes, u, L, floor_world(), W, H)[1][0]
    seen = ref.weights(planes, u, L, floor_world([(2, 0, 1)]), W, H)[1][0]
    P = points(planes, u).reshape(-1, 3)
    surely = _segment_meets_box(P, pos, (2, 0, 1), (3, 1, 2), -1e-3).reshape(H, W)
    maybe = _segment_meets_box(P, pos, (2, 0, 1), (3, 1, 2), 1e-3).reshape(H, W)
    assert open_seen.all() and 5 < surely.sum() < W * H // 4
    assert not seen[surely].any() and seen[~maybe].all()
    assert (maybe & ~surely).sum() <= 4                              # the undecided rim is a handful of pixels


def test_lights_that_add_nothing_leave_every_bit():
    u = down_camera()
    planes, mine = floor_planes(u), floor_world([(0, 0, 2), (1, 0, 2)])
    for what, L in (("inside a solid voxel", light((0.5, 0.5, 2.5))), ("behind the surface", light((0.5, 0.5, -3.0))),
                    ("just under the points' plane", light((0.5, 0.5, 0.03))), ("out of reach", light((0.5, 0.5, 5.0), radius=4.9)),
                    ("zero colour", light((5.5, 0.5, 2.0), color=(0.0, 0.0, 0.0))), ("none", np.zeros(0, dtype=render.POINT_LIGHT_DTYPE))):
        assert same(ref.add_lights(planes, u, L, mine, W, H), planes), what
    # the zero-colour light is seen: only its colour keeps the planes as they are
    assert ref.weights(planes, u, light((5.5, 0.5, 2.0)), mine, W, H)[1].any()
    # invalid records are skipped
    bad = np.concatenate([light((5.5, 0.5, 2.0))] * 5)
    bad["radius"][0], bad["color"][1][1], bad["reserved"][2], bad["position"][3][0], bad["radius"][4] = np.nan, -1.0, 1, 4194305.0, 1025.0
    assert not ref.valid(bad).any() and same(ref.add_lights(planes, u, bad, mine, W, H), planes)


def test_unorm16_round_trips_every_texel_under_a_zero_sum():
    q = np.arange(65536, dtype=np.uint16)
    assert np.array_equal(ref.unorm(((q.astype(f32) / f32(65535.0)).astype(f32) + f32(0.0)).astype(f32), 65535.0), q)


def test_a_solid_voxel_just_beyond_the_light_does_not_shadow_it():
    u = down_camera()
    planes = floor_planes(u)
    L = light((0.5, 0.5, 2.9), radius=7.0)
    a = ref.add_lights(planes, u, L, floor_world(), W, H)
    b = ref.add_lights(planes, u, L, floor_world([(0, 0, 3), (1, 0, 3), (0, 1, 3), (-1, 0, 3), (0, -1, 3)]), W, H)
    assert same(a, b) and not same(a, planes)


def test_the_sum_does_not_depend_on_skipped_lights():
    u = down_camera()
    planes, mine = floor_planes(u), floor_world([(2, 0, 1), (0, 0, 5)])
    A, C = light((0.5, 0.5, 3.0), color=(9.0, 3.0, 1.0)), light((-2.5, 1.5, 2.0), radius=5.0, color=(0.3, 7.0, 11.0))
    skipped = [light((0.5, 0.5, 5.5)), light((0.5, 0.5, -4.0)), light((3.5, 3.5, 9.0), radius=2.0), light((0, 0, 1), color=(0.0, 0.0, 0.0))]
    invalid = light((0.5, 0.5, 3.0))
    invalid["reserved"] = 7
    both = ref.add_lights(planes, u, np.concatenate([A, C]), mine, W, H)
    mixed = ref.add_lights(planes, u, np.concatenate([skipped[0], A, skipped[1], invalid, skipped[2], C, skipped[3]]), mine, W, H)
    assert same(both, mixed) and not same(both, planes)
    # ... but it does depend on the order of the lights that are seen: the sum is taken in index order
    swapped = ref.add_lights(planes, u, np.concatenate([C, A]), mine, W, H)
    assert np.allclose(swapped["lighting_f32"], both["lighting_f32"], rtol=1e-5)


def test_the_two_planes_are_updated_independently_and_unorm16_saturates():
    u = down_camera()
    syn = synthetic_planes.post_planes(W, H, seed=4)
    planes = floor_planes(u)
    planes["lighting_rgba16"] = syn["lighting"]                     # the whole u16 range, unrelated to the float plane
    planes["normal_r8"] = syn["normal"]                             # every byte: most pixels are no surface pixels
    mine = floor_world()
    L = light((0.5, 0.5, 3.0), radius=9.0, color=(4000.0, 40.0, 0.4))
    out = ref.add_lights(planes, u, L, mine, W, H)
    w, seen = ref.weights(planes, u, L, mine, W, H)
    lit = seen[0]
    none = planes["normal_r8"] >= 6
    assert lit[planes["normal_r8"] == 4].any() and not lit[none].any() and none.sum() > W * H // 4
    for name in out:
        assert np.array_equal(out[name][~lit], planes[name][~lit]), name
        if name not in ref.WRITTEN:
            assert out[name].tobytes() == planes[name].tobytes(), name
    s = ((np.array([4000.0, 40.0, 0.4], dtype=f32)[None] * w[0][lit][:, None]).astype(f32) / f32(16.0)).astype(f32)
    assert np.array_equal(out["lighting_f32"][lit][:, :3], (planes["lighting_f32"][lit][:, :3] + s).astype(f32))
    q = planes["lighting_rgba16"][lit][:, :3]
    assert np.array_equal(out["lighting_rgba16"][lit][:, :3], ref.unorm(((q.astype(f32) / f32(65535.0)).astype(f32) + s).astype(f32), 65535.0))
    assert (out["lighting_rgba16"][lit][:, 0] == 65535).any() and (out["lighting_rgba16"][lit][:, 2] < 65535).any()
    assert (out["lighting_f32"][lit][:, 0] > 1.0).any()             # the float plane does not saturate
    assert np.array_equal(out["lighting_rgba16"][..., 3], planes["lighting_rgba16"][..., 3])


def test_a_nan_depth_and_sky_are_no_surface_pixels():
    u = down_camera()
    planes = floor_planes(u)
    planes["depth_f32"][3, 5], planes["depth_f32"][4, 6], planes["normal_r8"][5, 7] = np.nan, 65535.0, 16
    surface = ref.surface_points(planes, u, W, H)[0]
    assert not surface[3, 5] and not surface[4, 6] and not surface[5, 7] and surface.sum() == W * H - 3
    out = ref.add_lights(planes, u, light((0.5, 0.5, 3.0), radius=30.0), floor_world(), W, H)
    for y, x in ((3, 5), (4, 6), (5, 7)):
        assert out["lighting_f32"][y, x].tobytes() == planes["lighting_f32"][y, x].tobytes()


def test_the_shadow_ray_agrees_with_the_oracles_trace_ray(procedural_region, blue_noise):
    """(point, light) pairs from a rendered 64x40 frame of the terrain fixture, lights 1 to 8 units off random hit points.  Where the
    oracle's trace_ray from P' reports air the restatement must say visible; a solid hit nearer than len - 2^-6: blocked; farther than
    len + 2^-6: visible.  Pairs inside that band are left out: measured share 0.0 % of 600 pairs with this seed (the bound is 5 %)."""
    mats, mine = procedural_region
    w, h = 64, 40
    u = po.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 5)
    planes, _ = po.render(mats, mine, blue_noise, u, w, h, 1, 2)
    surface, P, axis, even = ref.surface_points(planes, u, w, h)
    pts = P[surface]
    assert len(pts) > 500
    rng = np.random.default_rng(11)
    n = 600
    src = pts[rng.integers(0, len(pts), n)]
    off = rng.normal(size=(n, 3))
    off *= (rng.uniform(1.0, 8.0, n) / np.linalg.norm(off, axis=1))[:, None]
    lights = (src + off).astype(f32)
    near = rng.random(n) < 0.5                                       # half the pairs light the point they came from, half another one
    start = np.where(near[:, None], src, pts[rng.integers(0, len(pts), n)]).astype(f32)
    v = (lights - start).astype(f32)
    dist2 = ref.dot3(v, v)
    keep = dist2 > 0
    got = ref.trace_visible(mine, R, (0, 0, 0), start, v, dist2)
    length = np.sqrt(dist2.astype(np.float64))
    band = f32(2.0 ** -6)
    checked = left_out = 0
    for i in np.nonzero(keep)[0]:
        hit = po.trace_ray(mats, mine, start[i], v[i])
        if hit.limit_exit:
            continue
        if hit.air:
            assert got[i], "pair %d: the oracle's ray leaves the window" % i
        elif hit.distance < length[i] - band:
            assert not got[i], "pair %d: solid at %g before the light at %g" % (i, hit.distance, length[i])
        elif hit.distance > length[i] + band:
            assert got[i], "pair %d: solid at %g beyond the light at %g" % (i, hit.distance, length[i])
        else:
            left_out += 1
            continue
        checked += 1
    print("pairs checked %d, left out %d (%.2f %%), visible %d, blocked %d" % (checked, left_out, 100.0 * left_out / n, got[keep].sum(), (~got[keep]).sum()))
    assert left_out <= 0.05 * n and checked >= 0.9 * n
    assert got[keep].sum() > 50 and (~got[keep]).sum() > 50
