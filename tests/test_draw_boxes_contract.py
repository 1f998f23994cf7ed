"""The rules of rt_draw_boxes on the CPU: tests/draw_boxes_ref.py (the restatement the GPU tests compare with bit for bit) applied to
oracle-rendered 64x64 frames — what must leave a frame untouched, the two tie rules, the camera inside a box, the zero-component rule
on the centre pixel of an axis-aligned camera, the 2048-unit horizon, and what the feature means: a box drawn in the place of a carved
voxel cube gives the cube's normal, albedo and depth."""
import numpy as np
import pytest

from oracle import pyoracle as po
from raytrace_amd import render, world
from tests import draw_boxes_ref as ref
from tests import scenes, shader_formulas

W = H = 64
f32 = np.float32


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a) and a.keys() == b.keys()


def lights_for(n, seed=3):
    rng = np.random.default_rng(seed)
    out = np.zeros(6 * n, dtype=render.PROBE_LIGHT_DTYPE)
    out["light"] = rng.random((6 * n, 3), dtype=np.float32) * f32(20.0)
    return out


def axis_camera(origin):
    """Looks along +x with right = +y and up = +z (scaled 0.4 as the host scales them): pixel (32, 32) of a 64x64 frame has sx = sy = 0
    exactly, so its direction is (1, 0, 0) with d_y == d_z == 0."""
    u = po.camera_uniforms(origin, 0.0, 0.0, 0.3, 5)
    for k in range(3):
        u.origin[k] = float(origin[k])
        u.forward[k], u.right[k], u.up[k] = (1.0, 0.0, 0.0)[k], (0.0, 0.4, 0.0)[k], (0.0, 0.0, 0.4)[k]
    return u


@pytest.fixture(scope="module")
def terrain(procedural_region, blue_noise):
    mats, mine = procedural_region
    u = po.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 5)
    planes, _ = po.render(mats, mine, blue_noise, u, W, H, 1, 2)
    assert 0.2 < np.mean(planes["depth_r16"] == 65535) < 0.8          # sky and terrain both
    return u, planes


@pytest.fixture(scope="module")
def sky(native_built, blue_noise):
    """An empty region seen by the axis-aligned camera: every pixel is sky."""
    mats, mine = world.region_from_ids(scenes.empty_ids())
    u = axis_camera((0.5, 0.25, 0.75))
    planes, _ = po.render(mats, mine, blue_noise, u, W, H, 1, 2)
    assert (planes["depth_f32"] == f32(65535.0)).all()
    return u, planes


def in_front(u, dist, right=0.0, up=0.0):
    o, f = np.array(u.origin[:], dtype=np.float64), np.array(u.forward[:], dtype=np.float64)
    return o + f * dist + np.array(u.right[:]) / 0.4 * right + np.array(u.up[:]) / 0.4 * up


def test_direction_is_the_shaders_primary_direction(terrain):
    u, _ = terrain
    d = ref.directions(u, W, H)
    for px, py in ((0, 0), (63, 0), (17, 40), (32, 32), (63, 63)):
        want = shader_formulas.primary_direction(u.forward[:], u.up[:], u.right[:], px, py, W, H)
        assert np.abs(d[py, px].astype(np.float64) - want).max() < 1e-6


def test_the_restatements_shortcut_for_plain_frames_is_the_rule_itself(terrain):
    """draw_boxes_ref takes a shorter way through blocks of valid boxes when no direction component is zero; it is the same function."""
    u, _ = terrain
    rng = np.random.default_rng(5)
    d = ref.directions(u, W, H)
    inv = (f32(1.0) / d).astype(f32)
    o = np.array(u.origin[:], dtype=f32)
    c = np.array([in_front(u, t, r * t, v * t) for t, r, v in zip(rng.uniform(1, 200, 40), rng.uniform(-0.5, 0.5, 40), rng.uniform(-0.5, 0.5, 40))])
    half = rng.uniform(0.1, 30.0, (40, 3))
    c[:8] = o                                                           # some contain the camera
    lo, hi = (c - half).astype(f32), (c + half).astype(f32)
    lo[8:12, 0] = o[0]                                                  # a face through the origin
    a = ref._slab_general(lo, hi, o, d, inv, (40, H, W))
    b = ref._slab_plain(lo, hi, o, inv)
    assert a[3].all() and b[3] is True
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    hit = (a[0] > 0) & (a[0] < a[1])
    assert 0.01 < hit.mean() < 0.9


def test_no_boxes_invalid_boxes_and_hidden_boxes_leave_every_plane_as_it_was(terrain):
    u, planes = terrain
    empty = np.zeros(0, dtype=render.DRAW_BOX_DTYPE)
    assert same(ref.draw_boxes(planes, u, empty, lights_for(0), W, H), planes)
    c = in_front(u, 20.0)
    boxes = np.zeros(7, dtype=render.DRAW_BOX_DTYPE)
    boxes["lo"], boxes["hi"] = c - 1, c + 1                             # each would be drawn if it were valid ...
    boxes["lo"][0][0] = np.nan
    boxes["hi"][1][1] = np.inf
    boxes["hi"][2] = boxes["lo"][2]                                     # lo == hi
    boxes["hi"][3][2] = boxes["lo"][3][2] - 1                           # lo > hi
    boxes["lo"][4][0] = -4194305.0                                      # beyond 2^22
    behind = in_front(u, -20.0)
    boxes["lo"][5], boxes["hi"][5] = behind - 1, behind + 1             # valid, behind the camera
    far = in_front(u, 400.0, up=-150.0)
    boxes["lo"][6], boxes["hi"][6] = far - 1, far + 1                   # valid, deep inside the terrain
    assert ref.valid(boxes).tolist() == [False] * 5 + [True] * 2
    assert same(ref.draw_boxes(planes, u, boxes, lights_for(7), W, H), planes)
    # the same box, valid: drawn
    ok = render.make_draw_boxes([c - 1], [c + 1], 0x12345)
    assert not same(ref.draw_boxes(planes, u, ok, lights_for(1), W, H), planes)


def test_order_of_boxes_with_distinct_t_in_does_not_matter(terrain):
    u, planes = terrain
    rng = np.random.default_rng(11)
    n = 24
    dist = rng.uniform(8, 120, n)
    centres = np.array([in_front(u, d, r * d, v * d) for d, r, v in zip(dist, rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n))])
    half = rng.uniform(0.3, 2.5, (n, 3))
    boxes = render.make_draw_boxes(centres - half, centres + half, rng.integers(0, 1 << 21, n), rng.integers(0, 1 << 32, n, dtype=np.uint64))
    lights = lights_for(n)
    t_in, idx, _, _ = ref.winners(u, boxes, W, H)
    assert len(np.unique(idx[idx >= 0])) >= 8                            # several boxes win pixels, some overlap on screen
    base = ref.draw_boxes(planes, u, boxes, lights, W, H)
    assert np.count_nonzero(base["depth_f32"] != planes["depth_f32"]) > 100
    perm = rng.permutation(n)
    shuffled = ref.draw_boxes(planes, u, boxes[perm], lights.reshape(n, 6)[perm].reshape(-1), W, H)
    assert same(shuffled, base)


def test_of_two_identical_boxes_the_lower_index_wins(terrain):
    u, planes = terrain
    c = in_front(u, 15.0)
    boxes = render.make_draw_boxes([c - 1, c - 1], [c + 1, c + 1], [0x1FFFFF, 0x000000], [0xFF000000, 0xFF0000FF])
    lights = lights_for(2)
    out = ref.draw_boxes(planes, u, boxes, lights, W, H)
    first = ref.draw_boxes(planes, u, boxes[:1], lights[:6], W, H)
    second = ref.draw_boxes(planes, u, boxes[1:], lights[6:], W, H)
    assert same(out, first) and not same(out, second)
    assert same(ref.draw_boxes(planes, u, boxes[::-1], lights.reshape(2, 6)[::-1].reshape(-1), W, H), second)


def test_a_camera_inside_a_box_sees_nothing_of_it(terrain):
    u, planes = terrain
    o = np.array(u.origin[:])
    own = render.make_draw_boxes([o - (0.4, 0.4, 1.6)], [o + (0.4, 0.4, 0.2)], 0x3FFFF)      # the player's own box
    assert same(ref.draw_boxes(planes, u, own, lights_for(1), W, H), planes)
    huge = render.make_draw_boxes([o - 500], [o + 500], 0x3FFFF)
    assert same(ref.draw_boxes(planes, u, huge, lights_for(1), W, H), planes)
    # ... and it hides nothing: another box in front is drawn as if the first were not there
    c = in_front(u, 15.0)
    other = render.make_draw_boxes([c - 1], [c + 1], 0x155)
    both = np.concatenate([own, other])
    lights = lights_for(2)
    assert same(ref.draw_boxes(planes, u, both, lights, W, H), ref.draw_boxes(planes, u, other, lights[6:], W, H))


def test_zero_direction_components_pass_only_strictly_inside_the_slab(sky):
    u, planes = sky
    d = ref.directions(u, W, H)
    assert d[32, 32].tolist() == [1.0, 0.0, 0.0]
    o = np.array(u.origin[:], dtype=np.float32)                         # (0.5, 0.25, 0.75)

    def centre_drawn(lo, hi):
        out = ref.draw_boxes(planes, u, render.make_draw_boxes([lo], [hi], 0x7F), lights_for(1), W, H)
        return bool(out["depth_f32"][32, 32] != planes["depth_f32"][32, 32]), out

    hit, out = centre_drawn((5, 0, 0), (6, 1, 1))
    assert hit and out["normal_r8"][32, 32] == 1 and out["depth_f32"][32, 32] == f32(4.5 * 32)
    assert not centre_drawn((5, o[1], 0), (6, 1, 1))[0]                 # o_y == lo_y: not inside
    assert not centre_drawn((5, 0, 0), (6, o[1], 1))[0]                 # o_y == hi_y
    assert not centre_drawn((5, 0, o[2]), (6, 1, 1))[0]                 # o_z == lo_z
    assert not centre_drawn((5, 0, 0), (6, 1, o[2]))[0]                 # o_z == hi_z
    assert centre_drawn((5, np.nextafter(o[1], f32(-1)), 0), (6, np.nextafter(o[1], f32(1)), 1))[0]   # the thinnest slab round o_y
    # column 32 has d_y == 0 in every row, row 32 d_z == 0 in every column: the rule decides a whole line of pixels
    assert (d[:, 32, 1] == 0).all() and (d[32, :, 2] == 0).all()
    _, out = centre_drawn((5, o[1], -50), (6, 1, 50))
    assert not (out["depth_f32"][:, 32] != planes["depth_f32"][:, 32]).any()
    assert (out["depth_f32"][:, 33] != planes["depth_f32"][:, 33]).any()
    # a face plane through the origin on the bounded axis: t_in == 0 is no hit, the far side is not entered from inside
    assert not centre_drawn((o[0], 0, 0), (6, 1, 1))[0]


def test_a_box_2048_units_away_is_not_drawn_on_sky(sky):
    u, planes = sky
    o = np.array(u.origin[:], dtype=np.float64)
    near = render.make_draw_boxes([o + (2040, -5, -5)], [o + (2050, 5, 5)], 0x7F)
    out = ref.draw_boxes(planes, u, near, lights_for(1), W, H)
    assert out["depth_r16"][32, 32] == 65280 and out["normal_r8"][32, 32] == 1          # 2040 * 32
    far = render.make_draw_boxes([o + (2048, -50, -50)], [o + (2060, 50, 50)], 0x7F)
    assert same(ref.draw_boxes(planes, u, far, lights_for(1), W, H), planes)
    assert same(ref.draw_boxes(planes, u, render.make_draw_boxes([o + (3000, -900, -900)], [o + (3010, 900, 900)], 0), lights_for(1), W, H), planes)


# ---- what the feature means ---------------------------------------------------------------------------------------------------------
CUBE_LO, CUBE_HI, CUBE_ID = 12, 20, 4          # world coordinates of the 8^3 cube; texel = world + 128


def looking_at(origin, target):
    o, t = np.array(origin, dtype=np.float64), np.array(target, dtype=np.float64)
    f = (t - o) / np.linalg.norm(t - o)
    r = np.cross(f, (0.0, 0.0, 1.0))
    r /= np.linalg.norm(r)
    up = np.cross(r, f)
    u = po.camera_uniforms(origin, 0.0, 0.0, 0.3, 5)
    for k in range(3):
        u.forward[k], u.right[k], u.up[k] = float(f[k]), float(0.4 * r[k]), float(0.4 * up[k])
    return u


def test_a_box_in_the_place_of_a_carved_voxel_cube_looks_like_the_cube(native_built, blue_noise):
    ids = scenes.empty_ids()
    ids[128 + CUBE_LO:128 + CUBE_HI, 128 + CUBE_LO:128 + CUBE_HI, 128 + CUBE_LO:128 + CUBE_HI] = CUBE_ID
    u = looking_at((-21.3, -9.7, 33.1), (16.0, 16.0, 16.0))
    with_cube, _ = po.render(*world.region_from_ids(ids), blue_noise, u, W, H, 1, 2)
    carved, _ = po.render(*world.region_from_ids(scenes.empty_ids()), blue_noise, u, W, H, 1, 2)
    assert (carved["depth_r16"] == 65535).all()
    box = render.make_draw_boxes([(CUBE_LO,) * 3], [(CUBE_HI,) * 3], world.material_pack(CUBE_ID))
    drawn = ref.draw_boxes(carved, u, box, lights_for(1), W, H)
    cube_cov, box_cov = with_cube["depth_r16"] != 65535, drawn["depth_r16"] != 65535
    both = cube_cov & box_cov
    assert np.count_nonzero(both) > 150 and len(np.unique(with_cube["normal_r8"][both])) == 3      # three faces in view
    assert (with_cube["normal_r8"][both] == drawn["normal_r8"][both]).all()
    assert (with_cube["albedo_rgba8"][both] == drawn["albedo_rgba8"][both]).all()
    assert (with_cube["emission_rgba8"][both] == drawn["emission_rgba8"][both]).all()
    # the shader moves the hit 0.001 off the face before it measures the depth: 0.032 depth units
    assert np.abs(with_cube["depth_r16"][both].astype(np.int64) - drawn["depth_r16"][both].astype(np.int64)).max() <= 1
    # coverage may differ only on the silhouette: at pixels that have a differently-covered 8-neighbour in the world image
    pad = np.pad(cube_cov, 1, mode="edge")
    edge = np.zeros_like(cube_cov)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            edge |= pad[dy:dy + H, dx:dx + W] != cube_cov
    assert not ((cube_cov != box_cov) & ~edge).any()
    # the fog planes are the direction's alone: identical in all three images
    assert drawn["fog_rgba8"].tobytes() == with_cube["fog_rgba8"].tobytes() == carved["fog_rgba8"].tobytes()
