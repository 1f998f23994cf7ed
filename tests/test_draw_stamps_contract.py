"""The rules of rt_draw_stamps on the CPU: tests/draw_stamps_ref.py (the restatement the GPU tests compare with bit for bit) applied to
oracle-rendered 64x64 frames — a fully solid model is its bounding box drawn by rt_draw_boxes' rules, the 48 orientations are
stamp_edits.oriented()'s, absent and air voxels are equally see-through, a shell hides its inside, the walk keeps its step bound, a
sparse model agrees with its voxels drawn one box each, axis-aligned cameras walk the row they look along, and every invalid record is
refused."""
import numpy as np
import pytest

from oracle import pyoracle as po
from raytrace_amd import render, world
from tests import draw_boxes_ref as boxes_ref
from tests import draw_stamps_ref as ref
from tests import scenes
from tests import stamp_edits as se

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
    """Looks along +x with right = +y and up = +z: pixel (32, 32) of a 64x64 frame has direction (1, 0, 0) exactly."""
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


def sparse_stamp(ext, seed, fill=0.35):
    """An asymmetric model (materials u32[ez, ey, ex], state u8[ez, ey, ex]) with all three states and a material per voxel."""
    rng = np.random.default_rng(seed)
    ex, ey, ez = ext
    state = rng.choice(np.array([se.ABSENT, se.AIR, se.SOLID], dtype=np.uint8), size=(ez, ey, ex), p=[(1 - fill) / 2, (1 - fill) / 2, fill])
    state[0, 0, 0] = se.SOLID                                           # a marked corner, so that no orientation looks like another
    mats = rng.integers(1, 1 << 21, size=(ez, ey, ex)).astype(np.uint32)
    mats[state == se.ABSENT] = 0
    return mats, state


def solid_stamp(ext, material):
    ex, ey, ez = ext
    return np.full((ez, ey, ex), material, dtype=np.uint32), np.full((ez, ey, ex), se.SOLID, dtype=np.uint8)


# ---- a fully solid model is its bounding box ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.37, 1.0 / 16.0, 1.0, 2.5])
def test_a_solid_model_is_its_bounding_box(scale, terrain):
    u, planes = terrain
    rng = np.random.default_rng(int(scale * 1000))
    stamps, models = {}, []
    for i in range(12):
        ext = tuple(int(v) for v in rng.integers(1, 13, 3))
        stamps[100 + i] = solid_stamp(ext, 0x1234F * (i + 1) & 0x1FFFFF)
        at = in_front(u, rng.uniform(6, 260) * max(scale, 0.2), rng.uniform(-0.4, 0.4) * 40 * scale, rng.uniform(-0.4, 0.4) * 40 * scale)
        models.append(ref.model(100 + i, at, scale, int(rng.integers(0, 48)), 0xFF000000 + i))
    models = ref.batch(models)
    assert ref.valid(models, stamps).all()
    lights = lights_for(models.size)
    boxes = ref.bounding_boxes(models, stamps, [stamps[int(s)][0].flat[0] for s in models["stamp"]])
    want = boxes_ref.draw_boxes(planes, u, boxes, lights, W, H)
    got = ref.draw_stamps(planes, u, models, stamps, lights, W, H)
    assert same(got, want)
    assert np.count_nonzero(got["depth_f32"] != planes["depth_f32"]) > 30
    t, idx, axis, _, _ = ref.winners(u, models, stamps, W, H)
    bt, bidx, baxis, _ = boxes_ref.winners(u, boxes, W, H)
    assert np.array_equal(idx, bidx) and np.array_equal(t[idx >= 0], bt[idx >= 0]) and np.array_equal(axis[idx >= 0], baxis[idx >= 0])
    assert ref.walk_stats()["steps"] == 0                               # the first cell is solid: nobody steps


# ---- orientations ----------------------------------------------------------------------------------------------------------------------
def test_every_orientation_is_orientation_0_of_the_oriented_model(terrain):
    u, planes = terrain
    mats, state = sparse_stamp((5, 3, 7), seed=11, fill=0.5)
    at = in_front(u, 14.0, -1.0, -0.5)
    lights = lights_for(1)
    seen = set()
    for orient in range(48):
        stamps = {7: (mats, state), 8: (np.ascontiguousarray(se.oriented(mats, orient)), np.ascontiguousarray(se.oriented(state, orient)))}
        got = ref.draw_stamps(planes, u, ref.batch([ref.model(7, at, 0.37, orient)]), stamps, lights, W, H)
        want = ref.draw_stamps(planes, u, ref.batch([ref.model(8, at, 0.37, 0)]), stamps, lights, W, H)
        assert same(got, want), orient
        assert np.count_nonzero(got["albedo_rgba8"] != planes["albedo_rgba8"]) > 20
        seen.add(got["albedo_rgba8"].tobytes())
    assert len(seen) == 48                                               # and they are 48 different pictures


# ---- see-through states ------------------------------------------------------------------------------------------------------------------
def test_absent_and_air_are_equally_see_through(terrain):
    u, planes = terrain
    mats, state = sparse_stamp((9, 9, 12), seed=5)
    swapped = state.copy()
    swapped[state == se.AIR], swapped[state == se.ABSENT] = se.ABSENT, se.AIR
    all_air = np.where(state == se.SOLID, se.SOLID, se.AIR).astype(np.uint8)
    stamps = {1: (mats, state), 2: (mats, swapped), 3: (mats, all_air), 4: (mats, np.zeros_like(state)), 5: (mats, np.ones_like(state))}
    at = in_front(u, 20.0, -2.0, -2.0)
    lights = lights_for(1)
    pictures = [ref.draw_stamps(planes, u, ref.batch([ref.model(s, at, 0.5, 9)]), stamps, lights, W, H) for s in (1, 2, 3)]
    assert same(pictures[0], pictures[1]) and same(pictures[0], pictures[2])
    assert np.count_nonzero(pictures[0]["depth_f32"] != planes["depth_f32"]) > 50
    for s in (4, 5):                                                     # nothing solid: never drawn
        assert same(ref.draw_stamps(planes, u, ref.batch([ref.model(s, at, 0.5, 9)]), stamps, lights, W, H), planes)


def test_a_shell_with_an_empty_outer_layer_never_shows_its_inside(terrain):
    u, planes = terrain
    n = 9
    state = np.full((n, n, n), se.AIR, dtype=np.uint8)
    mats = np.full((n, n, n), 0x1FC000, dtype=np.uint32)                 # the shell: red
    state[1:-1, 1:-1, 1:-1] = se.SOLID
    inside = np.zeros((n, n, n), dtype=bool)
    inside[2:-2, 2:-2, 2:-2] = True
    mats[inside] = 0x00007F                                              # the inside: blue
    hollow = state.copy()
    hollow[inside] = se.ABSENT
    stamps = {1: (mats, state), 2: (mats, hollow)}
    lights = lights_for(1)
    blue = boxes_ref.albedo_rgba8(np.uint32(0x00007F)).tobytes()
    for scale, dist in ((1.0, 25.0), (1.0 / 16.0, 2.0), (2.5, 60.0)):
        at = in_front(u, dist, -4.0 * scale, -4.0 * scale)
        got = ref.draw_stamps(planes, u, ref.batch([ref.model(1, at, scale, 17)]), stamps, lights, W, H)
        drawn = got["depth_f32"] != planes["depth_f32"]
        assert np.count_nonzero(drawn) > 30
        assert not any(px.tobytes() == blue for px in got["albedo_rgba8"][drawn])
        assert same(got, ref.draw_stamps(planes, u, ref.batch([ref.model(2, at, scale, 17)]), stamps, lights, W, H))
        assert ref.walk_stats()["steps"] > 0                            # the outer layer was walked through


# ---- the step bound, and agreement with one box per voxel ------------------------------------------------------------------------------------
def test_the_walk_keeps_its_step_bound(terrain, sky):
    rng = np.random.default_rng(23)
    for (u, planes), dist in ((terrain, 30.0), (sky, 12.0)):
        stamps = {1: sparse_stamp((12, 12, 12), 1, fill=0.02), 2: sparse_stamp((64, 1, 3), 2, fill=0.05), 3: sparse_stamp((1, 1, 1), 3),
                  4: sparse_stamp((3, 40, 2), 4, fill=0.0)}
        models = ref.batch([ref.model(1 + i % 4, in_front(u, dist * rng.uniform(0.3, 2), rng.uniform(-8, 8), rng.uniform(-8, 8)),
                                      [1.0 / 16.0, 0.37, 1.0, 2.5][(i // 4) % 4], int(rng.integers(0, 48))) for i in range(48)])
        ref.winners(u, models, stamps, W, H)                             # (raises if a walk passes the bound)
        stats = ref.walk_stats()
        assert stats["bound_ok"] and stats["pairs"] > 500 and 0 < stats["max_steps"] <= 64 + 1 + 3


def test_a_sparse_model_agrees_with_one_box_per_voxel(terrain):
    """Each solid voxel as an rt_draw_boxes box between the model's own planes: in real arithmetic the first voxel a ray meets and the
    parameter at which it enters it are the walk's.  Rounding may move a tie, so a few pixels along voxel edges may differ."""
    u, planes = terrain
    mats, state = sparse_stamp((7, 6, 5), seed=31, fill=0.3)
    stamps = {1: (mats, state)}
    scale, at = f32(0.37), in_front(u, 9.0, -1.2, -0.8).astype(f32)
    m = ref.batch([ref.model(1, at, scale, 0, 0xFF000005)])
    z, y, x = np.nonzero(state == se.SOLID)
    cells = np.stack([x, y, z], axis=1)
    origin = np.repeat(m["origin"].astype(f32), len(cells), axis=0)
    sc = np.full(origin.shape, scale, dtype=f32)
    boxes = render.make_draw_boxes(boxes_ref.fma(cells.astype(f32), sc, origin), boxes_ref.fma((cells + 1).astype(f32), sc, origin),
                                   mats[z, y, x], 0xFF000005)
    got = ref.draw_stamps(planes, u, m, stamps, lights_for(1), W, H)
    t, idx, axis, material, _ = ref.winners(u, m, stamps, W, H)
    bt, bidx, baxis, _ = boxes_ref.winners(u, boxes, W, H)
    both = (idx >= 0) & (bidx >= 0)
    assert np.count_nonzero(both) > 200 and np.count_nonzero((idx >= 0) != (bidx >= 0)) <= 4
    agree = both & (material == boxes["material"][np.where(bidx >= 0, bidx, 0)]) & (axis == baxis) & (t == bt)
    assert np.count_nonzero(both & ~agree) <= 4
    assert np.count_nonzero(got["depth_f32"] != planes["depth_f32"]) > 200


# ---- axis-aligned cameras -------------------------------------------------------------------------------------------------------------------
def test_axis_aligned_rays_walk_the_row_they_look_along(sky):
    u, planes = sky
    d = boxes_ref.directions(u, W, H)
    assert tuple(d[32, 32]) == (1.0, 0.0, 0.0) and (d[32, :, 2] == 0).all() and (d[:, 32, 1] == 0).all()
    mats, state = sparse_stamp((10, 7, 9), seed=41, fill=0.25)
    stamps = {1: (mats, state)}
    o = np.array(u.origin[:])
    for scale in (1.0, 0.37, 1.0 / 16.0):
        # the camera's y and z lie strictly inside cell (., 3, 4) of the model
        at = (o + (6.0, 0.0, 0.0)) - np.array([0.0, 3.4, 4.6]) * scale
        m = ref.batch([ref.model(1, at, scale, 0)])
        t, idx, axis, material, _ = ref.winners(u, m, stamps, W, H)
        row = state[4, 3, :]
        if (row == se.SOLID).any():
            first = int(np.argmax(row == se.SOLID))
            assert idx[32, 32] == 0 and material[32, 32] == mats[4, 3, first] and axis[32, 32] == 0
            want_t = (boxes_ref.fma(np.array([first], dtype=f32), np.array([scale], dtype=f32), m["origin"][:, 0].astype(f32)) - f32(o[0])) * f32(1.0)
            assert t[32, 32] == want_t[0]
        else:
            assert idx[32, 32] == -1
        got = ref.draw_stamps(planes, u, m, stamps, lights_for(1), W, H)
        assert np.count_nonzero(got["depth_f32"] != planes["depth_f32"]) > 4
    # a solid model under the same camera is still its bounding box, zero components and all
    stamps[2] = solid_stamp((4, 5, 6), 0x7F3F9)
    m = ref.batch([ref.model(2, o + (8.0, -1.0, -1.5), 0.37, 29, 0xFF000001)])
    want = boxes_ref.draw_boxes(planes, u, ref.bounding_boxes(m, stamps, 0x7F3F9), lights_for(1), W, H)
    assert same(ref.draw_stamps(planes, u, m, stamps, lights_for(1), W, H), want)
    # and a camera whose zero-component ray lies ON a face of the bounding box does not enter it there
    m = ref.batch([ref.model(2, o + (8.0, 0.0, -1.5), 1.0, 0)])
    _, idx, _, _, _ = ref.winners(u, m, stamps, W, H)
    assert not (idx[:, 32] == 0).any() and (idx[:, 33] == 0).any()


# ---- the camera inside, invalid records ----------------------------------------------------------------------------------------------------
def test_a_camera_inside_the_bounding_box_does_not_see_the_model(terrain):
    u, planes = terrain
    stamps = {1: sparse_stamp((12, 12, 12), 3, fill=0.6)}
    o = np.array(u.origin[:])
    m = ref.batch([ref.model(1, o - 3.0, 0.5, 0)])
    assert ref.valid(m, stamps).all()
    assert same(ref.draw_stamps(planes, u, m, stamps, lights_for(1), W, H), planes)


def test_every_invalid_record_is_refused(terrain):
    u, planes = terrain
    stamps = {5: sparse_stamp((9, 9, 12), 3, fill=0.6), 6: solid_stamp((256, 1, 3), 1)}
    good = ref.model(5, in_front(u, 20.0), 0.5, 3)
    assert ref.valid(ref.batch([good]), stamps).all()
    big = 4194304.0

    def changed(**kw):
        m = good.copy()
        for k, v in kw.items():
            m[k] = v
        return m

    bad = [changed(stamp=0), changed(stamp=4), changed(orient=48), changed(orient=255), changed(reserved0=(0, 1, 0)), changed(reserved0=(0, 0, 7)),
           changed(reserved=1), changed(scale=np.nan), changed(scale=np.inf), changed(scale=0.0), changed(scale=-1.0),
           changed(scale=np.nextafter(f32(1.0 / 256.0), f32(0))), changed(scale=np.nextafter(f32(64.0), f32(100))),
           changed(origin=(np.nan, 0, 0)), changed(origin=(0, -np.inf, 0)), changed(origin=(0, 0, np.nextafter(f32(big), f32(1e9)))),
           changed(origin=(-np.nextafter(f32(big), f32(1e9)), 0, 0)),
           changed(origin=(big - 4.0, 0, 0)),                           # hi_x = 2^22 + 0.5
           changed(stamp=6, origin=(0, 0, big - 100.0), orient=5 << 3, scale=1.0)]   # orient (2, 1, 0): the 256 extent on z
    for m in bad:
        rec = ref.batch([good, m])
        assert ref.valid(rec, stamps).tolist() == [True, False], m
        # the restatement never draws it (the library refuses the whole call)
        assert same(ref.draw_stamps(planes, u, rec, stamps, lights_for(2), W, H), ref.draw_stamps(planes, u, rec[:1], stamps, lights_for(2)[:6], W, H))
    ok = [changed(scale=1.0 / 256.0), changed(scale=64.0), changed(origin=(big - 4.5, 0, 0)), changed(origin=(-big, -big, -big), scale=1.0 / 256.0),
          changed(orient=47), changed(emission=0x12345678)]
    assert ref.valid(ref.batch(ok), stamps).all()
