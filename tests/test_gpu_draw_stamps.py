"""Voxel-model entities on the GPU (rt_draw_stamps, rt_draw_stamps_async).  Every comparison is bit for bit, on all ten planes, with
tests/draw_stamps_ref.py — which has no cull and walks every model for every pixel — applied to the planes read back before the call:
the batch sizes round the kernel's 64-model batches and the 4096 limit on frames with partial tiles, the longest and the smallest
stamp, an adversarial set, the identity of a solid stamp with rt_draw_boxes on the device, the asynchronous call and its chaining
behind rt_probe_light_async, boxes and models in either order, every refusal, rt_stamp_destroy behind an enqueued draw, the absence
of leaks into the next frame and into the lighting history, and the host mirror."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from raytrace_amd import _lib, abi, render
from tests import draw_boxes_ref as boxes_ref
from tests import draw_stamps_ref as ref
from tests import entity_shadow_ref as shadow_ref
from tests import stamp_edits as se

pytestmark = pytest.mark.gpu

CACHE, ACC, REP, IN_FLIGHT_2 = abi.RT_FLAG_CACHE_PRIMARY, abi.RT_FLAG_ACCUMULATE, abi.RT_FLAG_REPROJECT, abi.RT_FLAG_FRAMES_IN_FLIGHT_2
POSE = dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.2, sun=0.3)
SHAPES = [(100, 60), (256, 128)]          # partial 8x8 tiles on both axes; whole tiles, several workgroups
COUNTS = [1, 63, 64, 65, 130, 4096]       # the 64-model batch edges and the limit
SCALES = [1.0 / 16.0, 0.37, 1.0, 2.5]
f32 = np.float32


def _u(seed=5, origin=None, pitch=None):
    return po.camera_uniforms(origin or POSE["origin"], POSE["heading"], POSE["pitch"] if pitch is None else pitch, POSE["sun"], seed, (0, 0, 0))


def _axis_u(seed=5):
    """Looks along +y with right = +x and up = +z: the middle column of an even-width frame has d_x == 0, the middle row d_z == 0."""
    u = _u(seed)
    for k in range(3):
        u.forward[k], u.right[k], u.up[k] = (0.0, 1.0, 0.0)[k], (0.4, 0.0, 0.0)[k], (0.0, 0.0, 0.4)[k]
    return u


def _ctx(scene, noise, W, H, **kw):
    kw.setdefault("flags", CACHE)
    ctx = render.Context(render.make_config(W, H, **kw))
    ctx.upload_world(*scene)
    ctx.upload_noise(noise)
    return ctx


def _all(ctx):
    """All ten planes."""
    return {abi.BUFFER_NAMES[b]: ctx.readback(b) for b in range(abi.RT_BUF_COUNT)}


def _assert_same(got, want, what=""):
    assert got.keys() == want.keys()
    for name in want:
        if got[name].tobytes() != want[name].tobytes():
            a, b = got[name].reshape(got[name].shape[0], got[name].shape[1], -1), want[name].reshape(want[name].shape[0], want[name].shape[1], -1)
            bad = np.argwhere((a.view(np.uint8) != b.view(np.uint8)).any(axis=-1))
            raise AssertionError("%s plane %s differs at %d pixels, first (row, col) %s" % (what, name, len(bad), bad[:5].tolist()))


def _restated(before, u, models, stamps, lights, W, H, won=None):
    want = ref.draw_stamps({k: v for k, v in before.items() if k != "final_bgra8"}, u, models, stamps, lights, W, H, won)
    want["final_bgra8"] = before["final_bgra8"]
    return want


def _restated_boxes(before, u, boxes, lights, W, H):
    want = boxes_ref.draw_boxes({k: v for k, v in before.items() if k != "final_bgra8"}, u, boxes, lights, W, H)
    want["final_bgra8"] = before["final_bgra8"]
    return want


def stamp_arrays(ext, seed, fill):
    """(materials u32[ez, ey, ex], state u8[ez, ey, ex]): fill = 1 is solid, otherwise that share solid and the rest air and absent."""
    rng = np.random.default_rng(seed)
    ex, ey, ez = ext
    rest = (1.0 - fill) / 2.0
    state = rng.choice(np.array([se.ABSENT, se.AIR, se.SOLID], dtype=np.uint8), size=(ez, ey, ex), p=[rest, rest, fill])
    mats = rng.integers(1, 1 << 21, size=(ez, ey, ex)).astype(np.uint32)
    mats[state == se.ABSENT] = 0
    return mats, state


FOUR = [((9, 9, 12), 1, 0.3), ((12, 5, 7), 2, 1.0), ((3, 11, 4), 3, 0.15), ((6, 6, 6), 4, 0.6)]   # sparse and solid, extents up to 12


def make_stamps(ctx, specs=FOUR):
    """{id: (materials, state)} of stamps created on ctx."""
    out = {}
    for ext, seed, fill in specs:
        mats, state = stamp_arrays(ext, seed, fill)
        out[ctx.stamp_create(mats, state)] = (mats, state)
    return out


def extents_of(models, stamps):
    return np.array([se.extent_of(stamps[int(s)][1]) for s in models["stamp"]]).reshape(-1, 3)


def scatter(u, n, seed, stamps, near=20.0, far=400.0, scales=SCALES):
    """n models spread over (and a little beyond) the view at log-uniform distances, of random stamps, scales, orientations and
    emissions.  A model of scale s starts no nearer than 80 s, so that it covers a few per cent of the view at the most."""
    rng = np.random.default_rng(seed)
    o, f, r, up = (np.array(v[:], dtype=np.float64) for v in (u.origin, u.forward, u.right, u.up))
    sx, sy = rng.uniform(-1.05, 1.05, n), rng.uniform(-1.05, 1.05, n)
    v = f[None] + r[None] * sx[:, None] + up[None] * sy[:, None]
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    ids = np.array(sorted(stamps), dtype=np.uint32)
    scale = np.array(scales)[rng.integers(0, len(scales), n)]
    nearest = np.minimum(np.maximum(near, 80.0 * scale), far / 2.0)
    c = o[None] + v * np.exp(rng.uniform(np.log(nearest), np.log(far), n))[:, None]
    return render.make_draw_stamps(ids[rng.integers(0, ids.size, n)], c - 4.0 * scale[:, None], scale, rng.integers(0, 48, n),
                                   rng.integers(0, 1 << 32, n, dtype=np.uint64))


def some_lights(n, seed=9):
    """6 n face lights: mostly what probes return (0 .. 20), with zeros, values that saturate the UNORM16 plane, a negative and a huge one."""
    rng = np.random.default_rng(seed)
    out = np.zeros(6 * n, dtype=render.PROBE_LIGHT_DTYPE)
    out["light"] = rng.random((6 * n, 3), dtype=np.float32) * f32(20.0)
    out["light"][rng.random(6 * n) < 0.05] = 0.0
    out["light"][::17, 1] = 400.0
    out["light"][3::29, 2] = -2.5
    out["light"][5::31, 0] = 1.0e30
    out["sun_samples"] = rng.integers(0, 5, 6 * n)
    return out


def _dev(records):
    return torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(len(records), -1).copy()).cuda()


@pytest.fixture(scope="module")
def frame_ctx(procedural_region, blue_noise):
    """One context per frame shape (spp 1 on the small terrain fixture) with the four stamps, shared by the tests that only need a
    frame to draw into."""
    made = {}
    for shape in SHAPES:
        ctx = _ctx(procedural_region, blue_noise, *shape, spp=1, depth=2)
        made[shape] = (ctx, make_stamps(ctx))
    yield made
    for ctx, _ in made.values():
        ctx.destroy()


def _fresh_frame(ctx, u):
    ctx.draw_frame(u)
    ctx.sync()
    return _all(ctx)


# ---- shapes and counts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_batches_equal_the_restatement(shape, count, frame_ctx):
    W, H = shape
    (ctx, stamps), u = frame_ctx[shape], _u()
    before = _fresh_frame(ctx, u)
    models, lights = scatter(u, count, 100 + count, stamps), some_lights(count)
    ctx.draw_stamps(u, models, lights)
    got = _all(ctx)
    won = ref.winners(u, models, stamps, W, H)
    stats, idx = ref.walk_stats(), won[1]
    _assert_same(got, _restated(before, u, models, stamps, lights, W, H, won), "count %d" % count)
    if count >= 63:    # the input is not trivial: models over sky and over terrain were drawn, others lost the depth test or missed
        drawn = got["depth_f32"] != before["depth_f32"]
        assert drawn[before["depth_r16"] == 65535].any() and drawn[before["depth_r16"] != 65535].any()
        assert count > 130 or np.count_nonzero((idx >= 0) & ~drawn) > 0           # (4096 models leave no pixel whose nearest one is hidden)
        assert stats["steps"] > stats["pairs"] > np.count_nonzero(idx >= 0)          # rays walked, and some walked through
        tiles = drawn[:H // 8 * 8, :W // 8 * 8].reshape(H // 8, 8, W // 8, 8).any(axis=(1, 3))
        assert tiles.any() and (count > 130 or not tiles.all())


def test_the_longest_and_the_smallest_stamp(frame_ctx):
    W, H = SHAPES[0]
    (ctx, _), u = frame_ctx[SHAPES[0]], _u()
    stamps = make_stamps(ctx, [((256, 1, 3), 7, 0.03), ((1, 1, 1), 8, 1.0)])
    long_id, one_id = sorted(stamps, key=lambda s: -stamps[s][1].size)
    o = np.array(u.origin[:])
    rows = [(long_id, o + (-30, 40, -6), 0.25, 0), (long_id, o + (-3, 30, -20), 0.25, 4 << 3 | 1), (long_id, o + (6, 50, -30), 0.37, 2 << 3 | 6),
            (long_id, o + (-8, 12, -3), 1.0 / 16.0, 1), (long_id, o + (-0.1, 20, -0.3), 0.25, 2 << 3),    # the last one seen lengthwise
            (one_id, o + (0, 10, -2), 1.0, 0), (one_id, o + (1, 6, -1), 1.0 / 16.0, 47),
            (one_id, o + (-20, 90, 5), 2.5, 13)]
    models = render.make_draw_stamps([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], 0xFF000003)
    lights = some_lights(len(rows))
    before = _fresh_frame(ctx, u)
    ctx.draw_stamps(u, models, lights)
    _assert_same(_all(ctx), _restated(before, u, models, stamps, lights, W, H), "256x1x3 and 1x1x1")
    _, idx, _, _, _ = ref.winners(u, models, stamps, W, H)
    assert set(np.unique(idx[idx >= 0]).tolist()) >= {0, 1, 2, 4, 5, 7} and ref.walk_stats()["max_steps"] > 24
    for s in stamps:
        ctx.stamp_destroy(s)


# ---- the adversarial set ----------------------------------------------------------------------------------------------------------------
def test_adversarial_set_equals_the_restatement(frame_ctx):
    W, H = SHAPES[0]
    (ctx, base), u = frame_ctx[SHAPES[0]], _axis_u()
    d = boxes_ref.directions(u, W, H)
    assert (d[:, W // 2, 0] == 0).all() and (d[H // 2, :, 2] == 0).all()
    extra = make_stamps(ctx, [((8, 8, 8), 21, 0.0), ((4, 4, 4), 22, 1.0), ((10, 10, 10), 23, 0.5), ((1, 256, 1), 24, 1.0), ((11, 10, 10), 25, 0.08)])
    absent, cube, half, pole, thin = sorted(extra, key=lambda s: [8 * 8 * 8, 64, 1000, 256, 1100].index(extra[s][1].size))
    stamps = {**base, **extra}
    o = np.array(u.origin[:], dtype=np.float64)            # the camera looks along +y
    big = 4194304.0
    rows = [
        (half, o - (2.5, 2.5, 2.5), 0.5, 0),                     # 0 the camera inside the bounding box
        (cube, o + (-2, -30, -2), 1.0, 0),                        # 1 behind the camera
        (half, o + (-6, -2, -2), 0.5, 9),                         # 2 straddling the camera plane, off axis
        (half, o + (1, 0, -3), 0.37, 3),                          # 3 touching the camera plane: origin_y == o_y
        (cube, (-big, o[1] + 100, o[2] + 20), 64.0, 0),           # 4 origin at -2^22, the largest scale (no model reaches the view from there)
        (pole, (o[0] + 14, o[1] + 60, -big), 64.0, 5 << 3),       # 5 origin at -2^22 on z: a pillar of 256 voxels of 64
        (cube, (big - 256.0, o[1] + 100, o[2] - 20), 64.0, 0),    # 6 hi at +2^22
        (half, o + (0.2, 0.5, -0.1), 1.0 / 256.0, 17),            # 7 the smallest scale, half a unit ahead
        (cube, o + (-0.3, 1.0, 0.1), 1.0 / 256.0, 0),             # 8 ... and a solid one
        (absent, o + (-4, 10, -4), 1.0, 0),                       # 9 nothing solid: never drawn
        (half, o + (40, 300, -125), 2.5, 30),                     # 10 wholly behind terrain
        (half, o + (-20, 195, -80), 2.5, 11),                     # 11 partly behind terrain
        (cube, o + (-30, 3000, -30), 16.0, 0),                    # 12 3000 units away
        (half, o + (0, 30, -12), 0.5, 0),                         # 13 origin_x == o_x: the d_x == 0 column sits on its face
        (half, o + (6, 25, 0), 0.5, 0),                           # 14 origin_z == o_z: the d_z == 0 row sits on its face
        (thin, o + (-2.2, 12, -2.7), 0.5, 21),                    # 15 dead ahead and sparse: the zero-component pixel walks a row of cells
        (half, o + (-2.5, 20, -2.5), 0.5, 0),                     # 16 behind it, and there along cell boundaries (o on a plane of both axes)
        (cube, o + (5, 30, -8), 0.5, 0), (cube, o + (5, 30, -8), 0.5, 0),   # 17, 18 two coincident models
    ]
    models = render.make_draw_stamps([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows],
                                     0xFF000000 + np.arange(len(rows)))
    assert ref.valid(models, stamps).all()
    lights = some_lights(models.size)
    before = _fresh_frame(ctx, u)
    ctx.draw_stamps(u, models, lights)
    got = _all(ctx)
    _assert_same(got, _restated(before, u, models, stamps, lights, W, H), "adversarial")
    _, idx, _, _, _ = ref.winners(u, models, stamps, W, H)
    won = set(np.unique(idx[idx >= 0]).tolist())
    assert {0, 1, 4, 5, 6, 9, 12, 18}.isdisjoint(won) and {2, 3, 7, 8, 10, 11, 13, 14, 15, 16, 17} <= won, won
    assert idx[H // 2, W // 2] in (15, 16) and {15, 16} <= set(idx[H // 2].tolist()) and {15, 16} <= set(idx[:, W // 2].tolist())
    drawn = got["depth_f32"] != before["depth_f32"]
    assert not drawn[idx == 10].any() and drawn[idx == 11].any() and not drawn[idx == 11].all() and not drawn[idx == 12].any()
    assert not (idx[:, W // 2] == 13).any() and not (idx[H // 2] == 14).any()
    for s in extra:
        ctx.stamp_destroy(s)


# ---- a solid stamp is rt_draw_boxes' box ------------------------------------------------------------------------------------------------
def test_solid_stamps_draw_what_rt_draw_boxes_draws(frame_ctx):
    W, H = SHAPES[1]
    (ctx, _), u = frame_ctx[SHAPES[1]], _u()
    rng = np.random.default_rng(77)
    stamps = {}
    for i in range(6):
        ext = tuple(int(v) for v in rng.integers(1, 13, 3))
        mats, state = np.full(ext[::-1], 0x2345 * (i + 3), dtype=np.uint32), np.full(ext[::-1], se.SOLID, dtype=np.uint8)
        stamps[ctx.stamp_create(mats, state)] = (mats, state)
    models = scatter(u, 200, 5, stamps, far=250.0, scales=[1.0 / 16.0, 0.37, 1.0, 2.5])
    lights = some_lights(models.size)
    boxes = ref.bounding_boxes(models, stamps, [stamps[int(s)][0].flat[0] for s in models["stamp"]])
    before = _fresh_frame(ctx, u)
    ctx.draw_boxes(u, boxes, lights)
    as_boxes = _all(ctx)
    _assert_same(_fresh_frame(ctx, u), before)
    ctx.draw_stamps(u, models, lights)
    _assert_same(_all(ctx), as_boxes, "solid stamps against their bounding boxes")
    assert np.count_nonzero(as_boxes["depth_f32"] != before["depth_f32"]) > 200
    for s in stamps:
        ctx.stamp_destroy(s)


# ---- async ------------------------------------------------------------------------------------------------------------------------------
def test_async_equals_sync_and_probes_chain_without_a_host_sync(frame_ctx):
    W, H = SHAPES[0]
    (ctx, stamps), u = frame_ctx[SHAPES[0]], _u()
    n = 40
    models = scatter(u, n, 21, stamps, far=100.0)
    probes = render.stamp_face_probes(models, extents_of(models, stamps), cells=np.stack([np.arange(n) % 16, np.arange(n) // 16], axis=-1))
    before = _fresh_frame(ctx, u)
    d_probes = _dev(probes)
    d_lights = torch.zeros((6 * n, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.probe_light_async(u, d_probes, d_lights, 4, 2)
    ctx.draw_stamps_async(u, models, d_lights)
    models_kept = models.copy()
    models[:] = 0                                                    # the records are free again when the call returns
    chained = _all(ctx)
    models = models_kept
    lights = ctx.probe_records(u, probes, 4, 2)
    assert d_lights.cpu().numpy().tobytes() == lights.tobytes() and np.count_nonzero(lights["light"]) > n
    _assert_same(chained, _restated(before, u, models, stamps, lights, W, H), "chained")
    _assert_same(_fresh_frame(ctx, u), before)
    ctx.draw_stamps(u, models, lights)
    _assert_same(_all(ctx), chained, "sync path")
    assert np.count_nonzero(chained["depth_f32"] != before["depth_f32"]) > 50
    # several asynchronous draws in a row, more than the staging sets, each with records of its own
    before = _fresh_frame(ctx, u)
    want, kept = before, []
    for k in range(5):
        part, part_lights = scatter(u, 30 + k, 300 + k, stamps, far=150.0), some_lights(30 + k, seed=k)
        kept.append(_dev(part_lights))                                 # (alive until the draws have run)
        torch.cuda.synchronize()
        ctx.draw_stamps_async(u, part, kept[-1])
        want = _restated(want, u, part, stamps, part_lights, W, H)
    _assert_same(_all(ctx), want, "five asynchronous draws")


# ---- boxes and models together ------------------------------------------------------------------------------------------------------------
def test_boxes_and_models_composite_by_depth_in_either_order(frame_ctx):
    W, H = SHAPES[0]
    (ctx, stamps), u = frame_ctx[SHAPES[0]], _u()
    models, model_lights = scatter(u, 80, 41, stamps, far=120.0), some_lights(80, seed=1)
    rng = np.random.default_rng(43)
    lo, _ = render.stamp_bounding_boxes(models[:60], extents_of(models[:60], stamps))
    lo = lo + rng.uniform(-1.0, 1.0, lo.shape)                         # boxes that overlap the models
    boxes = render.make_draw_boxes(lo, lo + rng.uniform(0.3, 2.0, lo.shape), rng.integers(0, 1 << 21, 60), 0xFF0000FF)
    box_lights = some_lights(60, seed=2)
    before = _fresh_frame(ctx, u)
    ctx.draw_boxes(u, boxes, box_lights)
    ctx.draw_stamps(u, models, model_lights)
    one = _all(ctx)
    _assert_same(one, _restated(_restated_boxes(before, u, boxes, box_lights, W, H), u, models, stamps, model_lights, W, H), "boxes then models")
    _assert_same(_fresh_frame(ctx, u), before)
    ctx.draw_stamps(u, models, model_lights)
    ctx.draw_boxes(u, boxes, box_lights)
    other = _all(ctx)
    _assert_same(other, _restated_boxes(_restated(before, u, models, stamps, model_lights, W, H), u, boxes, box_lights, W, H), "models then boxes")
    boxes_only = _restated_boxes(before, u, boxes, box_lights, W, H)
    models_only = _restated(before, u, models, stamps, model_lights, W, H)
    assert np.count_nonzero((one["depth_f32"] != boxes_only["depth_f32"])) > 30 and np.count_nonzero((one["depth_f32"] != models_only["depth_f32"])) > 30
    # the nearer surface wins whichever came first; only exact depth ties may differ
    assert np.count_nonzero(one["depth_f32"] != other["depth_f32"]) == 0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _code(fn, *a):
    with pytest.raises(render.RtError) as e:
        fn(*a)
    return e.value.code


def test_refusals_and_count_zero(procedural_region, blue_noise):
    W, H = 64, 40
    lib = _lib.amd()
    u = _u()
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        stamps = make_stamps(ctx)
        models, lights = scatter(u, 8, 3, stamps, far=60.0), some_lights(8)
        pm, pl = models.ctypes.data_as(C.c_void_p), lights.ctypes.data_as(C.c_void_p)
        h = ctx.handle
        d_lights = _dev(lights)
        dl = C.c_void_p(d_lights.data_ptr())
        assert _code(ctx.draw_stamps, u, models, lights) == abi.RT_ERR_NOT_READY            # no frame yet
        assert _code(ctx.draw_stamps_async, u, models, d_lights) == abi.RT_ERR_NOT_READY
        before = _fresh_frame(ctx, u)
        many = render.make_draw_stamps(sorted(stamps)[0], np.zeros((4096, 3)))
        many = np.concatenate([many, many[:1]])
        many_lights = np.zeros(6 * 4097, dtype=render.PROBE_LIGHT_DTYPE)
        d_many = _dev(many_lights)
        assert lib.rt_draw_stamps(h, C.byref(u), many.ctypes.data_as(C.c_void_p), many_lights.ctypes.data_as(C.c_void_p), 4097) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_draw_stamps_async(h, C.byref(u), many.ctypes.data_as(C.c_void_p), C.c_void_p(d_many.data_ptr()), 4097) == abi.RT_ERR_INVALID_ARG
        for call, l in ((lib.rt_draw_stamps, pl), (lib.rt_draw_stamps_async, dl)):
            assert call(h, None, pm, l, 8) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), None, l, 8) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), pm, None, 8) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), None, None, 0) == abi.RT_OK                         # count == 0 needs no arrays
        # host memory and unaligned device memory are not what the asynchronous call takes for the lights
        assert lib.rt_draw_stamps_async(h, C.byref(u), pm, pl, 8) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_draw_stamps_async(h, C.byref(u), pm, C.c_void_p(d_lights.data_ptr() + 4), 7) == abi.RT_ERR_INVALID_ARG
        big = 4194304.0
        unknown = max(stamps) + 1024                                 # a slot in use under a serial never issued
        changes = [("stamp", 0), ("stamp", unknown), ("stamp", max(stamps) + 1), ("orient", 48), ("reserved0", (0, 0, 1)), ("reserved", 1), ("scale", np.nan), ("scale", np.inf),
                   ("scale", 0.0039), ("scale", 64.001), ("origin", (np.nan, 0, 0)), ("origin", (0, -np.inf, 0)), ("origin", (0, 0, big + 1)),
                   ("origin", (big - 0.25, 0, 0))]
        for field, value in changes:
            bad = models.copy()
            bad[field][5] = value
            assert not ref.valid(bad, stamps)[5], (field, value)
            assert _code(ctx.draw_stamps, u, bad, lights) == abi.RT_ERR_INVALID_ARG, (field, value)
            assert _code(ctx.draw_stamps_async, u, bad, d_lights) == abi.RT_ERR_INVALID_ARG, (field, value)
        gone = models.copy()
        dead = ctx.stamp_create(*stamp_arrays((2, 2, 2), 1, 1.0))
        ctx.stamp_destroy(dead)
        gone["stamp"][2] = dead                                                            # a destroyed id stays unknown
        assert _code(ctx.draw_stamps, u, gone, lights) == abi.RT_ERR_INVALID_ARG
        _assert_same(_all(ctx), before, "after the rejected calls")
        ctx.draw_stamps(u, models[:0], lights[:0])                                          # count == 0 through the Python layer
        _assert_same(_all(ctx), before, "after count == 0")
        ctx.draw_stamps(u, models, lights)                                                  # and the context still works
        _assert_same(_all(ctx), _restated(before, u, models, stamps, lights, W, H))
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2, tile_rank=0, tile_world=2) as tiles:
        tstamps = make_stamps(tiles)
        tmodels = scatter(u, 8, 3, tstamps, far=60.0)
        tiles.draw_frame(u)
        tiles.sync()
        assert _code(tiles.draw_stamps, u, tmodels, lights) == abi.RT_ERR_UNIMPLEMENTED
        assert _code(tiles.draw_stamps_async, u, tmodels, _dev(lights)) == abi.RT_ERR_UNIMPLEMENTED


def test_count_zero_drops_no_prepass_and_a_draw_does(procedural_region, blue_noise):
    """RT_FLAG_TIMING_ALL counts a frame's launches: a frame that reuses its slot's prepass has one fewer."""
    W, H = 136, 72
    u = _u()
    with _ctx(procedural_region, blue_noise, W, H, spp=4, depth=2, kernel=abi.RT_KERNEL_PATHS, flags=CACHE | abi.RT_FLAG_TIMING_ALL) as ctx:
        stamps = make_stamps(ctx)
        models, lights = scatter(u, 24, 13, stamps, far=120.0), some_lights(24)

        def frame_launches():
            ctx.draw_frame(u)
            ctx.sync()
            return int(ctx.timing().other_launches)

        frame_launches()                                                 # (the first frame also builds the tables)
        ctx.denoise(True)                                                # writes the lighting plane: the next frame runs its prepass
        ctx.sync()
        ctx.timing()
        fresh, again = frame_launches(), frame_launches()
        assert again < fresh                                             # the second frame reused the slot's prepass
        ctx.draw_stamps(u, models[:0], lights[:0])
        ctx.sync()
        assert int(ctx.timing().other_launches) == 0                     # count == 0: nothing enqueued
        assert frame_launches() == again                                 # ... and the prepass is still the slot's
        ctx.draw_stamps(u, models, lights)
        ctx.sync()
        assert int(ctx.timing().other_launches) == 1                     # one launch per call
        assert frame_launches() == fresh                                 # the draw dropped the prepass


# ---- rt_stamp_destroy behind an enqueued draw -----------------------------------------------------------------------------------------------
def test_stamp_destroy_straight_after_an_async_draw(frame_ctx):
    W, H = SHAPES[1]
    (ctx, _), u = frame_ctx[SHAPES[1]], _u()
    stamps = make_stamps(ctx, [((12, 12, 12), 31, 0.2), ((9, 9, 12), 32, 0.3)])
    models, lights = scatter(u, 600, 51, stamps, far=200.0), some_lights(600)
    d_lights = _dev(lights)
    before = _fresh_frame(ctx, u)
    ctx.draw_frame(u)                                                  # the draw queues behind a frame
    ctx.draw_stamps_async(u, models, d_lights)
    for s in stamps:
        ctx.stamp_destroy(s)                                           # waits for the draw; the arrays are freed after it
    fill = [ctx.stamp_create(*stamp_arrays((12, 12, 12), 90 + k, 1.0)) for k in range(4)]   # what reuses the freed memory is not seen
    _assert_same(_all(ctx), _restated(before, u, models, stamps, lights, W, H), "draw, then destroy")
    assert _code(ctx.draw_stamps, u, models, lights) == abi.RT_ERR_INVALID_ARG
    for s in fill:
        ctx.stamp_destroy(s)


# ---- rt_draw_stamps and rt_shadow_entities take turns over the same two staging sets --------------------------------------------------------
class _DevBytes:
    """Zero-copy view of device memory for torch.as_tensor (CUDA array interface v2)."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


def _planes(copies):
    """The numpy planes of device copies made by test_draws_and_shadows_alternate_over_the_staging_sets."""
    W, H = 60, 36
    out = {}
    for b, t in copies.items():
        dt, ch = abi.BUFFER_FORMATS[b]
        out[abi.BUFFER_NAMES[b]] = t.cpu().numpy().view(dt).reshape((H, W, ch) if ch > 1 else (H, W))
    return out


def test_draws_and_shadows_alternate_over_the_staging_sets(procedural_region, blue_noise):
    """draw (3 models), shadows (1100: more than the 1024 records of a set's first 64 KiB, so the set grows while its twin's launch is
    still queued), draw (5), shadows (2) on one stream with no host sync in between — each step's planes are copied on that stream,
    device to device — against the same calls made synchronously, one by one, on a second context.  60 x 36: edge tiles on both axes."""
    W, H = 60, 36
    u = _u()
    specs = [((1, 1, 1), 41, 1.0), ((3, 2, 2), 42, 1.0)]                   # both solid: a ray through a model's centre hits it
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx, _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as twin:
        stamps = make_stamps(ctx, specs)
        assert sorted(make_stamps(twin, specs)) == sorted(stamps)           # (fresh contexts hand out the same ids)
        ids = np.array(sorted(stamps), dtype=np.uint32)
        # where models surely show or shade: halfway to a surface pixel, and eight units up the sun's line from a sunlit one
        before = _fresh_frame(twin, u)
        surface, P, axis, even = shadow_ref.surface_points(before, u, W, H)
        sun = shadow_ref.sun_of(u)[0].astype(np.float64)
        lit = np.zeros(surface.shape, dtype=bool)
        lit[surface] = shadow_ref.trace_kind(procedural_region[1], 256, (0, 0, 0), P[surface], shadow_ref.sun_of(u)[0]) == shadow_ref.AIR
        ys, xs = np.nonzero(lit & (axis == 2) & even)
        assert len(ys) >= 8
        near = np.argsort(before["depth_f32"][ys, xs], kind="stable")
        sunlit = P[ys[near], xs[near]].astype(np.float64)
        eye = np.array(u.origin[:], dtype=np.float64)

        def placed(centres, scale):
            which = np.arange(len(centres)) % 2
            half = 0.5 * scale * np.array([specs[k][0] for k in which], dtype=np.float64)
            return render.make_draw_stamps(ids[which], np.asarray(centres) - half, scale, 0, 0xFF102030)

        # 1100 models: a coarse lattice through the region, which mostly misses every tile's sun rays and is culled, and two that shade
        g = np.stack(np.meshgrid(*([np.arange(-120.0, 121.0, 24.0)] * 3), indexing="ij"), axis=-1).reshape(-1, 3)
        many = placed(np.concatenate([g[:1098], sunlit[[0, len(sunlit) // 2]] + 8.0 * sun]), 2.5)
        assert len(many) == 1100
        steps = [("draw", placed(eye + 0.5 * (sunlit[[1, 3, 5]] - eye), 1.0), some_lights(3, seed=1)), ("shade", many, None),
                 ("draw", placed(eye + 0.5 * (sunlit[[0, 2, 4, 6, 7]] - eye), 1.0), some_lights(5, seed=2)),
                 ("shade", placed(sunlit[[len(sunlit) // 3, 2]][::-1] + 8.0 * sun, 2.5), None)]
        # the same calls, synchronously
        want = []
        for kind, models, lights in steps:
            before = _fresh_frame(twin, u)
            if kind == "draw":
                twin.draw_stamps(u, models, lights)
            else:
                twin.shadow_entities(u, None, models)
            want.append(_all(twin))
            assert any(want[-1][k].tobytes() != before[k].tobytes() for k in before), "the step changes the frame"
        # ... and asynchronously on a caller's stream, nothing waited for until the last call has returned
        s = torch.cuda.Stream()
        d_lights = [None if lights is None else _dev(lights) for _, _, lights in steps]
        torch.cuda.synchronize()
        ctx.set_stream(s.cuda_stream)
        try:
            copies = []
            for (kind, models, _), d in zip(steps, d_lights):
                ctx.draw_frame(u)
                if kind == "draw":
                    ctx.draw_stamps_async(u, models, d)
                else:
                    ctx.shadow_entities_async(u, None, models)
                with torch.cuda.stream(s):
                    copies.append({b: torch.as_tensor(_DevBytes(ctx.device_ptr(b), ctx.buffer_bytes(b)), device="cuda").clone()
                                   for b in range(abi.RT_BUF_COUNT)})
            ctx.stamp_destroy(int(ids[1]))                                  # waits for the calls that read the stamp
            fill = ctx.stamp_create(*stamp_arrays((12, 12, 12), 95, 1.0))   # what reuses the freed memory is not seen
            s.synchronize()
            for k, (got, w) in enumerate(zip(copies, want)):
                _assert_same(_planes(got), w, "step %d" % k)
            _assert_same(_all(ctx), want[-1], "after the destroy")
            ctx.stamp_destroy(fill)
        finally:
            ctx.set_stream(0)


# ---- no leak into the next frame ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_flight", [1, 2])
def test_entity_pixels_do_not_leak_into_the_next_frame(in_flight, procedural_region, blue_noise):
    """The persistent route with cached primaries skips the prepass of a frame whose camera and world are unchanged: a slot whose
    planes rt_draw_stamps wrote must not be taken for one that still holds its prepass."""
    W, H = 136, 72
    u = _u()
    kw = dict(spp=4, depth=2, kernel=abi.RT_KERNEL_PATHS, flags=CACHE | (IN_FLIGHT_2 if in_flight == 2 else 0))
    nframes = 2 if in_flight == 1 else 3
    with _ctx(procedural_region, blue_noise, W, H, **kw) as clean:
        for _ in range(nframes):
            clean.draw_frame(u)
        clean.sync()
        want = _all(clean)
    with _ctx(procedural_region, blue_noise, W, H, **kw) as ctx:
        assert ctx.info().frames_in_flight == in_flight
        stamps = make_stamps(ctx)
        models, lights = scatter(u, 48, 13, stamps, far=120.0), some_lights(48)
        for k in range(nframes - 1):
            before = _fresh_frame(ctx, u)
            ctx.draw_stamps(u, models, lights)
            after = _all(ctx)
            assert np.count_nonzero(after["depth_f32"] != before["depth_f32"]) > 50
            _assert_same(after, _restated(before, u, models, stamps, lights, W, H), "frame %d" % k)
        _assert_same(_fresh_frame(ctx, u), want, "the frame after the models")


# ---- the lighting history is not touched ------------------------------------------------------------------------------------------------
def test_history_of_a_reprojecting_context_is_untouched(procedural_region, blue_noise):
    W, H = 96, 64
    kw = dict(spp=1, depth=2, flags=ACC | REP | CACHE)
    cams = [_u(seed=10 + k, origin=(-30.0 + 0.25 * k, -128.0, 100.0 - 0.1 * k)) for k in range(5)]
    with _ctx(procedural_region, blue_noise, W, H, **kw) as clean, _ctx(procedural_region, blue_noise, W, H, **kw) as ctx:
        stamps = make_stamps(ctx)
        models, lights = scatter(cams[0], 64, 17, stamps, far=120.0), some_lights(64)
        for k, u in enumerate(cams):
            want = _fresh_frame(clean, u)
            before = _fresh_frame(ctx, u)
            _assert_same(before, want, "frame %d before its models" % k)
            ctx.draw_stamps(u, models, lights)
            assert np.array_equal(ctx.read_history(), clean.read_history())
            assert ctx.accumulation() == clean.accumulation()
            after = _all(ctx)
            assert np.count_nonzero(after["depth_f32"] != before["depth_f32"]) > 50
        assert len(np.unique(clean.read_history())) > 1
        _assert_same(after, _restated(before, cams[-1], models, stamps, lights, W, H))


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------------
def test_the_mirror_draws_its_models_after_its_boxes(procedural_region, blue_noise):
    W, H = 96, 64
    cfg = render.make_config(W, H, spp=1, depth=2, flags=CACHE)
    g = render.Game(args=(-30, -128, 100, 1.5707964, -0.15, 0.3))
    g.set_world(*procedural_region)
    p = render.create_instance(cfg, g, blue_noise)
    p.enable_post_passes(faithful=True)
    specs = FOUR
    mirror_stamps = make_stamps(p.context, specs)
    cam = _u(pitch=-0.15)
    models = scatter(cam, 32, 37, mirror_stamps, far=100.0)
    lights = some_lights(32)
    rng = np.random.default_rng(5)
    lo, _ = render.stamp_bounding_boxes(models[:10], extents_of(models[:10], mirror_stamps))
    boxes, box_lights = render.make_draw_boxes(lo - 0.5, lo + rng.uniform(0.5, 2.0, lo.shape), 0x7F, 0xFF000000), some_lights(10, seed=4)
    p.set_boxes(boxes, box_lights)
    p.set_models(models, lights)
    uniforms = []
    for _ in range(2):
        p.draw_frame(g)
        p.wait()
        uniforms.append(abi.RtUniforms.from_buffer_copy(bytes(p.uniforms())))
    final = p.context.readback(abi.RT_BUF_FINAL_BGRA8)
    p.set_models(None, None)
    p.set_boxes(None, None)
    p.draw_frame(g)
    p.wait()
    bare = p.context.readback(abi.RT_BUF_FINAL_BGRA8)
    u_bare = abi.RtUniforms.from_buffer_copy(bytes(p.uniforms()))
    with pytest.raises(render.RtError):
        p.set_models(np.zeros(4097, dtype=render.DRAW_STAMP_DTYPE), np.zeros(6 * 4097, dtype=render.PROBE_LIGHT_DTYPE))
    p.close()
    g.close()
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        stamps = make_stamps(ctx, specs)
        mine = models.copy()
        mine["stamp"] = np.array(sorted(stamps), dtype=np.uint32)[np.searchsorted(sorted(mirror_stamps), models["stamp"])]
        for u in uniforms:
            ctx.draw_frame(u)
            ctx.draw_boxes(u, boxes, box_lights)
            ctx.draw_stamps(u, mine, lights)
            ctx.denoise(faithful=True)
            ctx.finalize()
        assert np.array_equal(ctx.readback(abi.RT_BUF_FINAL_BGRA8), final)
        ctx.draw_frame(u_bare)
        ctx.denoise(faithful=True)
        ctx.finalize()
        assert np.array_equal(ctx.readback(abi.RT_BUF_FINAL_BGRA8), bare)
    assert np.count_nonzero((final != bare).any(axis=-1)) > 30
