"""Point lights on the GPU (rt_add_lights, rt_add_lights_async).  Every comparison is bit for bit, on all ten planes, with
tests/point_light_ref.py — which has no cull, tests every light against every pixel and steps every shadow ray from the shader's
lines — applied to the planes read back before the call and to the minefield read back from the device: the batch sizes round the
kernel's 64-light batches and the 1024 limit on frames with partial tiles, an adversarial set, region 512, a scrolled window after a
streamed slab, entity pixels, the filtered plane, the asynchronous call, every refusal, the absence of leaks into the next frame and
the lighting history, two frames in flight, the ordering against world edits, every kernel route, the host mirror and rt_bench."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from raytrace_amd import _lib, abi, render, world
from tests import point_light_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CACHE, ACC, REP, IN_FLIGHT_2 = abi.RT_FLAG_CACHE_PRIMARY, abi.RT_FLAG_ACCUMULATE, abi.RT_FLAG_REPROJECT, abi.RT_FLAG_FRAMES_IN_FLIGHT_2
POSE = dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.2, sun=0.3)
SHAPES = [(100, 60), (64, 40)]            # partial 8x8 tiles on both axes; whole tiles
COUNTS = [1, 63, 64, 65, 130, 1024]       # the 64-light batch edges and the limit
f32 = np.float32


def _u(seed=5, origin=None, pitch=None, lr=(0, 0, 0)):
    return po.camera_uniforms(origin or POSE["origin"], POSE["heading"], POSE["pitch"] if pitch is None else pitch, POSE["sun"], seed, lr)


def _ctx(scene, noise, W, H, **kw):
    kw.setdefault("flags", CACHE)
    ctx = render.Context(render.make_config(W, H, **kw))
    if scene is None:
        ctx.generate_world(world.DEFAULT_SEED)
    else:
        ctx.upload_world(*scene)
    ctx.upload_noise(noise)
    return ctx


def _all(ctx):
    """All ten planes."""
    return {abi.BUFFER_NAMES[b]: ctx.readback(b) for b in range(abi.RT_BUF_COUNT)}


def _mine(ctx, R=256):
    """The resident region's minefield as the device holds it, [z][y][x] texels."""
    return ctx.read_box((0, 0, 0), (R, R, R))[1]


def _assert_same(got, want, what=""):
    assert got.keys() == want.keys()
    for name in want:
        if got[name].tobytes() != want[name].tobytes():
            a, b = got[name].reshape(got[name].shape[0], got[name].shape[1], -1), want[name].reshape(want[name].shape[0], want[name].shape[1], -1)
            bad = np.argwhere((a.view(np.uint8) != b.view(np.uint8)).any(axis=-1))
            raise AssertionError("%s plane %s differs at %d pixels, first (row, col) %s" % (what, name, len(bad), bad[:5].tolist()))


def _differ(a, b):
    return any(a[k].tobytes() != b[k].tobytes() for k in a)


def _restated(before, u, lights, mine, W, H, R=256):
    want = ref.add_lights({k: v for k, v in before.items() if k != "final_bgra8"}, u, lights, mine, W, H, R)
    want["final_bgra8"] = before["final_bgra8"]
    return want


def _lit(a, b):
    return (a["lighting_f32"] != b["lighting_f32"]).any(axis=-1)


def scatter(before, u, W, H, n, seed, rmin=2.0, rmax=12.0):
    """n lights just off the frame's surfaces: a random surface pixel's P', moved 0.2 to 5 units along its face's normal (one in ten
    the other way: into the ground) and up to 1.5 units sideways; radii rmin..rmax, colours up to 40 with some zeros."""
    rng = np.random.default_rng(seed)
    surface, P, axis, even = ref.surface_points(before, u, W, H)
    pts, ax, ev = P[surface].astype(np.float64), axis[surface], even[surface]
    assert len(pts) > 100
    j = rng.integers(0, len(pts), n)
    pos = pts[j] + rng.uniform(-1.5, 1.5, (n, 3))
    off = rng.uniform(0.2, 5.0, n) * np.where(ev[j], 1.0, -1.0) * np.where(rng.random(n) < 0.1, -1.0, 1.0)
    pos[np.arange(n), ax[j]] += off
    color = rng.random((n, 3)) * 40.0
    color[rng.random(n) < 0.05] = 0.0
    return render.make_point_lights(pos, rng.uniform(rmin, rmax, n), color)


def _dev(records):
    return torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(len(records), -1).copy()).cuda()


@pytest.fixture(scope="module")
def frame_ctx(procedural_region, blue_noise):
    """One context per frame shape (spp 1, depth 2 on the small terrain fixture), shared by the tests that only need a frame to light."""
    made = {shape: _ctx(procedural_region, blue_noise, *shape, spp=1, depth=2) for shape in SHAPES}
    yield made
    for ctx in made.values():
        ctx.destroy()


@pytest.fixture(scope="module")
def region_mine(procedural_region):
    return procedural_region[1]


def _fresh_frame(ctx, u):
    ctx.draw_frame(u)
    ctx.sync()
    return _all(ctx)


# ---- shapes and counts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_batches_equal_the_restatement(shape, count, frame_ctx, region_mine):
    W, H = shape
    ctx, u = frame_ctx[shape], _u()
    before = _fresh_frame(ctx, u)
    lights = scatter(before, u, W, H, count, seed=200 + count)
    ctx.add_lights(u, lights)
    got = _all(ctx)
    _assert_same(got, _restated(before, u, lights, region_mine, W, H), "count %d" % count)
    if count >= 63:    # the input is not trivial: lit and unlit surface pixels, shadowed pairs, untouched sky
        lit = _lit(got, before)
        surface = ref.surface_points(before, u, W, H)[0]
        assert lit.any() and not lit[~surface].any() and (~surface).any() and (count > 130 or not lit[surface].all())
        n = min(count, 130)
        surf, P, axis, even = ref.surface_points(before, u, W, H)
        passes = ref.pair_terms(P.reshape(-1, 3), axis.reshape(-1), even.reshape(-1), lights["position"][:n], lights["radius"][:n])[0] & surf.reshape(-1)[None]
        seen = ref.weights(before, u, lights[:n], region_mine, W, H)[1].reshape(n, -1)
        assert (passes & ~seen).any() and seen.any()                    # some pairs are in shadow, some are not


# ---- the adversarial set ----------------------------------------------------------------------------------------------------------------
def adversarial_lights(before, u, W, H):
    surface, P, axis, even = ref.surface_points(before, u, W, H)
    ys, xs = np.nonzero(surface)
    pick = lambda k: (ys[(k * 977) % len(ys)], xs[(k * 977) % len(ys)])
    rows = []

    def add(pos, radius, color=(20.0, 10.0, 5.0)):
        rows.append((np.asarray(pos, dtype=np.float64), float(radius), color))

    def off(k, dist):
        y, x = pick(k)
        p = P[y, x].astype(np.float64).copy()
        p[axis[y, x]] += dist if even[y, x] else -dist
        return p

    add(off(1, -1.5), 8.0)                                            # 0 inside the solid voxel under a surface
    p = off(2, 1.0)
    y, x = pick(2)
    p[axis[y, x]] = np.round(p[axis[y, x]])
    add(p, 6.0)                                                       # 1 on a face plane: an integer coordinate
    y, x = pick(3)
    add(P[y, x], 5.0)                                                 # 2 at a pixel's own P': dist2 == 0 there, its neighbours are lit
    for k, towards in ((4, np.inf), (5, -np.inf)):                    # 3, 4 radius one ulp above / below a pixel's sqrt(dist2)
        y, x = pick(k)
        pos = off(k, 3.0).astype(f32)
        v = (pos - P[y, x]).astype(f32)
        add(pos, np.nextafter(np.sqrt(ref.dot3(v, v)).astype(f32), f32(towards)))
    add((-30.0, -60.0, 300.0), 1024.0, (3000.0, 3000.0, 3000.0))      # 5 outside the window, radius 1024: its rays leave the window
    add((4194304.0, -4194304.0, 4194304.0), 1024.0)                   # 6 coordinates at 2^22: reaches nothing
    add(off(6, 2.0), 9.0, (1048576.0, 0.0, 1048576.0))                # 7 colour 2^20: the UNORM16 plane saturates
    add(off(7, 2.0), 9.0, (0.0, 0.0, 0.0))                            # 8 colour 0
    add(off(8, 0.01), 3.0)                                            # 9 a hair off the surface
    return render.make_point_lights(np.array([r[0] for r in rows]), [r[1] for r in rows], np.array([r[2] for r in rows]))


def test_adversarial_set_equals_the_restatement(frame_ctx, region_mine):
    W, H = SHAPES[0]
    ctx, u = frame_ctx[SHAPES[0]], _u()
    before = _fresh_frame(ctx, u)
    lights = adversarial_lights(before, u, W, H)
    ctx.add_lights(u, lights)
    got = _all(ctx)
    _assert_same(got, _restated(before, u, lights, region_mine, W, H), "adversarial")
    seen = ref.weights(before, u, lights, region_mine, W, H)[1]
    per_light = seen.reshape(len(lights), -1).sum(axis=1)
    t = np.floor(lights["position"][0]).astype(int) + 128
    assert region_mine[t[2], t[1], t[0]] == 0 and per_light[0] == 0                    # the light in the solid voxel lights nothing
    assert per_light[6] == 0 and per_light[5] > 100 and per_light[7] > 0 and per_light[8] > 0
    assert (got["lighting_rgba16"][seen[7]][:, 0] == 65535).any()
    # each light on its own too: a wrong cull of one could hide behind another's pixels
    for i in range(len(lights)):
        before = _fresh_frame(ctx, u)
        ctx.add_lights(u, lights[i:i + 1])
        _assert_same(_all(ctx), _restated(before, u, lights[i:i + 1], region_mine, W, H), "adversarial light %d alone" % i)


def test_a_frame_that_is_all_sky_keeps_every_bit(frame_ctx):
    W, H = SHAPES[0]
    ctx, u = frame_ctx[SHAPES[0]], _u(pitch=1.2)
    before = _fresh_frame(ctx, u)
    assert (before["depth_r16"] == 65535).all()
    o = np.array(u.origin[:]) + 5.0 * np.array(u.forward[:])
    ctx.add_lights(u, render.make_point_lights([o, o + 1.0], 1024.0, (100.0, 100.0, 100.0)))
    _assert_same(_all(ctx), before, "all sky")


# ---- regions and windows ----------------------------------------------------------------------------------------------------------------
def test_region_512(blue_noise):
    W, H = 64, 40
    u = _u()
    with _ctx(None, blue_noise, W, H, spp=1, depth=2, region=512) as big:          # the region generated on the device
        before = _fresh_frame(big, u)
        lights = scatter(before, u, W, H, 70, seed=41)
        mine = _mine(big, 512)
        big.add_lights(u, lights)
        got = _all(big)
        _assert_same(got, _restated(before, u, lights, mine, W, H, 512), "region 512")
        assert np.count_nonzero(_lit(got, before)) > 50


def test_a_scrolled_window_after_a_streamed_slab(procedural_region, blue_noise):
    """lr != 0: the kernel's other template.  The slab that entered at the window's far side is in the minefield the shadow rays read."""
    W, H = 100, 60
    lr = (16, 0, 0)
    u = _u(origin=(-14.0, -128.0, 100.0), lr=lr)
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        ctx.generate_slice(world.DEFAULT_SEED, 0, (128, -128, -128))                # world x 128..143 into texels 0..15
        before = _fresh_frame(ctx, u)
        mine = _mine(ctx)
        assert mine.tobytes() != procedural_region[1].tobytes()
        lights = scatter(before, u, W, H, 90, seed=43)
        # over the slab; outside the window; half a voxel under the slab's ground: with lr = 0 its rays would leave the window at x = 128
        far = render.make_point_lights([(136.0, -100.0, 60.0), (150.0, -100.0, 90.0), (141.5, -83.5, 40.5)], 1024.0, (500.0, 500.0, 500.0))
        assert mine[40 + 128, -84 + 128, 141 - 128] == 0 and procedural_region[1][40 + 128, -84 + 128, 141 - 128] != 0
        lights = np.concatenate([lights, far])
        ctx.add_lights(u, lights)
        got = _all(ctx)
        _assert_same(got, _restated(before, u, lights, mine, W, H), "lr %s" % (lr,))
        assert np.count_nonzero(_lit(got, before)) > 50
        zero = _u(origin=(-14.0, -128.0, 100.0))
        assert _differ(_restated(before, zero, lights, mine, W, H), got)            # lr is read


# ---- entity pixels and the filtered plane ------------------------------------------------------------------------------------------------
def test_entity_pixels_are_lit_through_the_boxes_depth_and_face(frame_ctx, region_mine):
    from tests.test_gpu_draw_boxes import scatter as scatter_boxes, some_lights
    W, H = SHAPES[0]
    ctx, u = frame_ctx[SHAPES[0]], _u()
    bare = _fresh_frame(ctx, u)
    boxes, face = scatter_boxes(u, 60, seed=31, far=120.0), some_lights(60)
    ctx.draw_boxes(u, boxes, face)
    before = _all(ctx)
    entity = before["depth_f32"] != bare["depth_f32"]
    assert entity.sum() > 50
    # lights off entity pixels only
    masked = dict(before)
    masked["normal_r8"] = np.where(entity, before["normal_r8"], 16).astype(np.uint8)
    lights = scatter(masked, u, W, H, 40, seed=47, rmin=3.0, rmax=10.0)
    ctx.add_lights(u, lights)
    got = _all(ctx)
    _assert_same(got, _restated(before, u, lights, region_mine, W, H), "after rt_draw_boxes")
    assert _lit(got, before)[entity].sum() > 20
    assert _differ(_restated(bare, u, lights, region_mine, W, H), got)


def test_after_the_denoise_each_plane_gets_the_light_in_its_own_representation(frame_ctx, region_mine, blue_noise):
    W, H = SHAPES[0]
    ctx, u = frame_ctx[SHAPES[0]], _u()
    raw = _fresh_frame(ctx, u)
    ctx.denoise(faithful=True)
    before = _all(ctx)
    assert before["lighting_rgba16"].tobytes() != raw["lighting_rgba16"].tobytes() and before["lighting_f32"].tobytes() == raw["lighting_f32"].tobytes()
    lights = scatter(before, u, W, H, 50, seed=53)
    ctx.add_lights(u, lights)
    got = _all(ctx)
    _assert_same(got, _restated(before, u, lights, region_mine, W, H), "after rt_denoise")
    lit = _lit(got, before)
    assert lit.sum() > 50 and (got["lighting_rgba16"][lit] != before["lighting_rgba16"][lit]).any()
    ctx.finalize()
    fin = po.finalize(got["albedo_rgba8"], got["emission_rgba8"], got["fog_rgba8"], got["lighting_rgba16"], got["depth_r16"], blue_noise)
    assert np.array_equal(ctx.readback(abi.RT_BUF_FINAL_BGRA8), fin)


# ---- async ------------------------------------------------------------------------------------------------------------------------------
def test_async_equals_sync_and_skips_invalid_records(frame_ctx, region_mine):
    W, H = SHAPES[0]
    ctx, u = frame_ctx[SHAPES[0]], _u()
    before = _fresh_frame(ctx, u)
    n = 96
    lights = scatter(before, u, W, H, n, seed=7)
    bad = lights.copy()
    bad["position"][5][0] = np.nan
    bad["color"][16][1] = -1.0
    bad["radius"][27] = 0.0
    bad["reserved"][38] = 1
    bad["radius"][49] = np.inf
    bad["color"][60][2] = 1048577.0
    bad["position"][71][2] = -4194305.0
    bad["radius"][82] = 1024.5
    skipped = ~ref.valid(bad)
    assert np.count_nonzero(skipped) == 8
    hidden = lights.copy()
    hidden["color"][skipped] = 0.0                                    # a valid light that adds nothing in the place of each
    ctx.add_lights_async(u, _dev(bad))
    got_bad = _all(ctx)
    _assert_same(got_bad, _restated(before, u, bad, region_mine, W, H), "async, invalid records")
    assert _differ(got_bad, _restated(before, u, lights, region_mine, W, H))          # the skipped lights would have been seen
    with pytest.raises(render.RtError) as e:
        ctx.add_lights(u, bad)
    assert e.value.code == abi.RT_ERR_INVALID_ARG
    _assert_same(_all(ctx), got_bad, "after the refused call")
    before2 = _fresh_frame(ctx, u)
    _assert_same(before2, before)
    ctx.add_lights(u, hidden)
    _assert_same(_all(ctx), got_bad, "sync with dark lights in their place")
    # ... and on a caller's stream
    s = torch.cuda.Stream()
    d = _dev(lights)
    torch.cuda.synchronize()
    ctx.set_stream(s.cuda_stream)
    try:
        ctx.draw_frame(u)
        ctx.add_lights_async(u, d)
        s.synchronize()
        _assert_same(_all(ctx), _restated(before, u, lights, region_mine, W, H), "on a caller's stream")
    finally:
        ctx.set_stream(0)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _code(fn, *a):
    with pytest.raises(render.RtError) as e:
        fn(*a)
    return e.value.code


def test_refusals(procedural_region, blue_noise):
    W, H = 64, 40
    lib = _lib.amd()
    u = _u()
    lights = render.make_point_lights([(-30.0, -100.0, 90.0)] * 8, 8.0, (10.0, 10.0, 10.0))
    pl = lights.ctypes.data_as(C.c_void_p)
    d_lights = _dev(lights)
    with render.Context(render.make_config(W, H, spp=1, depth=2, flags=CACHE)) as empty:
        empty.upload_noise(blue_noise)
        assert _code(empty.add_lights, u, lights) == abi.RT_ERR_NOT_READY                  # no frame, no world
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        h = ctx.handle
        assert _code(ctx.add_lights, u, lights) == abi.RT_ERR_NOT_READY                    # no frame yet
        assert _code(ctx.add_lights_async, u, d_lights) == abi.RT_ERR_NOT_READY
        before = _fresh_frame(ctx, u)
        lights = scatter(before, u, W, H, 8, seed=3)
        pl = lights.ctypes.data_as(C.c_void_p)
        d_lights = _dev(lights)
        many = np.concatenate([lights] * 129)[:1025].copy()
        d_many = _dev(many)
        assert lib.rt_add_lights(h, C.byref(u), many.ctypes.data_as(C.c_void_p), 1025) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_add_lights_async(h, C.byref(u), C.c_void_p(d_many.data_ptr()), 1025) == abi.RT_ERR_INVALID_ARG
        for call, p in ((lib.rt_add_lights, pl), (lib.rt_add_lights_async, C.c_void_p(d_lights.data_ptr()))):
            assert call(h, None, p, 8) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), None, 8) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), None, 0) == abi.RT_OK                               # count == 0 needs no array
        # host memory and unaligned device memory are not what the asynchronous call takes
        assert lib.rt_add_lights_async(h, C.byref(u), pl, 8) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_add_lights_async(h, C.byref(u), C.c_void_p(d_lights.data_ptr() + 4), 7) == abi.RT_ERR_INVALID_ARG
        for field, k, value in (("position", 1, np.nan), ("position", 0, 4194305.0), ("radius", None, 0.0), ("radius", None, -2.0),
                                ("radius", None, 1025.0), ("color", 2, -0.5), ("color", 0, np.inf), ("reserved", None, 3)):
            bad = lights.copy()
            if k is None:
                bad[field][5] = value
            else:
                bad[field][5][k] = value
            assert _code(ctx.add_lights, u, bad) == abi.RT_ERR_INVALID_ARG, (field, value)
        _assert_same(_all(ctx), before, "after the rejected calls")
        ctx.add_lights(u, lights)                                                          # and the context still works
        got = _all(ctx)
        _assert_same(got, _restated(before, u, lights, procedural_region[1], W, H))
        assert _lit(got, before).any()
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2, tile_rank=0, tile_world=2) as tiles:
        tiles.draw_frame(u)
        tiles.sync()
        assert _code(tiles.add_lights, u, lights) == abi.RT_ERR_UNIMPLEMENTED
        assert lib.rt_add_lights_async(tiles.handle, C.byref(u), C.c_void_p(d_lights.data_ptr()), 8) == abi.RT_ERR_UNIMPLEMENTED


# ---- no leak into the next frame ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["paths", "paths-2-in-flight", "frame"])
def test_the_light_does_not_leak_into_the_next_frame(route, procedural_region, blue_noise):
    """A still camera.  The persistent route with cached primaries skips the prepass of a frame whose camera and world are unchanged:
    a slot whose lighting rt_add_lights wrote must not be taken for one that still holds its prepass.  With two frames in flight the
    call lights the frame drawn last and leaves the other slot alone."""
    W, H = 136, 72
    u = _u()
    in_flight = 2 if route == "paths-2-in-flight" else 1
    kw = dict(spp=4, depth=2, kernel=abi.RT_KERNEL_PATHS, flags=CACHE | (IN_FLIGHT_2 if in_flight == 2 else 0))
    if route == "frame":
        kw = dict(spp=1, depth=2, kernel=abi.RT_KERNEL_FRAME, flags=CACHE)
    nframes = 2 if in_flight == 1 else 3
    with _ctx(procedural_region, blue_noise, W, H, **kw) as clean:
        for _ in range(nframes):
            clean.draw_frame(u)
        clean.sync()
        want = _all(clean)
    with _ctx(procedural_region, blue_noise, W, H, **kw) as ctx:
        assert ctx.info().frames_in_flight == in_flight
        for k in range(nframes - 1):
            before = _fresh_frame(ctx, u)
            lights = scatter(before, u, W, H, 48, seed=13 + k)
            ctx.add_lights(u, lights)
            after = _all(ctx)
            assert np.count_nonzero(_lit(after, before)) > 50
            _assert_same(after, _restated(before, u, lights, procedural_region[1], W, H), "frame %d" % k)
        _assert_same(_fresh_frame(ctx, u), want, "the frame after the lights")


def test_history_of_a_reprojecting_context_is_untouched(procedural_region, blue_noise):
    W, H = 96, 64
    kw = dict(spp=1, depth=2, flags=ACC | REP | CACHE)
    cams = [_u(seed=10 + k, origin=(-30.0 + 0.25 * min(k, 2), -128.0, 100.0 - 0.1 * min(k, 2))) for k in range(6)]   # moves, then holds still
    with _ctx(procedural_region, blue_noise, W, H, **kw) as clean, _ctx(procedural_region, blue_noise, W, H, **kw) as ctx:
        for k, u in enumerate(cams):
            want = _fresh_frame(clean, u)
            before = _fresh_frame(ctx, u)
            _assert_same(before, want, "frame %d before its lights" % k)
            if k < 3:                                               # the next three frames follow the last call
                lights = scatter(before, u, W, H, 64, seed=17 + k)
                ctx.add_lights(u, lights)
                after = _all(ctx)
                assert np.count_nonzero(_lit(after, before)) > 50
                _assert_same(after, _restated(before, u, lights, procedural_region[1], W, H), "frame %d" % k)
            assert np.array_equal(ctx.read_history(), clean.read_history())
            assert ctx.accumulation() == clean.accumulation()
        assert len(np.unique(clean.read_history())) > 1


# ---- ordering against world changes ---------------------------------------------------------------------------------------------------
def test_world_edits_and_lights_keep_their_order_without_a_host_sync(procedural_region, blue_noise):
    W, H = 100, 60
    u = _u()
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        before = _fresh_frame(ctx, u)
        surface, P, axis, even = ref.surface_points(before, u, W, H)
        ys, xs = np.nonzero(surface)
        k = np.argsort(before["depth_f32"][ys, xs], kind="stable")[len(ys) // 10]         # a near pixel: its surroundings fill many pixels
        y, x = ys[k], xs[k]
        a, s = int(axis[y, x]), (1.0 if even[y, x] else -1.0)
        pos = P[y, x].astype(np.float64).copy()
        pos[a] += 5.0 * s
        lights = render.make_point_lights([pos], 12.0, (60.0, 50.0, 40.0))
        # a wall one voxel thick, 17 x 17, two to three units off the surface, between it and the light
        lo = np.floor(pos).astype(int) - 8
        hi = np.floor(pos).astype(int) + 8
        lo[a] = hi[a] = int(np.floor(P[y, x][a] + 2.5 * s))
        wall = render.box_shape(lo + 128, hi + 128, material=0x1FFFFF, solid=True)
        gone = render.box_shape(lo + 128, hi + 128, material=0, solid=False)
        open_mine = _mine(ctx)
        ctx.edit_shapes([wall])                                       # no sync: the launch reads the minefield the edit leaves
        ctx.add_lights(u, lights)
        got = _all(ctx)
        walled_mine = _mine(ctx)
        assert walled_mine.tobytes() != open_mine.tobytes()
        walled, unwalled = _restated(before, u, lights, walled_mine, W, H), _restated(before, u, lights, open_mine, W, H)
        assert np.count_nonzero(_lit(unwalled, before)) > np.count_nonzero(_lit(walled, before)) + 5      # the wall casts a shadow
        _assert_same(got, walled, "edit, then lights")
        # the other way round: the asynchronous call, then an edit that removes the wall
        before2 = _fresh_frame(ctx, u)
        d = _dev(lights)
        torch.cuda.synchronize()
        ctx.add_lights_async(u, d)
        ctx.edit_shapes([gone])
        ctx.sync()
        got2 = _all(ctx)
        after_mine = _mine(ctx)
        assert after_mine.tobytes() != walled_mine.tobytes()
        _assert_same(got2, _restated(before2, u, lights, walled_mine, W, H), "lights, then edit")
        assert _differ(got2, _restated(before2, u, lights, after_mine, W, H))


# ---- every route ------------------------------------------------------------------------------------------------------------------------
def test_every_route_lights_the_same_frame(procedural_region, blue_noise):
    W, H = 100, 60
    u = _u()
    results, used = [], []
    routes = (abi.RT_KERNEL_FRAME, abi.RT_KERNEL_PATHS, abi.RT_KERNEL_PERSISTENT, abi.RT_KERNEL_WAVEFRONT, abi.RT_KERNEL_MEGA)
    lights = None
    for kernel in routes:
        with _ctx(procedural_region, blue_noise, W, H, spp=2, depth=2, kernel=kernel) as ctx:
            before = _fresh_frame(ctx, u)
            used.append(ctx.kernel_in_use())
            if lights is None:
                lights = scatter(before, u, W, H, 70, seed=29)
            ctx.add_lights(u, lights)
            results.append((before, _all(ctx)))
    assert used == list(routes)
    _assert_same(results[0][1], _restated(results[0][0], u, lights, procedural_region[1], W, H), "k_frame")
    assert np.count_nonzero(_lit(results[0][1], results[0][0])) > 50
    for before, after in results[1:]:
        _assert_same(before, results[0][0], "the routes' frames")
        _assert_same(after, results[0][1], "the routes' frames with lights")


# ---- the mirror and the bench binary ------------------------------------------------------------------------------------------------------
def test_the_mirror_adds_its_lights_between_ray_trace_and_denoise(procedural_region, blue_noise):
    W, H = 96, 64
    cfg = render.make_config(W, H, spp=1, depth=2, flags=CACHE)
    g = render.Game(args=(-30, -128, 100, 1.5707964, -0.15, 0.3))
    g.set_world(*procedural_region)
    p = render.create_instance(cfg, g, blue_noise)
    p.enable_post_passes(faithful=True)
    p.draw_frame(g)
    p.wait()
    lights = scatter(_all(p.context), abi.RtUniforms.from_buffer_copy(bytes(p.uniforms())), W, H, 32, seed=37)
    p.set_lights(lights)
    uniforms = []
    for _ in range(2):
        p.draw_frame(g)
        p.wait()
        uniforms.append(abi.RtUniforms.from_buffer_copy(bytes(p.uniforms())))
    final = p.context.readback(abi.RT_BUF_FINAL_BGRA8)
    p.set_lights(None)
    p.draw_frame(g)
    p.wait()
    bare = p.context.readback(abi.RT_BUF_FINAL_BGRA8)
    u_bare = abi.RtUniforms.from_buffer_copy(bytes(p.uniforms()))
    with pytest.raises(render.RtError):
        p.set_lights(np.zeros(1025, dtype=render.POINT_LIGHT_DTYPE))
    p.close()
    g.close()
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        for u in uniforms:
            ctx.draw_frame(u)
            ctx.add_lights(u, lights)
            ctx.denoise(faithful=True)
            ctx.finalize()
        assert np.array_equal(ctx.readback(abi.RT_BUF_FINAL_BGRA8), final)
        ctx.draw_frame(u_bare)
        ctx.denoise(faithful=True)
        ctx.finalize()
        assert np.array_equal(ctx.readback(abi.RT_BUF_FINAL_BGRA8), bare)
    assert np.count_nonzero((final != bare).any(axis=-1)) > 30


def test_rt_bench_lights_runs_and_reports(native_built):
    exe = os.path.join(ROOT, "raytrace_amd", "rt_bench")
    r = subprocess.run([exe, "--width", "128", "--height", "96", "--lights", "16"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["lights"] == 16 and j["launches_per_call"] == 1.0 and j["add_lights_device_ms"] > 0 and j["add_lights_call_ms"] > 0
    assert j["pixels_lit"] > 50
    bad = subprocess.run([exe, "--lights", "1025"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--lights" in bad.stderr
