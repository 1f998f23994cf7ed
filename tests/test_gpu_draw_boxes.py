"""Entity boxes on the GPU (rt_draw_boxes, rt_draw_boxes_async).  Every comparison is bit for bit, on all ten planes, with
tests/draw_boxes_ref.py — which has no cull and tests every box against every pixel — applied to the planes read back before the call:
the batch sizes round the kernel's 64-box batches and the 4096 limit on frames with partial tiles, an adversarial set, the asynchronous
call and its chaining behind rt_probe_light_async, every refusal, the absence of leaks into the next frame and into the lighting
history, every kernel route, the post chain, and the host mirror."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from raytrace_amd import _lib, abi, render, world
from tests import draw_boxes_ref as ref

pytestmark = pytest.mark.gpu

CACHE, ACC, REP, IN_FLIGHT_2 = abi.RT_FLAG_CACHE_PRIMARY, abi.RT_FLAG_ACCUMULATE, abi.RT_FLAG_REPROJECT, abi.RT_FLAG_FRAMES_IN_FLIGHT_2
POSE = dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.2, sun=0.3)
SHAPES = [(100, 60), (256, 128)]          # partial 8x8 tiles on both axes; whole tiles, several workgroups
COUNTS = [1, 63, 64, 65, 130, 4096]       # the 64-box batch edges and the limit
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
    if scene is None:
        ctx.generate_world(world.DEFAULT_SEED)
    else:
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


def _restated(before, u, boxes, lights, W, H):
    want = ref.draw_boxes({k: v for k, v in before.items() if k != "final_bgra8"}, u, boxes, lights, W, H)
    want["final_bgra8"] = before["final_bgra8"]
    return want


def scatter(u, n, seed, near=20.0, far=400.0):
    """n entity-sized boxes spread over (and a little beyond) the view at log-uniform distances, with random materials and emissions."""
    rng = np.random.default_rng(seed)
    o, f, r, up = (np.array(v[:], dtype=np.float64) for v in (u.origin, u.forward, u.right, u.up))
    sx, sy = rng.uniform(-1.05, 1.05, n), rng.uniform(-1.05, 1.05, n)
    v = f[None] + r[None] * sx[:, None] + up[None] * sy[:, None]
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    c = o[None] + v * np.exp(rng.uniform(np.log(near), np.log(far), n))[:, None]
    half = rng.uniform(0.15, 1.0, (n, 3))
    return render.make_draw_boxes(c - half, c + half, rng.integers(0, 1 << 21, n), rng.integers(0, 1 << 32, n, dtype=np.uint64))


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
    """One context per frame shape (spp 1 on the small terrain fixture), shared by the tests that only need a frame to draw into."""
    made = {shape: _ctx(procedural_region, blue_noise, *shape, spp=1, depth=2) for shape in SHAPES}
    yield made
    for ctx in made.values():
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
    ctx, u = frame_ctx[shape], _u()
    before = _fresh_frame(ctx, u)
    boxes, lights = scatter(u, count, seed=100 + count), some_lights(count)
    ctx.draw_boxes(u, boxes, lights)
    got = _all(ctx)
    _assert_same(got, _restated(before, u, boxes, lights, W, H), "count %d" % count)
    if count >= 63:    # the input is not trivial: boxes over sky and over terrain were drawn, others lost the depth test or missed
        drawn = got["depth_f32"] != before["depth_f32"]
        assert drawn[before["depth_r16"] == 65535].any() and drawn[before["depth_r16"] != 65535].any()
        _, idx, _, _ = ref.winners(u, boxes, W, H)
        assert np.count_nonzero((idx >= 0) & ~drawn) > 0
        tiles = drawn[:H // 8 * 8, :W // 8 * 8].reshape(H // 8, 8, W // 8, 8).any(axis=(1, 3))
        assert tiles.any() and (count > 130 or not tiles.all())


# ---- the adversarial set ----------------------------------------------------------------------------------------------------------------
def adversarial_boxes(u):
    o = np.array(u.origin[:], dtype=np.float64)           # the camera looks along +y
    big = 4194304.0
    rows = [
        (o - (0.4, 0.4, 1.6), o + (0.4, 0.4, 0.2)),                                  # 0 the camera inside a box
        (o + (-1, -30, -1), o + (1, -28, 1)),                                        # 1 behind the camera
        (o + (-1.5, -2, -1), o + (-0.5, 3, 0.2)),                                    # 2 straddling the camera plane, off axis
        (o + (-900, 400, -900), o + (900, 402, 900)),                                # 3 covers the whole view, beyond the terrain
        (o + (-1, 9, 1), o + (0, 9.001, 2)),                                         # 4 1e-3 thin along the view
        (o + (3, 8, -3), o + (3.001, 14, -1)),                                       # 5 1e-3 thin across it
        (o + (-4, 12, 2), o + (-2, 16, 2.001)),                                      # 6 1e-3 thin, horizontal
        (o + (-20, 195, -90), o + (20, 215, -40)),                                   # 7 partly behind terrain
        (o + (40, 300, -125), o + (60, 310, -100)),                                 # 8 wholly behind terrain
        (o + (-8, 40, 10), o + (-2, 46, 14)),                                        # 9 over sky
        (o + (-30, 3000, -30), o + (30, 3020, 30)),                                  # 10 3000 units away
        (o + (5, 30, -8), o + (7, 32, -6)), (o + (5, 30, -8), o + (7, 32, -6)),      # 11, 12 two coincident boxes
        (o + (0, 30, -12), o + (4, 32, -9)),                                         # 13 lo_x == o_x: the d_x == 0 column sits on its face
        (o + (6, 25, 0), o + (9, 27, 3)),                                           # 14 lo_z == o_z: the d_z == 0 row sits on its face
        (o + (-1, 50, -1), o + (1, 52, 1)),                                          # 15 dead ahead: the zero-component pixel is strictly inside
        (o + (1, 0, -2), o + (2, 6, -1)),                                            # 16 a face plane through o (lo_y == o_y), seen from the side
        (o + (-1, 0, -1), o + (1, 5, 1)),                                            # 17 the camera ON a face: t_in == 0 for every ray
        ((o[0] + 14, o[1] + 60, -big), (o[0] + 15, o[1] + 61, big)),                 # 18 lo / hi at 2^22: a pillar through the view
        ((-big, o[1] + 100, o[2] + 20), (big, o[1] + 101, o[2] + 21)),               # 19 ... and a beam across it
    ]
    lo, hi = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    return render.make_draw_boxes(lo, hi, np.arange(len(rows)) * 0x1234F + 0x7F, 0xFF000000 + np.arange(len(rows)))


def test_adversarial_set_equals_the_restatement(frame_ctx):
    W, H = SHAPES[0]
    ctx, u = frame_ctx[SHAPES[0]], _axis_u()
    d = ref.directions(u, W, H)
    assert (d[:, W // 2, 0] == 0).all() and (d[H // 2, :, 2] == 0).all()
    before = _fresh_frame(ctx, u)
    boxes = adversarial_boxes(u)
    lights = some_lights(boxes.size)
    ctx.draw_boxes(u, boxes, lights)
    got = _all(ctx)
    _assert_same(got, _restated(before, u, boxes, lights, W, H), "adversarial")
    _, idx, _, _ = ref.winners(u, boxes, W, H)
    won = set(np.unique(idx[idx >= 0]).tolist())
    assert {0, 1, 10, 12, 17}.isdisjoint(won) and {2, 3, 4, 5, 6, 7, 8, 9, 11, 13, 14, 15, 16, 18, 19} <= won
    drawn = got["depth_f32"] != before["depth_f32"]
    assert not drawn[idx == 8].any() and drawn[idx == 7].any() and not drawn[idx == 7].all() and drawn[idx == 9].all()
    assert not (idx[:, W // 2] == 13).any() and (idx[:, W // 2 + 1] == 13).any()      # the zero-component column is not inside box 13
    assert not (idx[H // 2] == 14).any() and (idx[H // 2 + 1] == 14).any() and idx[H // 2, W // 2] == 15


# ---- async ------------------------------------------------------------------------------------------------------------------------------
def test_async_equals_sync_and_skips_out_of_domain_records(frame_ctx):
    W, H = SHAPES[0]
    ctx, u = frame_ctx[SHAPES[0]], _u()
    n = 96
    boxes, lights = scatter(u, n, seed=7, far=120.0), some_lights(n)
    bad = boxes.copy()
    hidden = boxes.copy()
    behind = np.array(u.origin[:]) - 50.0 * np.array(u.forward[:])
    for i, (field, k, value) in enumerate([("lo", 0, np.nan), ("hi", 2, np.nan), ("hi", 1, np.inf), ("lo", 2, -np.inf), ("lo", 1, 4194305.0),
                                           ("hi", 0, -4194305.0)]):
        bad[field][5 + 11 * i][k] = value
    bad["hi"][80] = bad["lo"][80]                                     # lo == hi
    bad["hi"][81][1] = bad["lo"][81][1] - 1                           # lo > hi
    skipped = ~ref.valid(bad)
    assert np.count_nonzero(skipped) == 8
    hidden["lo"][skipped], hidden["hi"][skipped] = behind - 1, behind + 1
    before = _fresh_frame(ctx, u)
    ctx.draw_boxes_async(u, _dev(bad), _dev(lights))
    got_bad = _all(ctx)
    _assert_same(got_bad, _restated(before, u, bad, lights, W, H), "async, out-of-domain records")
    before2 = _fresh_frame(ctx, u)
    _assert_same(before2, before)
    ctx.draw_boxes(u, hidden, lights)
    _assert_same(_all(ctx), got_bad, "sync with hidden boxes in their place")
    assert np.count_nonzero(got_bad["depth_f32"] != before["depth_f32"]) > 50


def test_probes_chain_into_boxes_without_a_host_sync(frame_ctx):
    W, H = SHAPES[0]
    ctx, u = frame_ctx[SHAPES[0]], _u()
    n = 40
    boxes = scatter(u, n, seed=21, far=100.0)
    probes = render.face_probes(boxes, cells=np.stack([np.arange(n) % 16, np.arange(n) // 16], axis=-1))
    before = _fresh_frame(ctx, u)
    d_probes, d_boxes = _dev(probes), _dev(boxes)
    d_lights = torch.zeros((6 * n, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.probe_light_async(u, d_probes, d_lights, 4, 2)
    ctx.draw_boxes_async(u, d_boxes, d_lights)
    chained = _all(ctx)
    lights = ctx.probe_records(u, probes, 4, 2)
    assert d_lights.cpu().numpy().tobytes() == lights.tobytes() and np.count_nonzero(lights["light"]) > n
    _assert_same(chained, _restated(before, u, boxes, lights, W, H), "chained")
    _assert_same(_fresh_frame(ctx, u), before)
    ctx.draw_boxes(u, boxes, lights)
    _assert_same(_all(ctx), chained, "sync path")
    assert np.count_nonzero(chained["depth_f32"] != before["depth_f32"]) > 50


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _code(fn, *a):
    with pytest.raises(render.RtError) as e:
        fn(*a)
    return e.value.code


def test_refusals(procedural_region, blue_noise):
    W, H = 64, 40
    lib = _lib.amd()
    u = _u()
    boxes, lights = scatter(u, 8, seed=3, far=60.0), some_lights(8)
    pb, pl = boxes.ctypes.data_as(C.c_void_p), lights.ctypes.data_as(C.c_void_p)
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        h = ctx.handle
        d_boxes, d_lights = _dev(boxes), _dev(lights)
        assert _code(ctx.draw_boxes, u, boxes, lights) == abi.RT_ERR_NOT_READY            # no frame yet
        assert _code(ctx.draw_boxes_async, u, d_boxes, d_lights) == abi.RT_ERR_NOT_READY
        before = _fresh_frame(ctx, u)
        many = np.zeros(4097, dtype=render.DRAW_BOX_DTYPE)
        many["hi"] = 1.0
        many_lights = np.zeros(6 * 4097, dtype=render.PROBE_LIGHT_DTYPE)
        assert lib.rt_draw_boxes(h, C.byref(u), many.ctypes.data_as(C.c_void_p), many_lights.ctypes.data_as(C.c_void_p), 4097) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_draw_boxes_async(h, C.byref(u), C.c_void_p(d_boxes.data_ptr()), C.c_void_p(d_lights.data_ptr()), 4097) == abi.RT_ERR_INVALID_ARG
        for call, b, l in ((lib.rt_draw_boxes, pb, pl), (lib.rt_draw_boxes_async, C.c_void_p(d_boxes.data_ptr()), C.c_void_p(d_lights.data_ptr()))):
            assert call(h, None, b, l, 8) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), None, l, 8) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), b, None, 8) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), None, None, 0) == abi.RT_OK                         # count == 0 needs no arrays
        # host memory and unaligned device memory are not what the asynchronous call takes
        assert lib.rt_draw_boxes_async(h, C.byref(u), pb, C.c_void_p(d_lights.data_ptr()), 8) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_draw_boxes_async(h, C.byref(u), C.c_void_p(d_boxes.data_ptr() + 4), C.c_void_p(d_lights.data_ptr()), 7) == abi.RT_ERR_INVALID_ARG
        for field, value in (("lo", np.nan), ("hi", np.inf), ("hi", -1.0e6), ("lo", 4194305.0)):
            bad = boxes.copy()
            bad[field][5][1] = value
            assert _code(ctx.draw_boxes, u, bad, lights) == abi.RT_ERR_INVALID_ARG
        _assert_same(_all(ctx), before, "after the rejected calls")
        ctx.draw_boxes(u, boxes, lights)                                                   # and the context still works
        _assert_same(_all(ctx), _restated(before, u, boxes, lights, W, H))
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2, tile_rank=0, tile_world=2) as tiles:
        tiles.draw_frame(u)
        tiles.sync()
        assert _code(tiles.draw_boxes, u, boxes, lights) == abi.RT_ERR_UNIMPLEMENTED
        assert lib.rt_draw_boxes_async(tiles.handle, C.byref(u), C.c_void_p(d_boxes.data_ptr()), C.c_void_p(d_lights.data_ptr()), 8) == abi.RT_ERR_UNIMPLEMENTED


# ---- no leak into the next frame ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_flight", [1, 2])
def test_entity_pixels_do_not_leak_into_the_next_frame(in_flight, procedural_region, blue_noise):
    """The persistent route with cached primaries skips the prepass of a frame whose camera and world are unchanged: a slot whose
    planes rt_draw_boxes wrote must not be taken for one that still holds its prepass."""
    W, H = 136, 72
    u = _u()
    boxes, lights = scatter(u, 48, seed=13, far=120.0), some_lights(48)
    kw = dict(spp=4, depth=2, kernel=abi.RT_KERNEL_PATHS, flags=CACHE | (IN_FLIGHT_2 if in_flight == 2 else 0))
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
            ctx.draw_boxes(u, boxes, lights)
            after = _all(ctx)
            assert np.count_nonzero(after["depth_f32"] != before["depth_f32"]) > 50
            _assert_same(after, _restated(before, u, boxes, lights, W, H), "frame %d" % k)
        _assert_same(_fresh_frame(ctx, u), want, "the frame after the boxes")


# ---- the lighting history is not touched ------------------------------------------------------------------------------------------------
def test_history_of_a_reprojecting_context_is_untouched(procedural_region, blue_noise):
    W, H = 96, 64
    kw = dict(spp=1, depth=2, flags=ACC | REP | CACHE)
    cams = [_u(seed=10 + k, origin=(-30.0 + 0.25 * k, -128.0, 100.0 - 0.1 * k)) for k in range(5)]
    boxes, lights = scatter(cams[0], 64, seed=17, far=120.0), some_lights(64)
    with _ctx(procedural_region, blue_noise, W, H, **kw) as clean, _ctx(procedural_region, blue_noise, W, H, **kw) as ctx:
        for k, u in enumerate(cams):
            want = _fresh_frame(clean, u)
            before = _fresh_frame(ctx, u)
            _assert_same(before, want, "frame %d before its boxes" % k)
            ctx.draw_boxes(u, boxes, lights)
            assert np.array_equal(ctx.read_history(), clean.read_history())
            assert ctx.accumulation() == clean.accumulation()
            after = _all(ctx)
            assert np.count_nonzero(after["depth_f32"] != before["depth_f32"]) > 50
        assert len(np.unique(clean.read_history())) > 1
        _assert_same(after, _restated(before, cams[-1], boxes, lights, W, H))


# ---- every route ------------------------------------------------------------------------------------------------------------------------
def test_every_route_and_region_draws_the_same_boxes(procedural_region, blue_noise):
    W, H = 100, 60
    u = _u()
    boxes, lights = scatter(u, 70, seed=29, far=150.0), some_lights(70)
    results, used = [], []
    for kernel in (abi.RT_KERNEL_FRAME, abi.RT_KERNEL_PATHS, abi.RT_KERNEL_PERSISTENT):
        with _ctx(procedural_region, blue_noise, W, H, spp=2, depth=2, kernel=kernel) as ctx:
            before = _fresh_frame(ctx, u)
            used.append(ctx.kernel_in_use())
            ctx.draw_boxes(u, boxes, lights)
            results.append((before, _all(ctx)))
    assert used == [abi.RT_KERNEL_FRAME, abi.RT_KERNEL_PATHS, abi.RT_KERNEL_PERSISTENT]
    _assert_same(results[0][1], _restated(results[0][0], u, boxes, lights, W, H), "k_frame")
    for before, after in results[1:]:
        _assert_same(before, results[0][0], "the routes' frames")
        _assert_same(after, results[0][1], "the routes' frames with boxes")
    with _ctx(None, blue_noise, W, H, spp=2, depth=2, region=512) as big:        # the region generated on the device
        before = _fresh_frame(big, u)
        big.draw_boxes(u, boxes, lights)
        _assert_same(_all(big), _restated(before, u, boxes, lights, W, H), "region 512")


# ---- the post chain and the mirror ------------------------------------------------------------------------------------------------------
def test_entity_pixels_go_through_the_unchanged_post_passes(frame_ctx, blue_noise):
    W, H = SHAPES[0]
    ctx, u = frame_ctx[SHAPES[0]], _u()
    boxes, lights = scatter(u, 60, seed=31, far=120.0), some_lights(60)
    before = _fresh_frame(ctx, u)
    ctx.draw_boxes(u, boxes, lights)
    ctx.denoise(faithful=True)
    ctx.finalize()
    got = _all(ctx)
    g = _restated(before, u, boxes, lights, W, H)
    den = po.denoise(g["lighting_rgba16"], g["depth_r16"], g["normal_r8"], faithful=True)
    fin = po.finalize(g["albedo_rgba8"], g["emission_rgba8"], g["fog_rgba8"], den, g["depth_r16"], blue_noise)
    assert np.array_equal(got["lighting_rgba16"], den) and np.array_equal(got["final_bgra8"], fin)
    plain = po.finalize(before["albedo_rgba8"], before["emission_rgba8"], before["fog_rgba8"],
                        po.denoise(before["lighting_rgba16"], before["depth_r16"], before["normal_r8"], faithful=True), before["depth_r16"], blue_noise)
    assert np.count_nonzero((fin != plain).any(axis=-1)) > 50                       # the entities are in the image


def test_the_mirror_draws_its_boxes_between_ray_trace_and_denoise(procedural_region, blue_noise):
    W, H = 96, 64
    cfg = render.make_config(W, H, spp=1, depth=2, flags=CACHE)
    g = render.Game(args=(-30, -128, 100, 1.5707964, -0.15, 0.3))
    g.set_world(*procedural_region)
    p = render.create_instance(cfg, g, blue_noise)
    p.enable_post_passes(faithful=True)
    boxes = scatter(_u(pitch=-0.15), 32, seed=37, far=100.0)
    lights = some_lights(32)
    p.set_boxes(boxes, lights)
    uniforms = []
    for _ in range(2):
        p.draw_frame(g)
        p.wait()
        uniforms.append(abi.RtUniforms.from_buffer_copy(bytes(p.uniforms())))
    final = p.context.readback(abi.RT_BUF_FINAL_BGRA8)
    p.set_boxes(None, None)
    p.draw_frame(g)
    p.wait()
    bare = p.context.readback(abi.RT_BUF_FINAL_BGRA8)
    u_bare = abi.RtUniforms.from_buffer_copy(bytes(p.uniforms()))
    with pytest.raises(render.RtError):
        p.set_boxes(np.zeros(4097, dtype=render.DRAW_BOX_DTYPE), np.zeros(6 * 4097, dtype=render.PROBE_LIGHT_DTYPE))
    p.close()
    g.close()
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        for u in uniforms:
            ctx.draw_frame(u)
            ctx.draw_boxes(u, boxes, lights)
            ctx.denoise(faithful=True)
            ctx.finalize()
        assert np.array_equal(ctx.readback(abi.RT_BUF_FINAL_BGRA8), final)
        ctx.draw_frame(u_bare)
        ctx.denoise(faithful=True)
        ctx.finalize()
        assert np.array_equal(ctx.readback(abi.RT_BUF_FINAL_BGRA8), bare)
    assert np.count_nonzero((final != bare).any(axis=-1)) > 30
