"""Particles on the GPU (rt_draw_particles, rt_draw_particles_async).  Every comparison is bit for bit, on all ten planes, with
tests/draw_particles_ref.py — the reduction to tests/draw_boxes_ref.py, which has no cull and no bins and tests every box against
every pixel — applied to the planes read back before the call: counts round the 64-index batches and far beyond rt_draw_boxes'
limit on frames of whole and of ragged tiles, an adversarial set, rt_draw_boxes itself on the expanded records, the asynchronous
call and its chaining behind rt_probe_light_async, composition with boxes and models, every refusal, the scratch growing and not
shrinking, and the absence of leaks into the next frame and into the lighting history."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from raytrace_amd import _lib, abi, render
from tests import draw_boxes_ref as boxes_ref
from tests import draw_particles_ref as ref
from tests import draw_particles_sets as sets
from tests import draw_stamps_ref as stamps_ref
from tests import test_gpu_draw_stamps as stamps_t

pytestmark = pytest.mark.gpu

CACHE, ACC, REP, IN_FLIGHT_2 = abi.RT_FLAG_CACHE_PRIMARY, abi.RT_FLAG_ACCUMULATE, abi.RT_FLAG_REPROJECT, abi.RT_FLAG_FRAMES_IN_FLIGHT_2
POSE = dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.2, sun=0.3)
SHAPES = [(72, 40), (70, 45)]             # 9 x 5 whole tiles; ragged edge tiles on both axes
COUNTS = [1, 63, 64, 65, 5000]            # the 64-index batch edges, and more than rt_draw_boxes takes
NLIGHTS = 7
f32 = np.float32


def _u(seed=5, origin=None, pitch=None):
    return po.camera_uniforms(origin or POSE["origin"], POSE["heading"], POSE["pitch"] if pitch is None else pitch, POSE["sun"], seed, (0, 0, 0))


def _axis_u(seed=5):
    """Looks along +y with right = +x and up = +z."""
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


def _through(fn, before, *a):
    """A restatement applied to all ten planes (none of them writes final_bgra8)."""
    want = fn({k: v for k, v in before.items() if k != "final_bgra8"}, *a)
    want["final_bgra8"] = before["final_bgra8"]
    return want


def _restated(before, u, particles, lights, W, H):
    return _through(ref.draw_particles, before, u, particles, lights, W, H)


def _restated_boxes(before, u, boxes, lights, W, H):
    return _through(boxes_ref.draw_boxes, before, u, boxes, lights, W, H)


def _dev(records):
    return torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(len(records), -1).copy()).cuda()


def cloud_with_twins(u, n, seed, **kw):
    """A seeded cloud whose last tenth repeats its first tenth's cubes with other materials, emissions and lights: equal t_in rivals."""
    p = sets.cloud(u, n, seed, nlights=NLIGHTS, **kw)
    k = n // 10
    if k:
        p["center"][n - k:], p["half"][n - k:] = p["center"][:k], p["half"][:k]
    return p, k


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
def test_clouds_equal_the_restatement(shape, count, frame_ctx):
    W, H = shape
    ctx, u = frame_ctx[shape], _u()
    before = _fresh_frame(ctx, u)
    particles, twins = cloud_with_twins(u, count, seed=100 + count)
    lights = sets.some_lights(NLIGHTS)
    # what the input must be, asked of the restatement alone
    want = _restated(before, u, particles, lights, W, H)
    if count >= 63:
        boxes, _ = ref.expand(particles, lights)
        _, idx, _, _ = boxes_ref.winners(u, boxes, W, H)
        drawn = want["depth_f32"] != before["depth_f32"]
        assert drawn.any() and np.count_nonzero((idx >= 0) & ~drawn) > 0                  # some pixel is drawn, some hit loses the depth test
        assert (drawn & (idx >= 0) & (idx < twins)).any()                                 # a drawn winner had a rival of equal t_in: its twin
        assert drawn[before["depth_r16"] == 65535].any() and drawn[before["depth_r16"] != 65535].any()
    ctx.draw_particles(u, particles, lights)
    _assert_same(_all(ctx), want, "count %d" % count)


# ---- the adversarial set ----------------------------------------------------------------------------------------------------------------
def test_adversarial_set_equals_the_restatement(frame_ctx):
    W, H = SHAPES[0]
    ctx, u = frame_ctx[SHAPES[0]], _axis_u()
    before = _fresh_frame(ctx, u)
    particles, nlights, notes = sets.adversarial(u, W, H)
    lights = sets.some_lights(nlights)
    want = _restated(before, u, particles, lights, W, H)
    boxes, _ = ref.expand(particles, lights)
    _, idx, _, _ = boxes_ref.winners(u, boxes, W, H)
    drawn = want["depth_f32"] != before["depth_f32"]
    won = set(np.unique(idx[idx >= 0]).tolist())
    assert drawn.any() and np.count_nonzero((idx >= 0) & ~drawn) > 0
    first, second, third = notes["duplicates"]
    assert drawn[idx == first].any() and second not in won and third not in won            # the lowest index of equal cubes shows
    assert not drawn[idx == notes["too_far"]].any() and notes["behind_terrain"] not in set(np.unique(idx[drawn]).tolist())
    assert len(set(particles["light"][ref.valid(particles, nlights)].tolist())) < np.count_nonzero(ref.valid(particles, nlights)) // 4   # shared lights
    ctx.draw_particles_async(u, _dev(particles), _dev(lights))                             # (the synchronous call refuses the invalid records)
    _assert_same(_all(ctx), want, "adversarial")
    assert abi.RT_ERR_INVALID_ARG == _code(ctx.draw_particles, u, particles, lights)


def test_tile_block_and_wide_lists_together(procedural_region, blue_noise):
    """A frame of 41 x 25 tiles, 6 x 4 blocks of 8 x 8 tiles: cubes from under a pixel to the whole frame, so that some are listed by
    tile, some by block and some — more than 16 blocks — on the wide list, in one call with a cloud of small ones."""
    W, H = 328, 200
    u = _axis_u()
    o = np.array(u.origin[:], dtype=np.float64)
    lights = sets.some_lights(NLIGHTS)
    sizes = (0.01, 0.1, 0.5, 1.0, 2.0, 3.0, 4.5, 6.0, 9.0, 14.0, 30.0)
    sweep = render.make_particles([o + (3.0 * k - 15.0, 60.0 + 2.0 * k + 2.2 * sizes[k], 1.5 * k - 8.0) for k in range(len(sizes))] + [o + (0.0, 450.0, 0.0), o + (2.0, 300.0, 1.0)],
                                  sizes + (200.0, 110.0), 0x155555 + np.arange(len(sizes) + 2), np.arange(len(sizes) + 2) % NLIGHTS)
    particles = np.concatenate([sets.cloud(u, 300, seed=61, nlights=NLIGHTS), sweep, sets.cloud(u, 300, seed=62, nlights=NLIGHTS)])
    boxes, _ = ref.expand(particles, lights)
    tiles, blocks = [], []
    for i in range(300, 300 + sweep.size):
        ys, xs = np.nonzero(boxes_ref.winners(u, boxes[i:i + 1], W, H)[1] >= 0)
        tiles.append(len(set(zip((ys // 8).tolist(), (xs // 8).tolist()))))
        blocks.append(len(set(zip((ys // 64).tolist(), (xs // 64).tolist()))))
    assert min(tiles) <= 1 and any(1 < t <= 16 for t in tiles) and any(t > 16 and b <= 4 for t, b in zip(tiles, blocks))
    assert sum(b > 16 for b in blocks) >= 2 and max(tiles) == 41 * 25         # what covers more than 16 blocks can only be wide
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        before = _fresh_frame(ctx, u)
        want = _restated(before, u, particles, lights, W, H)
        _, idx, _, _ = boxes_ref.winners(u, boxes, W, H)
        drawn = want["depth_f32"] != before["depth_f32"]
        assert len(set(np.unique(idx[drawn]).tolist()) & set(range(300, 300 + sweep.size))) >= 8 and np.count_nonzero((idx >= 0) & ~drawn) > 0
        ctx.draw_particles(u, particles, lights)
        _assert_same(_all(ctx), want, "three kinds of list")


# ---- rt_draw_boxes on the expanded records------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_particles_equal_rt_draw_boxes_on_the_expanded_records(shape, frame_ctx):
    W, H = shape
    ctx, u = frame_ctx[shape], _u()
    particles, _ = cloud_with_twins(u, 300, seed=77, far=150.0)
    lights = sets.some_lights(NLIGHTS)
    boxes, face = ref.expand(particles, lights)
    assert boxes_ref.valid(boxes).all()
    before = _fresh_frame(ctx, u)
    ctx.draw_boxes(u, boxes, face)
    by_boxes = _all(ctx)
    _assert_same(_fresh_frame(ctx, u), before)
    ctx.draw_particles(u, particles, lights)
    _assert_same(_all(ctx), by_boxes, "particles against rt_draw_boxes")
    assert np.count_nonzero(by_boxes["depth_f32"] != before["depth_f32"]) > 50


# ---- async ------------------------------------------------------------------------------------------------------------------------------
def test_async_equals_sync_skips_out_of_domain_records_and_repeats_its_bits(frame_ctx):
    W, H = SHAPES[1]
    ctx, u = frame_ctx[SHAPES[1]], _u()
    n = 200
    particles, _ = cloud_with_twins(u, n, seed=7, far=120.0)
    lights = sets.some_lights(NLIGHTS)
    bad, hidden = particles.copy(), particles.copy()
    behind = np.array(u.origin[:]) - 50.0 * np.array(u.forward[:])
    for i, (field, value) in enumerate([("center", np.nan), ("half", np.nan), ("center", np.inf), ("half", -1.0), ("half", 0.0), ("center", 4194305.0),
                                        ("light", NLIGHTS), ("reserved", 1)]):
        if field == "center":
            bad[field][5 + 11 * i][i % 3] = value
        else:
            bad[field][5 + 11 * i] = value
    skipped = ~ref.valid(bad, NLIGHTS)
    assert np.count_nonzero(skipped) == 8
    hidden["center"][skipped], hidden["half"][skipped], hidden["light"][skipped], hidden["reserved"][skipped] = behind, 1.0, 0, 0
    before = _fresh_frame(ctx, u)
    d_bad, d_lights = _dev(bad), _dev(lights)
    ctx.draw_particles_async(u, d_bad, d_lights)
    got_bad = _all(ctx)
    _assert_same(got_bad, _restated(before, u, bad, lights, W, H), "async, out-of-domain records")
    _assert_same(_fresh_frame(ctx, u), before)
    ctx.draw_particles_async(u, d_bad, d_lights)                          # the identical call on identical planes: identical bits
    _assert_same(_all(ctx), got_bad, "the same call again")
    _assert_same(_fresh_frame(ctx, u), before)
    ctx.draw_particles(u, hidden, lights)
    _assert_same(_all(ctx), got_bad, "sync with hidden cubes in their place")
    assert np.count_nonzero(got_bad["depth_f32"] != before["depth_f32"]) > 50


def test_probes_chain_into_particles_without_a_host_sync(frame_ctx):
    W, H = SHAPES[0]
    ctx, u = frame_ctx[SHAPES[0]], _u()
    n, nl = 400, 12
    particles = sets.cloud(u, n, seed=21, far=100.0, nlights=nl)
    probes = render.make_probes(particles["center"][:nl], np.full(nl, abi.RT_PROBE_SPHERE), np.stack([np.arange(nl) % 16, np.arange(nl) // 16], axis=-1))
    before = _fresh_frame(ctx, u)
    d_probes, d_particles = _dev(probes), _dev(particles)
    d_lights = torch.zeros((nl, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.probe_light_async(u, d_probes, d_lights, 4, 2)
    ctx.draw_particles_async(u, d_particles, d_lights)
    chained = _all(ctx)
    lights = ctx.probe_records(u, probes, 4, 2)
    assert d_lights.cpu().numpy().tobytes() == lights.tobytes() and np.count_nonzero(lights["light"]) > nl
    _assert_same(chained, _restated(before, u, particles, lights, W, H), "chained")
    _assert_same(_fresh_frame(ctx, u), before)
    ctx.draw_particles(u, particles, lights)
    _assert_same(_all(ctx), chained, "sync path")
    assert np.count_nonzero(chained["depth_f32"] != before["depth_f32"]) > 50


# ---- boxes, models and particles together -------------------------------------------------------------------------------------------------
def test_boxes_models_and_particles_composite_by_depth_in_either_order(frame_ctx):
    W, H = SHAPES[1]
    ctx, u = frame_ctx[SHAPES[1]], _u()
    stamps = stamps_t.make_stamps(ctx)
    try:
        models, model_lights = stamps_t.scatter(u, 40, 41, stamps, far=120.0), stamps_t.some_lights(40, seed=1)
        rng = np.random.default_rng(43)
        lo, _ = render.stamp_bounding_boxes(models, stamps_t.extents_of(models, stamps))
        lo = lo + rng.uniform(-1.0, 1.0, lo.shape)                     # boxes that overlap the models
        boxes = render.make_draw_boxes(lo, lo + rng.uniform(0.3, 2.0, lo.shape), rng.integers(0, 1 << 21, 40), 0xFF0000FF)
        box_lights = stamps_t.some_lights(40, seed=2)
        particles = sets.cloud(u, 600, seed=45, far=120.0, nlights=NLIGHTS)
        particles["center"][:40] = (lo + rng.uniform(-0.5, 1.5, lo.shape)).astype(f32)   # ... and particles in among both
        lights = sets.some_lights(NLIGHTS)

        def ref_boxes(p): return _restated_boxes(p, u, boxes, box_lights, W, H)
        def ref_models(p): return _through(stamps_ref.draw_stamps, p, u, models, stamps, model_lights, W, H, None)
        def ref_particles(p): return _restated(p, u, particles, lights, W, H)

        before = _fresh_frame(ctx, u)
        ctx.draw_boxes(u, boxes, box_lights)
        ctx.draw_stamps(u, models, model_lights)
        ctx.draw_particles(u, particles, lights)
        one = _all(ctx)
        _assert_same(one, ref_particles(ref_models(ref_boxes(before))), "boxes, models, particles")
        _assert_same(_fresh_frame(ctx, u), before)
        ctx.draw_particles(u, particles, lights)
        ctx.draw_stamps(u, models, model_lights)
        ctx.draw_boxes(u, boxes, box_lights)
        other = _all(ctx)
        _assert_same(other, ref_boxes(ref_models(ref_particles(before))), "particles, models, boxes")
        for alone in (ref_boxes(before), ref_models(before), ref_particles(before)):
            assert np.count_nonzero(one["depth_f32"] != alone["depth_f32"]) > 20
        assert np.count_nonzero(one["depth_f32"] != other["depth_f32"]) == 0             # the nearer surface wins whichever came first
    finally:
        for s in stamps:
            ctx.stamp_destroy(s)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _code(fn, *a):
    with pytest.raises(render.RtError) as e:
        fn(*a)
    return e.value.code


def test_refusals(procedural_region, blue_noise):
    W, H = 72, 40
    lib = _lib.amd()
    u = _u()
    particles, lights = sets.cloud(u, 8, seed=3, far=60.0, nlights=3), sets.some_lights(3)
    pp, pl = particles.ctypes.data_as(C.c_void_p), lights.ctypes.data_as(C.c_void_p)
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        h = ctx.handle
        d_particles, d_lights = _dev(particles), _dev(lights)
        dp, dl = C.c_void_p(d_particles.data_ptr()), C.c_void_p(d_lights.data_ptr())
        assert _code(ctx.draw_particles, u, particles, lights) == abi.RT_ERR_NOT_READY            # no frame yet
        assert _code(ctx.draw_particles_async, u, d_particles, d_lights) == abi.RT_ERR_NOT_READY
        before = _fresh_frame(ctx, u)
        for call, p, l in ((lib.rt_draw_particles, pp, pl), (lib.rt_draw_particles_async, dp, dl)):
            assert call(h, None, p, 8, l, 3) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), None, 8, l, 3) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), p, 8, None, 3) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), p, 8, l, 0) == abi.RT_ERR_INVALID_ARG                       # particles need a light
            assert call(h, C.byref(u), p, (1 << 20) + 1, l, 3) == abi.RT_ERR_INVALID_ARG           # (refused before anything is read)
            assert call(h, C.byref(u), p, 8, l, (1 << 20) + 1) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), None, 0, None, 0) == abi.RT_OK                              # count == 0 needs no arrays
            assert call(h, C.byref(u), None, 0, l, 3) == abi.RT_OK
        # host memory and unaligned device memory are not what the asynchronous call takes
        assert lib.rt_draw_particles_async(h, C.byref(u), pp, 8, dl, 3) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_draw_particles_async(h, C.byref(u), dp, 8, pl, 3) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_draw_particles_async(h, C.byref(u), C.c_void_p(d_particles.data_ptr() + 4), 7, dl, 3) == abi.RT_ERR_INVALID_ARG
        for field, value in (("center", np.nan), ("center", np.inf), ("half", 0.0), ("half", -1.0), ("half", np.nan), ("light", 3), ("reserved", 1)):
            bad = particles.copy()
            if field == "center":
                bad[field][5][1] = value
            else:
                bad[field][5] = value
            assert _code(ctx.draw_particles, u, bad, lights) == abi.RT_ERR_INVALID_ARG
        vanishing = particles.copy()
        vanishing["center"][2], vanishing["half"][2] = (4194304.0, 0.0, 0.0), 0.1
        assert _code(ctx.draw_particles, u, vanishing, lights) == abi.RT_ERR_INVALID_ARG
        _assert_same(_all(ctx), before, "after the rejected calls")
        ctx.draw_particles(u, particles, lights)                                                  # and the context still works
        _assert_same(_all(ctx), _restated(before, u, particles, lights, W, H))
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2, tile_rank=0, tile_world=2) as tiles:
        tiles.draw_frame(u)
        tiles.sync()
        assert _code(tiles.draw_particles, u, particles, lights) == abi.RT_ERR_UNIMPLEMENTED
        assert lib.rt_draw_particles_async(tiles.handle, C.byref(u), dp, 8, dl, 3) == abi.RT_ERR_UNIMPLEMENTED


# ---- the scratch grows and does not shrink ----------------------------------------------------------------------------------------------
def test_scratch_grows_once_and_serves_smaller_calls(procedural_region, blue_noise):
    W, H = SHAPES[1]
    u = _u()
    lights = sets.some_lights(NLIGHTS)
    big, _ = cloud_with_twins(u, 5000, seed=51)
    small = sets.cloud(u, 10, seed=52, near=10.0, far=40.0, half=(0.3, 0.6), nlights=NLIGHTS)
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        bytes_before = ctx.info().device_bytes
        sizes = []
        for k, particles in enumerate((big, small, big)):
            before = _fresh_frame(ctx, u)
            ctx.draw_particles(u, particles, lights)
            got = _all(ctx)
            _assert_same(got, _restated(before, u, particles, lights, W, H), "call %d" % k)
            assert np.count_nonzero(got["depth_f32"] != before["depth_f32"]) > 5
            sizes.append(ctx.info().device_bytes)
        tx, ty = (W + 7) // 8, (H + 7) // 8
        lists = tx * ty + ((tx + 7) // 8) * ((ty + 7) // 8)
        # (the synchronous call's staging grows with the first call too)
        assert sizes[0] - bytes_before >= 8 + 8 * lists + 72 * 5000 and sizes[1] == sizes[0] and sizes[2] == sizes[0]


# ---- no leak into the next frame ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_flight", [1, 2])
def test_entity_pixels_do_not_leak_into_the_next_frame(in_flight, procedural_region, blue_noise):
    """The persistent route with cached primaries skips the prepass of a frame whose camera and world are unchanged: a slot whose
    planes rt_draw_particles wrote must not be taken for one that still holds its prepass."""
    W, H = 70, 45
    u = _u()
    particles, lights = sets.cloud(u, 400, seed=13, far=120.0, nlights=NLIGHTS), sets.some_lights(NLIGHTS)
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
            ctx.draw_particles(u, particles, lights)
            after = _all(ctx)
            assert np.count_nonzero(after["depth_f32"] != before["depth_f32"]) > 50
            _assert_same(after, _restated(before, u, particles, lights, W, H), "frame %d" % k)
        _assert_same(_fresh_frame(ctx, u), want, "the frame after the particles")


# ---- the lighting history is not touched ------------------------------------------------------------------------------------------------
def test_history_of_a_reprojecting_context_is_untouched(procedural_region, blue_noise):
    W, H = 72, 40
    kw = dict(spp=1, depth=2, flags=ACC | REP | CACHE)
    cams = [_u(seed=10 + k, origin=(-30.0 + 0.25 * k, -128.0, 100.0 - 0.1 * k)) for k in range(5)]
    particles, lights = sets.cloud(cams[0], 400, seed=17, far=120.0, nlights=NLIGHTS), sets.some_lights(NLIGHTS)
    with _ctx(procedural_region, blue_noise, W, H, **kw) as clean, _ctx(procedural_region, blue_noise, W, H, **kw) as ctx:
        for k, u in enumerate(cams):
            want = _fresh_frame(clean, u)
            before = _fresh_frame(ctx, u)
            _assert_same(before, want, "frame %d before its particles" % k)
            ctx.draw_particles(u, particles, lights)
            assert np.array_equal(ctx.read_history(), clean.read_history())
            assert ctx.accumulation() == clean.accumulation()
            after = _all(ctx)
            assert np.count_nonzero(after["depth_f32"] != before["depth_f32"]) > 50
        assert len(np.unique(clean.read_history())) > 1
        _assert_same(after, _restated(before, cams[-1], particles, lights, W, H))
