"""Temporal reprojection (RT_FLAG_REPROJECT) on the GPU.  Every frame is compared with tests/temporal_ref.py fed with the oracle's
one-sample frames: the two lighting planes and the per-pixel counts (rt_read_history) bit for bit, the other seven planes against
the oracle's own frame.  tests/test_reprojection_contract.py shows on the CPU that the paths walked here take both branches."""
import ctypes as C

import numpy as np
import pytest

from raytrace_amd import abi, render
from oracle import pyoracle as po
from tests import temporal_ref as tr
from tests.test_gpu_accumulation import _peek

pytestmark = pytest.mark.gpu

W, H, DEPTH = 104, 56, 2          # a partial tile in x
ACC, REP, CACHE = abi.RT_FLAG_ACCUMULATE, abi.RT_FLAG_REPROJECT, abi.RT_FLAG_CACHE_PRIMARY
FLAGS = ACC | REP | CACHE
LIGHTING = ("lighting_f32", "lighting_rgba16")

_oracle_cache = {}


def _oracle(region, noise, u, r=256):
    key = (bytes(u), r, id(region[0]))
    if key not in _oracle_cache:
        _oracle_cache[key] = po.render(region[0], region[1], noise, u, W, H, 1, DEPTH, region=r)[0]
    return _oracle_cache[key]


def _ctx(scene, noise, kernel=abi.RT_KERNEL_DEFAULT, flags=FLAGS, **kw):
    ctx = render.Context(render.make_config(W, H, spp=1, depth=DEPTH, kernel=kernel, flags=flags, **kw))
    ctx.upload_world(*scene)
    ctx.upload_noise(noise)
    return ctx


def _expect(h, region, noise, u, r=256):
    """The frame the contract asks for: the oracle's planes with the lighting planes of the restatement, and the counts."""
    want = dict(_oracle(region, noise, u, r))
    want["lighting_f32"], want["lighting_rgba16"], counts, _ = h.step(want, u)
    return want, counts


def _same(got, want, what):
    for name in want:
        assert np.array_equal(got[name], want[name], equal_nan=True), "%s: plane %s differs at %d values" % (
            what, name, int(np.count_nonzero(got[name] != want[name])))


def _check(ctx, h, region, noise, u, what, r=256):
    ctx.draw_frame(u)
    want, counts = _expect(h, region, noise, u, r)
    assert ctx.accumulation() == (h.frames, h.samples), what
    got = ctx.readback_all()
    hist = ctx.read_history()
    assert np.array_equal(hist, counts), "%s: %d counts differ" % (what, int(np.count_nonzero(hist != counts)))
    _same(got, want, what)


def _path(**kw):
    return [tr.path_uniforms(k, step=s, **kw) for k, s in enumerate(tr.GPU_PATH_STEPS)]


KERNEL_FLAGS = [(k, f) for k in (abi.RT_KERNEL_DEFAULT, abi.RT_KERNEL_FRAME, abi.RT_KERNEL_PATHS, abi.RT_KERNEL_PERSISTENT)
                for f in (FLAGS, ACC | REP)]


@pytest.mark.parametrize("cap", [4, 0])
@pytest.mark.parametrize("kernel,flags", KERNEL_FLAGS)
def test_a_path_with_two_still_frames(procedural_region, blue_noise, kernel, flags, cap):
    h = tr.History(W, H, cap or tr.DEFAULT_CAP)
    with _ctx(procedural_region, blue_noise, kernel, flags, history_cap=cap) as ctx:
        assert (ctx.read_history() == 0).all() and ctx.accumulation() == (0, 0)
        for k, u in enumerate(_path()):
            _check(ctx, h, procedural_region, blue_noise, u, "frame %d" % k)
    assert h.mode == "moved" and h.frames == 12 and h.samples == min(cap or 32, 11) + 1


@pytest.fixture(scope="module")
def region512(native_built):
    from raytrace_amd import world
    return world.generate_region(world.DEFAULT_SEED, region=512)


def test_region_512_with_a_scrolling_window(region512, blue_noise):
    """World coordinates carry over when lr changes: the region is a toroidal window on them."""
    h = tr.History(W, H)
    with _ctx(region512, blue_noise, region=512) as ctx:
        for k, s in enumerate(tr.GPU_PATH_STEPS):
            u = tr.path_uniforms(k, step=s, lr=(k // 2, -(k // 3), 0))
            _check(ctx, h, region512, blue_noise, u, "frame %d" % k, r=512)


def test_a_camera_below_the_region(procedural_region, blue_noise):
    """primary_ray moves the start of such a ray; the hit point is still rebuilt from the uniform origin, as depth_f32 is."""
    h = tr.History(W, H)
    with _ctx(procedural_region, blue_noise) as ctx:
        for k, u in enumerate(_path(base=(-30.0, -200.0, 100.0))):
            _check(ctx, h, procedural_region, blue_noise, u, "frame %d" % k)


RESTARTS = ["upload_world", "upload_slice", "upload_noise", "generate_world", "generate_slice", "edit_voxels", "reset", "sun_angle"]


@pytest.mark.parametrize("moving", [True, False])
@pytest.mark.parametrize("what", RESTARTS)
def test_what_restarts_the_history(procedural_region, blue_noise, what, moving):
    """Each cause leaves the world as it was (the same bytes again), so the oracle's frames stay valid."""
    from raytrace_amd import world
    mats, mine = procedural_region
    h = tr.History(W, H)
    kw = {}
    with _ctx(procedural_region, blue_noise) as ctx:
        for k in range(3):
            _check(ctx, h, procedural_region, blue_noise, tr.path_uniforms(k), "frame %d" % k)
        assert h.frames == 3
        if what == "upload_world":
            ctx.upload_world(mats, mine)
        elif what == "upload_slice":
            ctx.upload_slice(2, 128, mats[128:144], mine[128:144])
        elif what == "upload_noise":
            ctx.upload_noise(blue_noise)
        elif what == "generate_world":
            ctx.generate_world(world.DEFAULT_SEED)
        elif what == "generate_slice":
            ctx.generate_slice(world.DEFAULT_SEED, 2, (-128, -128, 0))
        elif what == "edit_voxels":
            ctx.edit_voxels([(10, 20, 30)], [mats[30, 20, 10]], [mine[30, 20, 10] == 0])
        elif what == "reset":
            ctx.reset_accumulation()
        else:
            kw = dict(sun=0.7)
        if what != "sun_angle":
            h.reset()
        u = tr.path_uniforms(3, step=3 if moving else 2, **kw)
        _check(ctx, h, procedural_region, blue_noise, u, "after %s" % what)
        assert h.mode == "restart" and ctx.accumulation() == (1, 1) and (ctx.read_history() == 1).all()
        # ... and the history goes on from there
        _check(ctx, h, procedural_region, blue_noise, tr.path_uniforms(4, **kw), "second frame after %s" % what)
        assert h.mode == "moved" and ctx.accumulation() == (2, 2)


def test_an_empty_edit_batch_and_the_dead_fields_do_not_restart_it(procedural_region, blue_noise):
    h = tr.History(W, H)
    with _ctx(procedural_region, blue_noise) as ctx:
        for k in range(2):
            _check(ctx, h, procedural_region, blue_noise, tr.path_uniforms(k), "frame %d" % k)
        ctx.edit_records(np.zeros(0, dtype=[("x", "<u2"), ("y", "<u2"), ("z", "<u2"), ("solid", "<u2"), ("material", "<u4"), ("reserved", "<u4")]))
        u = tr.path_uniforms(2)
        u.old_origin[0] = 5.0
        u.old_transform_c1[2] = -1.0
        u.region_offset[1] = 64
        _check(ctx, h, procedural_region, blue_noise, u, "frame 2")
        assert h.mode == "moved" and ctx.accumulation() == (3, 3)


def test_a_context_that_never_moves_equals_plain_accumulation(procedural_region, blue_noise):
    us = [tr.path_uniforms(k, step=0) for k in range(6)]
    with _ctx(procedural_region, blue_noise) as ctx, _ctx(procedural_region, blue_noise, flags=ACC | CACHE) as plain:
        for u in us:
            ctx.draw_frame(u)
            plain.draw_frame(u)
            assert ctx.accumulation() == plain.accumulation()
        got, want = ctx.readback_all(), plain.readback_all()
        assert (ctx.read_history() == 6).all()
    _same(got, want, "after 6 still frames")
    _same(got, po.render(procedural_region[0], procedural_region[1], blue_noise, us[0], W, H, 6, DEPTH)[0], "against the oracle")


@pytest.mark.parametrize("kernel", [abi.RT_KERNEL_DEFAULT, abi.RT_KERNEL_PATHS, abi.RT_KERNEL_PERSISTENT])
def test_two_frames_in_flight_form_one_chain(procedural_region, blue_noise, kernel):
    """Eight frames enqueued without a wait into two frame slots: each pass reads the set the previous frame's pass wrote."""
    h = tr.History(W, H)
    us = _path()[:8]
    with _ctx(procedural_region, blue_noise, kernel, FLAGS | abi.RT_FLAG_FRAMES_IN_FLIGHT_2) as ctx:
        assert ctx.info().frames_in_flight == 2
        seen = []
        for u in us:
            ctx.draw_frame(u)
            seen.append({b: ctx.device_ptr(b) for b in range(abi.RT_BUF_FINAL_BGRA8)})
        ctx.sync()
        assert seen[6] != seen[7]
        last, hist = ctx.readback_all(), ctx.read_history()
        before = _peek(seen[6], W, H)
    for k, u in enumerate(us):
        want, counts = _expect(h, procedural_region, blue_noise, u)
        if k == 6:
            _same(before, want, "other slot")
    _same(last, want, "last slot")
    assert np.array_equal(hist, counts)


def test_caller_stream_part_way(procedural_region, blue_noise):
    import torch
    s = torch.cuda.Stream(device=0)
    h = tr.History(W, H)
    with _ctx(procedural_region, blue_noise) as ctx:
        for k, u in enumerate(_path()):
            if k == 3:
                ctx.set_stream(s.cuda_stream)
            if k == 8:
                ctx.set_stream(0)
            _check(ctx, h, procedural_region, blue_noise, u, "frame %d" % k)


def test_post_passes_between_frames_leave_the_history_alone(procedural_region, blue_noise):
    h = tr.History(W, H)
    us = _path()
    with _ctx(procedural_region, blue_noise) as ctx:
        for u in us[:-1]:
            ctx.draw_frame(u)
            ctx.denoise(True)
            ctx.finalize()
            _expect(h, procedural_region, blue_noise, u)
        _check(ctx, h, procedural_region, blue_noise, us[-1], "last frame")


def test_read_history_errors_and_device_bytes(procedural_region, blue_noise):
    with _ctx(procedural_region, blue_noise) as ctx, _ctx(procedural_region, blue_noise, flags=ACC | CACHE) as plain:
        lib = ctx._lib
        out = np.zeros(W * H + 1, dtype=np.uint32)
        p = out.ctypes.data_as(C.c_void_p)
        assert lib.rt_read_history(ctx.handle, p, W * H * 4) == abi.RT_OK
        for bad in (W * H * 4 - 4, W * H * 4 + 4, 0):
            assert lib.rt_read_history(ctx.handle, p, bad) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_read_history(ctx.handle, None, W * H * 4) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_read_history(plain.handle, p, W * H * 4) == abi.RT_ERR_INVALID_ARG
        assert b"RT_FLAG_REPROJECT" in lib.rt_last_error(plain.handle)
        npix_pad = ((W + 7) // 8) * ((H + 7) // 8) * 64
        assert ctx.info().device_bytes - plain.info().device_bytes == npix_pad * 32


def test_without_the_flag_a_camera_change_restarts_as_before(procedural_region, blue_noise):
    with _ctx(procedural_region, blue_noise, flags=ACC | CACHE, history_cap=-5) as ctx:
        for k in range(3):
            u = tr.path_uniforms(k)
            ctx.draw_frame(u)
            assert ctx.accumulation() == (1, 1)
            _same(ctx.readback_all(), _oracle(procedural_region, blue_noise, u), "frame %d" % k)
        with pytest.raises(render.RtError) as ei:
            ctx.read_history()
        assert ei.value.code == abi.RT_ERR_INVALID_ARG
