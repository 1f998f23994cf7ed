"""RtConfig.edit_radius on the GPU: the lighting history kept across rt_edit_voxels and restarted only near an edit or in its sun
shadow.  Every frame is compared with tests/edit_history_ref.py fed with the oracle's one-sample frames of the EDITED world: the two
lighting planes and the per-pixel counts (rt_read_history) bit for bit, the other seven planes against the oracle's own frame;
rt_get_accumulation and rt_edit_boxes_pending against the restatement's host state.  tests/test_edit_history_contract.py shows on the
CPU that the sequences walked here take every branch of the test."""
import ctypes as C

import numpy as np
import pytest

from raytrace_amd import abi, render
from tests import edit_history_ref as er
from tests import temporal_ref as tr
from tests.test_gpu_accumulation import _peek

pytestmark = pytest.mark.gpu

ACC, REP, CACHE = abi.RT_FLAG_ACCUMULATE, abi.RT_FLAG_REPROJECT, abi.RT_FLAG_CACHE_PRIMARY
FLAGS = ACC | REP | CACHE


def _ctx(scene, noise, width=er.SW, height=er.SH, kernel=abi.RT_KERNEL_DEFAULT, flags=FLAGS, radius=er.RADIUS, **kw):
    ctx = render.Context(render.make_config(width, height, spp=1, depth=er.DEPTH, kernel=kernel, flags=flags, edit_radius=radius, **kw))
    ctx.upload_world(*scene)
    ctx.upload_noise(noise)
    return ctx


def _same(got, want, what):
    for name in want:
        assert np.array_equal(got[name], want[name], equal_nan=True), "%s: plane %s differs at %d values" % (
            what, name, int(np.count_nonzero(got[name] != want[name])))


def _edit(ctx, walk, op):
    ctx.edit_voxels(*op[1:])
    walk.edit(*op[1:])
    assert ctx.edit_boxes_pending() == walk.h.pending()


def _frame(ctx, walk, u, what):
    ctx.draw_frame(u)
    assert ctx.edit_boxes_pending() == (0, False), what          # the frame consumed them
    want, counts = walk.frame(u)
    assert ctx.accumulation() == (walk.h.frames, walk.h.samples), what
    got = ctx.readback_all()
    hist = ctx.read_history()
    assert np.array_equal(hist, counts), "%s (%s): %d counts differ" % (what, walk.h.mode, int(np.count_nonzero(hist != counts)))
    _same(got, want, "%s (%s)" % (what, walk.h.mode))


def _walk(ctx, walk, ops):
    """Every op on the context and on the restatement, every frame compared; returns the modes of the frames."""
    modes, k = [], 0
    for op in ops:
        if op[0] == "edit":
            _edit(ctx, walk, op)
        else:
            _frame(ctx, walk, op[1], "frame %d" % k)
            modes.append(walk.h.mode)
            k += 1
    return modes


MAIN_MODES = ["restart", "moved", "moved", "moved", "moved_boxes", "moved", "moved", "still"]
KERNEL_FLAGS = [(k, f) for k in (abi.RT_KERNEL_DEFAULT, abi.RT_KERNEL_FRAME, abi.RT_KERNEL_PATHS, abi.RT_KERNEL_PERSISTENT)
                for f in (FLAGS, ACC | REP)]


@pytest.mark.parametrize("kernel,flags", KERNEL_FLAGS)
def test_path_edit_three_moved_frames_and_a_still_one(procedural_region, blue_noise, kernel, flags):
    walk = er.Walk(procedural_region, blue_noise, er.W, er.H, er.RADIUS)
    with _ctx(procedural_region, blue_noise, er.W, er.H, kernel, flags) as ctx:
        assert ctx.edit_boxes_pending() == (0, False)
        assert _walk(ctx, walk, er.main_ops()) == MAIN_MODES
        assert ctx.accumulation() == (8, 8)


def test_a_still_camera_with_an_edit(procedural_region, blue_noise):
    """The moved pass against the same camera: every live uniform is bitwise equal to the previous frame's."""
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, er.RADIUS)
    with _ctx(procedural_region, blue_noise) as ctx:
        assert _walk(ctx, walk, er.still_ops()) == ["restart", "still", "still", "moved_boxes", "still"]
        assert ctx.accumulation() == (5, 5)


def test_a_cap_below_the_history_under_a_still_camera(procedural_region, blue_noise):
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, er.RADIUS, cap=2)
    with _ctx(procedural_region, blue_noise, history_cap=2) as ctx:
        _walk(ctx, walk, er.still_ops())
        assert ctx.accumulation() == (5, 4)


def test_two_edit_calls_before_one_frame(procedural_region, blue_noise):
    """The second call's block straddles the chunk boundary at x = 128: two boxes of one call, three in all."""
    ops = er.main_ops()
    ops.insert(5, er.block(126, 128, 142, 4, 3, 3))
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, er.RADIUS)
    with _ctx(procedural_region, blue_noise) as ctx:
        assert _walk(ctx, walk, ops) == MAIN_MODES
    assert len(walk.h.frame_boxes) == 0


def test_three_boxes_are_pending_after_those_two_calls(procedural_region, blue_noise):
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, er.RADIUS)
    with _ctx(procedural_region, blue_noise) as ctx:
        _edit(ctx, walk, er.block(*er.PILLAR))
        assert ctx.edit_boxes_pending() == (1, False)
        _edit(ctx, walk, er.block(126, 128, 142, 4, 3, 3))
        assert ctx.edit_boxes_pending() == (3, False)
        ctx.edit_records(np.zeros(0, dtype=[("x", "<u2"), ("y", "<u2"), ("z", "<u2"), ("solid", "<u2"), ("material", "<u4"), ("reserved", "<u4")]))
        assert ctx.edit_boxes_pending() == (3, False)
        # the first frame of a context restarts whatever waits, and consumes it
        _frame(ctx, walk, er.pose(0), "first frame")
        assert walk.h.mode == "restart"


def test_sixteen_boxes(procedural_region, blue_noise):
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, er.RADIUS)
    with _ctx(procedural_region, blue_noise) as ctx:
        assert _walk(ctx, walk, er.boxes_ops(16)) == ["restart", "moved", "moved_boxes", "moved"]


def test_seventeen_boxes_overflow_and_the_frame_restarts(procedural_region, blue_noise):
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, er.RADIUS)
    ops = er.boxes_ops(17)
    with _ctx(procedural_region, blue_noise) as ctx:
        assert _walk(ctx, walk, ops[:2 + 16]) == ["restart", "moved"]
        assert ctx.edit_boxes_pending() == (16, False)
        _edit(ctx, walk, ops[2 + 16])
        assert ctx.edit_boxes_pending() == (0, True)
        _edit(ctx, walk, er.block(*er.PILLAR))                      # (an overflowed set takes no more)
        assert ctx.edit_boxes_pending() == (0, True)
        assert _walk(ctx, walk, ops[2 + 17:]) == ["restart", "moved"]
        assert ctx.accumulation() == (2, 2)


def test_a_broken_block(procedural_region, blue_noise):
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, er.RADIUS)
    with _ctx(procedural_region, blue_noise) as ctx:
        assert _walk(ctx, walk, er.main_ops(edit=er.block(*er.PIT, solid=0))) == MAIN_MODES


def test_sun_angle_zero(procedural_region, blue_noise):
    """s_y == 0 exactly: that axis of the shadow test is the interval test.  Radius 1, so that the shadow decides pixels."""
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, 1)
    with _ctx(procedural_region, blue_noise, radius=1) as ctx:
        assert _walk(ctx, walk, er.main_ops(sun=0.0)) == MAIN_MODES


@pytest.fixture(scope="module")
def region512(native_built):
    from raytrace_amd import world
    return world.generate_region(world.DEFAULT_SEED, region=512)


def test_region_512_with_a_scrolling_window_and_a_box_on_the_seam(region512, blue_noise):
    walk = er.Walk(region512, blue_noise, er.W, er.H, er.RADIUS, region=512)
    with _ctx(region512, blue_noise, er.W, er.H, region=512) as ctx:
        modes = _walk(ctx, walk, er.seam_ops())
    assert modes[er.SEAM_EDIT_FRAME] == "moved_boxes" and modes.count("moved_boxes") == 1


def test_333_by_77(procedural_region, blue_noise):
    walk = er.Walk(procedural_region, blue_noise, 333, 77, er.RADIUS)
    with _ctx(procedural_region, blue_noise, 333, 77) as ctx:
        assert _walk(ctx, walk, er.main_ops()[:6]) == MAIN_MODES[:5]


@pytest.mark.parametrize("kernel", [abi.RT_KERNEL_DEFAULT, abi.RT_KERNEL_PERSISTENT])
def test_two_frames_in_flight_with_edits_between_them(procedural_region, blue_noise, kernel):
    """Frames and edits enqueued without a wait into two frame slots: the boxes belong to the next frame drawn."""
    ops = er.main_ops()
    ops.insert(7, er.block(*er.PIT, solid=0))       # a second edit, before frame 6
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, er.RADIUS)
    with _ctx(procedural_region, blue_noise, kernel=kernel, flags=FLAGS | abi.RT_FLAG_FRAMES_IN_FLIGHT_2) as ctx:
        assert ctx.info().frames_in_flight == 2
        seen = []
        for op in ops:
            if op[0] == "edit":
                ctx.edit_voxels(*op[1:])
                assert ctx.edit_boxes_pending() == (1, False)
            else:
                ctx.draw_frame(op[1])
                seen.append({b: ctx.device_ptr(b) for b in range(abi.RT_BUF_FINAL_BGRA8)})
        ctx.sync()
        assert seen[6] != seen[7] and ctx.accumulation() == (8, 8)
        last, hist = ctx.readback_all(), ctx.read_history()
        before = _peek(seen[6], er.SW, er.SH)
    res = er.run(walk, ops)
    assert [r["mode"] for r in res] == MAIN_MODES[:6] + ["moved_boxes", "still"]
    _same(before, res[6]["planes"], "other slot")
    _same(last, res[7]["planes"], "last slot")
    assert np.array_equal(hist, res[7]["counts"])


def test_a_caller_stream(procedural_region, blue_noise):
    import torch
    s = torch.cuda.Stream(device=0)
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, er.RADIUS)
    ops = er.main_ops()
    with _ctx(procedural_region, blue_noise) as ctx:
        assert _walk(ctx, walk, ops[:2]) == MAIN_MODES[:2]
        ctx.set_stream(s.cuda_stream)
        assert _walk(ctx, walk, ops[2:7]) == MAIN_MODES[2:6]
        ctx.set_stream(0)
        assert _walk(ctx, walk, ops[7:]) == MAIN_MODES[6:]


def test_an_upload_after_the_edit_wins(procedural_region, blue_noise):
    """rt_upload_slice (here: the edited world's own slab again) restarts the history and drops the boxes."""
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, er.RADIUS)
    ops = er.main_ops()
    with _ctx(procedural_region, blue_noise) as ctx:
        _walk(ctx, walk, ops[:5])
        assert ctx.edit_boxes_pending() == (1, False)
        ctx.upload_slice(2, 128, walk.mats[128:144], walk.mine[128:144])
        walk.h.reset()
        assert ctx.edit_boxes_pending() == (0, False)
        assert _walk(ctx, walk, ops[5:7]) == ["restart", "moved"]
        assert ctx.accumulation() == (2, 2)


@pytest.mark.parametrize("what", ["reset", "upload_noise", "generate_slice", "sun_angle"])
def test_the_other_restarts_drop_the_boxes_too(procedural_region, blue_noise, what):
    from raytrace_amd import world
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, er.RADIUS)
    ops = er.main_ops()
    with _ctx(procedural_region, blue_noise) as ctx:
        _walk(ctx, walk, ops[:5])
        kw = {}
        if what == "reset":
            ctx.reset_accumulation()
        elif what == "upload_noise":
            ctx.upload_noise(blue_noise)
        elif what == "generate_slice":
            # (a slab of the generated world that the pillar does not stand in: the edited world stays what it is)
            ctx.generate_slice(world.DEFAULT_SEED, 2, (-128, -128, 64))
        else:
            kw = dict(sun=0.7)
        if what != "sun_angle":
            walk.h.reset()
            assert ctx.edit_boxes_pending() == (0, False)
        else:
            assert ctx.edit_boxes_pending() == (1, False)
        _frame(ctx, walk, er.pose(4, **kw), "after %s" % what)
        assert walk.h.mode == "restart" and ctx.accumulation() == (1, 1) and (ctx.read_history() == 1).all()
        _frame(ctx, walk, er.pose(5, **kw), "the frame after")
        assert walk.h.mode == "moved"


def test_edit_radius_zero_is_what_it_was(procedural_region, blue_noise):
    """(This test alone passes without the feature.)  An edit restarts the history; nothing is ever pending."""
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, 0)
    with _ctx(procedural_region, blue_noise, radius=0) as ctx:
        modes = _walk(ctx, walk, er.main_ops())
        assert modes == ["restart", "moved", "moved", "moved", "restart", "moved", "moved", "still"]
        assert ctx.accumulation() == (4, 4)


@pytest.mark.parametrize("radius", [65, -1])
def test_an_edit_radius_outside_0_to_64_is_rejected(radius):
    with pytest.raises(render.RtError) as ei:
        render.Context(render.make_config(er.SW, er.SH, flags=FLAGS, edit_radius=radius))
    assert ei.value.code == abi.RT_ERR_INVALID_ARG and "edit_radius" in str(ei.value)


def test_the_largest_radius_restarts_every_hit_in_reach(procedural_region, blue_noise):
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, er.MAX_RADIUS)
    with _ctx(procedural_region, blue_noise, radius=er.MAX_RADIUS) as ctx:
        _walk(ctx, walk, er.main_ops()[:6])
    assert walk.h.mode == "moved_boxes" and walk.h.touch["touched"].sum() > 0.5 * (walk.h.nrm < 6).sum()


def test_without_the_flag_edit_radius_is_ignored(procedural_region, blue_noise):
    """An accumulating context without RT_FLAG_REPROJECT: any value is accepted, the edit restarts the sum, nothing is pending."""
    op = er.block(*er.PILLAR)
    u = [er.pose(k, step=2) for k in range(3)]
    for radius in (4, 999):
        walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, 0)
        with _ctx(procedural_region, blue_noise, flags=ACC | CACHE, radius=radius) as ctx:
            ctx.draw_frame(u[0])
            ctx.draw_frame(u[1])
            assert ctx.accumulation() == (2, 2)
            ctx.edit_voxels(*op[1:])
            walk.edit(*op[1:])
            assert ctx.edit_boxes_pending() == (0, False)
            ctx.draw_frame(u[2])
            assert ctx.accumulation() == (1, 1)
            _same(ctx.readback_all(), walk.render(u[2]), "after the edit")
            lib = ctx._lib
            n = C.c_uint32(7)
            assert lib.rt_edit_boxes_pending(ctx.handle, None, C.byref(n)) == abi.RT_ERR_INVALID_ARG
            assert lib.rt_edit_boxes_pending(None, C.byref(n), C.byref(n)) == abi.RT_ERR_INVALID_ARG
