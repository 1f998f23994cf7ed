"""Temporal reprojection (RT_FLAG_REPROJECT) on the GPU, away from the one shape and the one gentle path of
tests/test_gpu_reprojection.py: the sequences of tests/temporal_ref.py (hits behind and beside the previous camera, some of which only the
in-front test rejects; rolled, zoomed and non-unit camera bases; a 0/0 projection; caps 1, 3 and 65535 with counts below, at and above
the cap; analytic scenes with faces one voxel apart, the arbitrary minefield
and the pyramid world; frames of one pixel, of less than a tile and with partial tiles on both axes) and one frame of more pixels than
one trip of the pass's grid covers.  Every frame is compared as there: the two lighting planes and rt_read_history bit for bit with
the restatement, the other seven planes with the oracle's frame, rt_get_accumulation with the restatement's pair.
tests/test_reprojection_contract.py states on the CPU what each sequence exercises."""
import numpy as np
import pytest

from raytrace_amd import abi, render
from oracle import pyoracle as po
from tests import temporal_ref as tr

pytestmark = pytest.mark.gpu

ACC, REP, CACHE = abi.RT_FLAG_ACCUMULATE, abi.RT_FLAG_REPROJECT, abi.RT_FLAG_CACHE_PRIMARY
FLAGS = ACC | REP | CACHE


def _ctx(scene, noise, width, height, cap, kernel=abi.RT_KERNEL_DEFAULT, flags=FLAGS):
    ctx = render.Context(render.make_config(width, height, spp=1, depth=tr.SEQ_DEPTH, kernel=kernel, flags=flags, history_cap=cap))
    ctx.upload_world(*scene)
    ctx.upload_noise(noise)
    return ctx


def _same(got, want, what):
    for name in want:
        assert np.array_equal(got[name], want[name], equal_nan=True), "%s: plane %s differs at %d values" % (
            what, name, int(np.count_nonzero(got[name] != want[name])))


def _check(ctx, u, e, what):
    """One frame against its expected record (see temporal_ref.sequence_expected)."""
    ctx.draw_frame(u)
    assert ctx.accumulation() == e["accumulation"], what
    got = ctx.readback_all()
    hist = ctx.read_history()
    assert np.array_equal(hist, e["counts"]), "%s: %d counts differ" % (what, int(np.count_nonzero(hist != e["counts"])))
    _same(got, e["planes"], what)


def _walk(name, noise, kernel=abi.RT_KERNEL_DEFAULT, flags=FLAGS):
    q = tr.sequences()[name]
    expected = tr.sequence_expected(name, noise)
    with _ctx(tr.sequence_world(q.world), noise, q.width, q.height, q.cap, kernel, flags) as ctx:
        assert (ctx.read_history() == 0).all() and ctx.accumulation() == (0, 0)
        for k, (u, e) in enumerate(zip(q.uniforms, expected)):
            _check(ctx, u, e, "%s frame %d (%s)" % (name, k, e["mode"]))


@pytest.mark.parametrize("name", tr.SEQUENCE_NAMES)
def test_every_frame_of_a_sequence(native_built, blue_noise, name):
    _walk(name, blue_noise)


@pytest.mark.parametrize("name", ["turn", "lens"])
def test_the_path_kernel_without_cached_primaries(native_built, blue_noise, name):
    _walk(name, blue_noise, abi.RT_KERNEL_PATHS, ACC | REP)


@pytest.mark.parametrize("name", ["turn", "lens"])
def test_two_frames_in_flight(native_built, blue_noise, name):
    """Every frame enqueued without a wait into two frame slots: the last frame's planes and counts are those of the chain."""
    q = tr.sequences()[name]
    e = tr.sequence_expected(name, blue_noise)[-1]
    with _ctx(tr.sequence_world(q.world), blue_noise, q.width, q.height, q.cap, flags=FLAGS | abi.RT_FLAG_FRAMES_IN_FLIGHT_2) as ctx:
        assert ctx.info().frames_in_flight == 2
        for u in q.uniforms:
            ctx.draw_frame(u)
        ctx.sync()
        assert ctx.accumulation() == e["accumulation"]
        last, hist = ctx.readback_all(), ctx.read_history()
    assert np.array_equal(hist, e["counts"])
    _same(last, e["planes"], "last frame")


# ---- a frame the grid does not cover in one trip -----------------------------------------------------------------------------------
BIG_W, BIG_H = 1028, 1021          # 1,049,588 pixels: 1,012 more than 4096 blocks of 256 lanes; partial tiles on both axes
ONE_TRIP = 4096 * 256
BIG_STEPS = (0, 1, 1, 2)           # restart, moved, still, moved: all three instantiations of the pass


@pytest.fixture(scope="module")
def big_frames(procedural_region, blue_noise):
    """The expected records of the four large frames, computed once for both kernels.  The second trip's pixels are the top row.
    At the paths' usual pitch they are sky, whose light is the same in every sample: a pass that skipped them would leave planes
    that still compare equal.  At pitch -0.8 they are terrain whose light changes from seed to seed; that is asserted here."""
    assert BIG_W * BIG_H - ONE_TRIP == 1012
    mats, mine = procedural_region
    h = tr.History(BIG_W, BIG_H)
    us = [tr.path_uniforms(k, step=s, pitch=-0.8) for k, s in enumerate(BIG_STEPS)]
    out, first = [], []
    for u in us:
        planes = po.render(mats, mine, blue_noise, u, BIG_W, BIG_H, 1, tr.SEQ_DEPTH)[0]
        first.append(planes["lighting_f32"].reshape(-1, 4)[ONE_TRIP:])
        tail_hit = planes["normal_r8"].reshape(-1)[ONE_TRIP:] < 6
        want = dict(planes)
        want["lighting_f32"], want["lighting_rgba16"], counts, acc = h.step(planes, u)
        out.append(dict(planes=want, counts=counts, accumulation=(h.frames, h.samples), mode=h.mode,
                        tail_accepted=int(acc.reshape(-1)[ONE_TRIP:].sum())))
        assert tail_hit.sum() >= 0.9 * 1012
    changed = int((first[0] != first[1]).any(axis=1).sum())
    print("tail: %d of 1012 pixels change their light between the first two frames; accepted in the tail %s" % (
        changed, [e["tail_accepted"] for e in out]))
    assert changed >= 0.8 * 1012
    assert [e["mode"] for e in out] == ["restart", "moved", "still", "moved"]
    # the moved frames take both branches inside the tail as well
    assert all(0 < e["tail_accepted"] < 1012 for e in out if e["mode"] == "moved")
    return us, out


@pytest.mark.parametrize("kernel", [abi.RT_KERNEL_DEFAULT, abi.RT_KERNEL_PATHS])
def test_a_frame_of_more_pixels_than_one_trip_of_the_grid(procedural_region, blue_noise, big_frames, kernel):
    us, expected = big_frames
    with _ctx(procedural_region, blue_noise, BIG_W, BIG_H, 0, kernel) as ctx:
        for k, (u, e) in enumerate(zip(us, expected)):
            _check(ctx, u, e, "frame %d (%s)" % (k, e["mode"]))
