"""Voxel detachment on the GPU (rt_detach_voxels, rt_detach_voxels_async).  Every comparison is bit for bit with
tests/detach_voxels_ref.py: the result record (added and merged onto starting values that wrap), the region's minefield and materials
through rt_read_box over the box's chunks and an untouched neighbour, the captured stamp through rt_stamp_read, and the nibble maps
(RT_SELFTEST_SCENE_MAPS) after every call.  The named cases of tests/detach_voxels_sets.py run as a query, with CAPTURE, with CARVE and
with both, through both calls; then the pass limit, the empty box, arbitrary minefield values (which show the chunks that were rebuilt
and the ones that were not), the whole region of the terrain after a block of it was cut loose, region 512, two runs of one call, the
paste that undoes a carve, the captured stamp drawn as an entity, a frame and picks on the carved world, the side effects on the
lighting history, tile contexts and the other kernels, and every refusal that needs a device.  That the cases detach what their names
say is asserted from the restatement in tests/test_detach_voxels_contract.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from raytrace_amd import abi, render
from oracle import pyoracle as po
from tests import adversarial_worlds as aw
from tests import detach_voxels_ref as ref
from tests import detach_voxels_sets as sets
from tests import shape_edits as se
from tests.test_gpu_draw_stamps import _all, _assert_same, _restated, some_lights
from tests.test_gpu_edit_history import _ctx as _history_ctx
from tests.test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

MAPS = abi.RT_SELFTEST_SCENE_MAPS
CASES = sets.cases()
# what the result holds before a call: counters that wrap, bounds that some cases widen and some do not, a reserved word nobody writes
RES0 = ref.result0(0xFFFFFFF0, 7, 0xFFFFFFFE, 3, (50, 60, 139), 0xFFFFFFFF, (60, 70, 141), 77)
RUNS = [(0, "async"), (ref.CAPTURE, "sync"), (ref.CARVE | ref.CAPTURE, "async"), (ref.CARVE, "sync")]


def _ctx(mats, mine, R=256, W=64, H=40, **kw):
    ctx = render.Context(render.make_config(W, H, region=R, **kw))
    ctx.upload_world(np.asarray(mats).reshape(-1), np.asarray(mine).reshape(-1))
    return ctx


def _reset(ctx, mats, mine):
    ctx.upload_world(np.asarray(mats).reshape(-1), np.asarray(mine).reshape(-1))


def _p(p):
    return abi.RtVoxelDetach.from_buffer_copy(np.asarray(p).tobytes())


def _dev(records):
    records = np.ascontiguousarray(records).reshape(-1)
    t = torch.from_numpy(records.view(np.uint8).reshape(len(records), -1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _host(t, dtype):
    return t.cpu().numpy().view(dtype).reshape(-1)


def _hull(p, R):
    """The chunks of the clipped box and one more along x — (origin, extent) in texels."""
    bb = ref.clipped_box(p, R)
    c0, c1 = [int(v) >> 6 for v in bb[0]], [int(v) >> 6 for v in bb[1]]
    if c1[0] + 1 < R // 64:
        c1[0] += 1
    else:
        c0[0] -= 1
    return tuple(64 * v for v in c0), tuple(64 * (b - a + 1) for a, b in zip(c0, c1))


def _check_world(ctx, p, want_mats, want_mine, what=""):
    o, e = _hull(p, want_mine.shape[0])
    gm, gf = ctx.read_box(o, e)
    sl = tuple(slice(o[k], o[k] + e[k]) for k in (2, 1, 0))
    assert np.array_equal(gf, want_mine[sl]), what + ": minefield"
    assert np.array_equal(gm, want_mats[sl]), what + ": materials"
    assert ctx.selftest(MAPS) == 0, what


def _detach(ctx, p, call="async", result=None):
    """One call -> (its result as a RESULT_DTYPE record — the asynchronous call's after sync() —, the stamp's id or None)."""
    result = np.asarray(RES0 if result is None else result).reshape(1)
    if call == "async":
        t_r = _dev(result)
        stamp = ctx.detach_voxels_async(_p(p), t_r)
        ctx.sync()
        return _host(t_r, ref.RESULT_DTYPE)[0], stamp
    got, stamp = ctx.detach_voxels(_p(p), result.view(abi.DETACH_RESULT_DTYPE)[0])
    return np.asarray(got).reshape(1).view(ref.RESULT_DTYPE)[0], stamp


def _same_result(got, want, what=""):
    assert np.asarray(got).tobytes() == np.asarray(want).tobytes(), (what, got, want)


def _check_stamp(ctx, stamp, want, what="", keep=False):
    """The stamp through rt_stamp_info and rt_stamp_read, then destroyed."""
    assert stamp and ctx.stamp_info(stamp) == tuple(want[1].shape[::-1]), what
    gm, gs = ctx.stamp_read(stamp)
    assert np.array_equal(gs, want[1]), what + ": stamp states"
    assert np.array_equal(gm, want[0]), what + ": stamp words"
    if not keep:
        ctx.stamp_destroy(stamp)


def _case_on(ctx, case, world=None, runs=RUNS, what=""):
    """The case's call as a query, with CAPTURE, with CARVE and with both (one restatement serves all four: the flags change what is
    written, not what is found).  Returns (result, dirty chunks) of the restatement."""
    mats0, mine0 = world if world is not None else sets.case_world(case)
    keep = int(case["p"]["flags"]) & ref.ANCHOR_MATERIAL
    mats, mine = mats0.copy(), mine0.copy()
    want_r, want_s, dirty = ref.detach(mats, mine, ref.with_(case["p"], flags=keep | ref.CARVE | ref.CAPTURE), RES0)
    print(what, "result", want_r, "dirty", dirty)
    _reset(ctx, mats0, mine0)
    carved = False
    for flags, call in runs:
        if carved:
            _reset(ctx, mats0, mine0)
        p = ref.with_(case["p"], flags=keep | flags)
        got_r, stamp = _detach(ctx, p, call)
        tag = "%s flags %d %s" % (what, flags, call)
        _same_result(got_r, want_r, tag)
        carved = bool(flags & ref.CARVE)
        _check_world(ctx, p, mats if carved else mats0, mine if carved else mine0, tag)
        if flags & ref.CAPTURE:
            _check_stamp(ctx, stamp, want_s, tag)
        else:
            assert stamp is None
    return want_r, dirty


@pytest.fixture(scope="module")
def base(native_built):
    mats, mine = sets.world()
    ctx = _ctx(mats, mine)
    yield mats, mine, ctx
    ctx.destroy()


# ---- the named cases: query, capture, carve and both, through both calls ---------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_a_case_equals_the_restatement_bit_for_bit(name, base):
    _case_on(base[2], CASES[name], what=name)


def test_every_flag_combination_through_both_calls(base):
    runs = [(f, c) for f in (0, ref.CAPTURE, ref.CARVE, ref.CARVE | ref.CAPTURE) for c in ("sync", "async")]
    _case_on(base[2], CASES["straddles three faces"], runs=runs, what="all eight")


def test_without_a_result_the_world_and_the_stamp_are_alike(base):
    ctx, case = base[2], CASES["inside one chunk off the word grid"]
    mats0, mine0 = sets.case_world(case)
    mats, mine = mats0.copy(), mine0.copy()
    _, want_s, _ = ref.detach(mats, mine, case["p"])
    for call in ("async", "sync"):
        _reset(ctx, mats0, mine0)
        if call == "async":
            stamp = ctx.detach_voxels_async(_p(case["p"]))
        else:
            out = C.c_uint32(0)
            assert ctx._lib.rt_detach_voxels(ctx._h, C.byref(_p(case["p"])), None, C.byref(out)) == abi.RT_OK
            stamp = out.value
        ctx.sync()
        _check_world(ctx, case["p"], mats, mine, call)
        _check_stamp(ctx, stamp, want_s, call)
    got, stamp = ctx.detach_voxels(_p(ref.with_(case["p"], flags=0)))                   # from result0(): nothing is left to detach
    assert stamp is None and got.tobytes() == ref.result0(0, 14, 2).tobytes()


def test_two_runs_of_one_call_give_equal_bits(base):
    ctx, case = base[2], CASES["random 40 % over eight chunks"]
    mats0, mine0 = sets.case_world(case)
    runs = []
    for _ in range(2):
        _reset(ctx, mats0, mine0)
        got, stamp = _detach(ctx, case["p"])
        sm, ss = ctx.stamp_read(stamp)
        ctx.stamp_destroy(stamp)
        runs.append(got.tobytes() + sm.tobytes() + ss.tobytes() + b"".join(a.tobytes() for a in ctx.read_box(*_hull(case["p"], 256))))
    assert runs[0] == runs[1]


# ---- the pass limit -------------------------------------------------------------------------------------------------------------------------
def test_a_pass_limit_of_the_pass_count_converges_and_one_fewer_changes_nothing(base):
    ctx, case = base[2], CASES["re-enters a chunk twice"]
    mats0, mine0 = sets.case_world(case)
    n = case["expect"]["passes"]
    assert n >= 4
    for limit in (n, n - 1):
        p = ref.with_(case["p"], max_passes=limit)
        mats, mine = mats0.copy(), mine0.copy()
        want_r, want_s, dirty = ref.detach(mats, mine, p, RES0)
        for call in ("async", "sync"):
            _reset(ctx, mats0, mine0)
            got_r, stamp = _detach(ctx, p, call)
            _same_result(got_r, want_r, "limit %d %s" % (limit, call))
            _check_world(ctx, p, mats, mine, "limit %d %s" % (limit, call))
            _check_stamp(ctx, stamp, want_s, "limit %d %s" % (limit, call))
        if limit == n:
            assert int(want_r["unconverged"]) == int(RES0["unconverged"]) and dirty and want_s[1].any()
        else:   # unconverged: no world byte, no count, no bound, an empty stamp
            assert int(want_r["unconverged"]) == int(RES0["unconverged"]) + 1 and int(want_r["passes"]) == (int(RES0["passes"]) + limit) & 0xFFFFFFFF
            assert all(want_r[k].tolist() == RES0[k].tolist() for k in ("detached", "supported", "chunks", "lo", "hi"))
            assert np.array_equal(mats, mats0) and np.array_equal(mine, mine0) and not want_s[1].any() and not want_s[0].any()


def test_an_empty_clipped_box_enqueues_nothing_and_gives_stamp_zero(base):
    mats0, mine0, ctx = base
    _reset(ctx, mats0, mine0)
    live = ctx.info().device_bytes
    for call in ("async", "sync"):
        got, stamp = _detach(ctx, sets.EMPTY_BOX, call)
        _same_result(got, RES0, call)
        assert stamp == 0
    assert ctx.info().device_bytes == live
    _check_world(ctx, CASES["no anchors"]["p"], mats0, mine0, "empty box")


# ---- arbitrary minefield values: dirty chunks are rebuilt, clean chunks keep bytes pack_into would never write ---------------------------
def test_eight_chunks_on_arbitrary_values_rebuild_the_dirty_chunks_only():
    mats, mine, _, _ = aw.arbitrary_world(256, seed=1)
    mats, mine = np.asarray(mats).reshape(256, 256, 256).copy(), np.asarray(mine).reshape(256, 256, 256).copy()
    # a 40 % fill of 80^3 texels over 2 x 2 x 2 chunks, written straight into the minefield so that every other byte keeps its value;
    # chunk (1, 1, 1)'s corner of the box is emptied, so that one chunk of the box holds nothing to detach
    lo, hi = (24, 24, 24), (103, 103, 103)
    fill = np.random.default_rng(3).random((80, 80, 80)) < 0.4
    fill[40:, 40:, 40:] = False
    box = mine[24:104, 24:104, 24:104]
    box[...] = np.where(fill, 0, np.maximum(box, 1))
    p = ref.params(lo, hi, ref.CARVE | ref.CAPTURE, ref.FACE_LO_X, sets.AIR)
    mats0, mine0 = mats.copy(), mine.copy()
    want_r, want_s, dirty = ref.detach(mats, mine, p, RES0)
    assert 3 <= len(dirty) <= 7 and (1, 1, 1) not in dirty and (int(want_r["detached"]) - int(RES0["detached"])) & 0xFFFFFFFF > 500
    ctx = _ctx(mats0, mine0)
    try:
        got_r, stamp = _detach(ctx, p)
        _same_result(got_r, want_r)
        _check_stamp(ctx, stamp, want_s)
        gm, gf = ctx.read_box((0, 0, 0), (192, 128, 128))
        assert np.array_equal(gf, mine[:128, :128, :192]) and np.array_equal(gm, mats[:128, :128, :192])
        assert ctx.selftest(MAPS) == 0
        for cz in range(2):
            for cy in range(2):
                for cx in range(2):
                    sl = (slice(64 * cz, 64 * cz + 64), slice(64 * cy, 64 * cy + 64), slice(64 * cx, 64 * cx + 64))
                    if (cx, cy, cz) in dirty:
                        assert gf[sl].max() <= 6 and not np.array_equal(gf[sl], mine0[sl])      # pack_into's values
                    else:
                        assert gf[sl].max() > 6 and np.array_equal(gf[sl], mine0[sl])           # the early exit: not a byte rewritten
        # a second call finds nothing to detach and rebuilds no chunk — the clean chunks' arbitrary bytes would show one that was
        again, _ = _detach(ctx, ref.with_(p, flags=ref.CARVE), result=ref.result0())
        assert (int(again["detached"]), int(again["chunks"]), int(again["unconverged"])) == (0, 0, 0)
        gm2, gf2 = ctx.read_box((0, 0, 0), (192, 128, 128))
        assert np.array_equal(gf2, gf) and np.array_equal(gm2, gm) and ctx.selftest(MAPS) == 0
    finally:
        ctx.destroy()


# ---- the whole region of the terrain, and region 512 ------------------------------------------------------------------------------------
def test_the_whole_region_after_a_block_of_the_terrain_was_cut_loose(procedural_region):
    mats, mine = (np.asarray(a).reshape(256, 256, 256) for a in procedural_region)
    mats0, mine0, p = sets.slab_case(mats, mine)
    mats, mine = mats0.copy(), mine0.copy()
    want_r, want_s, dirty = ref.detach(mats, mine, p, RES0)
    assert (int(want_r["detached"]) - int(RES0["detached"])) & 0xFFFFFFFF > 100000 and len(dirty) >= 8 and int(want_r["unconverged"]) == 3
    ctx = _ctx(mats0, mine0)
    try:
        got_r, stamp = _detach(ctx, p)
        _same_result(got_r, want_r)
        _check_stamp(ctx, stamp, want_s)
        gm, gf = ctx.read_box((0, 0, 0), (256, 256, 256))
        assert np.array_equal(gf, mine) and np.array_equal(gm, mats) and ctx.selftest(MAPS) == 0
    finally:
        ctx.destroy()


def test_region_512_with_a_box_across_the_middle_of_the_region():
    R = 512
    mats, mine, _, _ = aw.arbitrary_world(R, seed=5)
    mats, mine = np.asarray(mats).reshape(R, R, R).copy(), np.asarray(mine).reshape(R, R, R).copy()
    lo, hi = (236, 236, 236), (275, 275, 275)                                            # chunks 3..4 on every axis
    fill = np.random.default_rng(4).random((40, 40, 40)) < 0.35
    box = mine[236:276, 236:276, 236:276]
    box[...] = np.where(fill, 0, np.maximum(box, 1))
    mats0, mine0 = mats.copy(), mine.copy()
    p = ref.params(lo, hi, ref.CARVE | ref.CAPTURE, ref.FACE_HI_Y, sets.AIR)
    want_r, want_s, dirty = ref.detach(mats, mine, p, RES0)
    assert len(dirty) >= 4 and (int(want_r["detached"]) - int(RES0["detached"])) & 0xFFFFFFFF > 100 and int(want_r["supported"]) > 1000
    ctx = _ctx(mats0, mine0, R=R)
    try:
        got_r, stamp = _detach(ctx, p)
        _same_result(got_r, want_r)
        _check_stamp(ctx, stamp, want_s)
        _check_world(ctx, p, mats, mine, "512")
    finally:
        ctx.destroy()


# ---- the stamp: pasted back, and drawn as an entity ----------------------------------------------------------------------------------------
def test_pasting_the_captured_stamp_back_restores_every_occupancy_and_word(base):
    ctx, case = base[2], CASES["random 40 % over eight chunks"]
    mats0, mine0 = sets.case_world(case)
    mats, mine = mats0.copy(), mine0.copy()
    ref.detach(mats, mine, case["p"])
    assert not np.array_equal(mine, mine0)
    bb = ref.clipped_box(case["p"], 256)
    _reset(ctx, mats0, mine0)
    stamp = ctx.detach_voxels_async(_p(case["p"]))
    ctx.edit_stamps([render.stamp_place(stamp, tuple(int(v) for v in bb[0]), 0, abi.RT_WHERE_ALL)])     # no host read in between
    ctx.sync()
    _check_world(ctx, case["p"], mats0, mine0, "pasted back")
    ctx.stamp_destroy(stamp)


POSE = dict(origin=(-108.0, -112.0, 18.0), heading=np.pi / 2, pitch=-0.05, sun=0.3)     # looks at the word-grid case's pillar and bar from the south


def _u(pose=POSE, seed=3):
    return po.camera_uniforms(pose["origin"], pose["heading"], pose["pitch"], pose["sun"], seed, (0, 0, 0))


def test_the_captured_stamp_drawn_as_an_entity_equals_the_restatements_stamp_drawn(blue_noise, native_built):
    case = CASES["inside one chunk off the word grid"]
    mats0, mine0 = sets.case_world(case)
    carve = se.box((20, 80, 138), (20, 80, 139), sets.AIR, 0)                            # cuts the pillar: its top joins the floating bar's fate
    mats, mine = mats0.copy(), mine0.copy()
    se.apply_shapes(mats, mine, se.batch([carve]))
    want_r, want_s, _ = ref.detach(mats, mine, case["p"])
    assert int(want_r["detached"]) == 32 + 5
    W, H, u = 100, 60, _u()
    ctx = _ctx(mats0, mine0, W=W, H=H, spp=1, depth=2, flags=abi.RT_FLAG_CACHE_PRIMARY)
    try:
        ctx.upload_noise(blue_noise)
        ctx.edit_shapes(se.batch([carve]))
        stamp = ctx.detach_voxels_async(_p(case["p"]))
        ctx.draw_frame(u)
        ctx.sync()
        before = _all(ctx)
        models = render.make_draw_stamps([stamp], [(-124.5, -70.25, 6.0)], 1.0, 0, 0xFF000003)
        lights = some_lights(1)
        ctx.draw_stamps(u, models, lights)
        got = _all(ctx)
        _assert_same(got, _restated(before, u, models, {stamp: want_s}, lights, W, H), "detached stamp")
        assert np.count_nonzero(got["depth_f32"] != before["depth_f32"]) > 20           # the body is in view
    finally:
        ctx.destroy()


# ---- frames and picks -----------------------------------------------------------------------------------------------------------------------
def test_a_frame_drawn_after_the_carve_shows_the_carved_world(blue_noise, native_built):
    case = CASES["inside one chunk off the word grid"]
    mats0, mine0 = sets.case_world(case)
    mats, mine = mats0.copy(), mine0.copy()
    ref.detach(mats, mine, case["p"])
    W, H, u = 64, 40, _u()
    cpu, _ = po.render(mats.reshape(-1), mine.reshape(-1), blue_noise, u, W, H, 1, 3)
    old, _ = po.render(mats0.reshape(-1), mine0.reshape(-1), blue_noise, u, W, H, 1, 3)
    assert any(not np.array_equal(old[k], cpu[k]) for k in cpu)                          # the pose does look at what left
    ctx = _ctx(mats0, mine0, spp=1, depth=3)
    try:
        ctx.upload_noise(blue_noise)
        ctx.draw_frame(u)                                                                # a frame in flight on the old world
        stamp = ctx.detach_voxels_async(_p(case["p"]))
        ctx.draw_frame(u)
        ctx.sync()
        _compare(ctx.readback_all(), cpu)
        ctx.stamp_destroy(stamp)
    finally:
        ctx.destroy()


def test_picks_on_the_carved_world_equal_picks_on_the_restatements_world(base):
    ctx, case = base[2], CASES["inside one chunk off the word grid"]
    mats0, mine0 = sets.case_world(case)
    mats, mine = mats0.copy(), mine0.copy()
    ref.detach(mats, mine, case["p"])
    u = _u()
    xy = np.array([(x, y) for y in range(1, 40, 2) for x in range(1, 64, 2)])
    _reset(ctx, mats0, mine0)
    before = ctx.pick_pixels(u, xy)
    ctx.detach_voxels_async(_p(ref.with_(case["p"], flags=ref.CARVE)))
    got = ctx.pick_pixels(u, xy)
    other = _ctx(mats, mine)
    try:
        assert got.tobytes() == other.pick_pixels(u, xy).tobytes()
    finally:
        other.destroy()
    assert got.tobytes() != before.tobytes()                                            # a pick landed on the bar before it left


# ---- side effects ------------------------------------------------------------------------------------------------------------------------
def test_a_query_keeps_the_accumulation_and_a_carve_restarts_it_whether_or_not_anything_detaches(base, blue_noise):
    mats0, mine0, _ = base
    box = ref.params(*sets.STUBS_BOX, 0, 63, sets.AIR)                                   # air over the floor: nothing occupied
    u = [_u(seed=s) for s in range(11, 17)]
    ctx = _ctx(mats0, mine0, spp=1, depth=2, flags=abi.RT_FLAG_CACHE_PRIMARY | abi.RT_FLAG_ACCUMULATE)
    try:
        ctx.upload_noise(blue_noise)
        ctx.draw_frame(u[0])
        ctx.draw_frame(u[1])
        assert ctx.accumulation() == (2, 2)
        ctx.detach_voxels_async(_p(sets.EMPTY_BOX))                                      # an empty clipped box: nothing is reset
        ctx.draw_frame(u[2])
        assert ctx.accumulation() == (3, 3)
        bytes_before = ctx.info().device_bytes
        ctx.detach_voxels_async(_p(box))                                                 # a query
        stamp = ctx.detach_voxels_async(_p(ref.with_(box, flags=ref.CAPTURE)))           # ... and a capture: the renderer reads nothing of theirs
        ctx.draw_frame(u[3])
        assert ctx.accumulation() == (4, 4)
        # the scratch is the context's and the stamp's arrays are counted while it lives
        grown = ctx.info().device_bytes - bytes_before
        voxels = 21 * 23 * 27
        assert 3 * 32768 + 5 * voxels <= grown <= 3 * 32768 + 5 * voxels + (1 << 20)
        ctx.stamp_destroy(stamp)
        assert ctx.info().device_bytes - bytes_before == grown - 5 * voxels
        ctx.detach_voxels_async(_p(ref.with_(box, flags=ref.CARVE)))                     # nothing detaches; the host cannot know
        ctx.draw_frame(u[4])
        assert ctx.accumulation() == (1, 1)
        got, _ = ctx.detach_voxels(_p(ref.with_(box, flags=ref.CARVE)))
        assert got.tobytes() == ref.result0(0, 0, 1).tobytes()
        ctx.draw_frame(u[5])
        assert ctx.accumulation() == (1, 1)
        gm, gf = ctx.read_box((64, 64, 128), (64, 64, 64))
        assert np.array_equal(gf, mine0[128:192, 64:128, 64:128]) and np.array_equal(gm, mats0[128:192, 64:128, 64:128])
        assert ctx.selftest(MAPS) == 0
    finally:
        ctx.destroy()


def test_a_kept_history_takes_one_pending_box_per_carve_and_none_per_query(procedural_region, blue_noise):
    with _history_ctx(procedural_region, blue_noise) as ctx:
        assert ctx.edit_boxes_pending() == (0, False)
        ctx.detach_voxels_async(_p(sets.EMPTY_BOX))
        assert ctx.edit_boxes_pending() == (0, False)
        ctx.detach_voxels_async(_p(ref.params((60, 60, 100), (70, 70, 140), 0, ref.FACE_LO_Z)))
        stamp = ctx.detach_voxels_async(_p(ref.params((60, 60, 100), (70, 70, 140), ref.CAPTURE, ref.FACE_LO_Z)))
        assert ctx.edit_boxes_pending() == (0, False)
        ctx.detach_voxels_async(_p(ref.params((60, 60, 100), (70, 70, 140), ref.CARVE, ref.FACE_LO_Z)))
        assert ctx.edit_boxes_pending() == (1, False)
        ctx.detach_voxels(_p(ref.params((-5, 60, 100), (3, 70, 140), ref.CARVE, ref.FACE_LO_Z)))
        assert ctx.edit_boxes_pending() == (2, False)
        ctx.sync()
        ctx.stamp_destroy(stamp)
        assert ctx.selftest(MAPS) == 0


# ---- tile contexts and every RtKernel answer the same --------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(tile_rank=1, tile_world=2), dict(kernel=abi.RT_KERNEL_PATHS), dict(kernel=abi.RT_KERNEL_WAVEFRONT)],
                         ids=["tile 1 of 2", "paths", "wavefront"])
def test_tile_contexts_and_other_kernels_answer_the_same(kw, native_built):
    case = CASES["straddles three faces"]
    mats0, mine0 = sets.case_world(case)
    ctx = _ctx(mats0, mine0, **kw)
    try:
        _case_on(ctx, case, runs=[(ref.CARVE | ref.CAPTURE, "async")])
    finally:
        ctx.destroy()


# ---- refusals that need a device ---------------------------------------------------------------------------------------------------
def _rc(ctx, fn, p, result, stamp):
    return getattr(ctx._lib, fn)(ctx._h, p, result, stamp)


def test_refusals_and_what_they_leave(base):
    ctx, case = base[2], CASES["no anchors"]
    mats0, mine0 = sets.case_world(case)
    res = np.asarray(RES0).reshape(1).copy()
    t_r, h_r = _dev(res), res.copy()
    stamp = np.full(1, 0xABCD, np.uint32)
    good = np.asarray(case["p"]).reshape(1).copy()
    P, K, HK, S = render._p(good), render._dp(t_r), render._p(h_r), render._p(stamp)
    INVALID, NOT_READY = abi.RT_ERR_INVALID_ARG, abi.RT_ERR_NOT_READY
    with render.Context(render.make_config(64, 40)) as fresh:                 # no world yet
        assert _rc(fresh, "rt_detach_voxels", P, HK, S) == NOT_READY
        assert _rc(fresh, "rt_detach_voxels_async", P, K, S) == NOT_READY
        assert _rc(fresh, "rt_detach_voxels_async", None, K, S) == INVALID
    _reset(ctx, mats0, mine0)
    bytes_before = ctx.info().device_bytes
    ids_before = ctx.stamp_capture((0, 0, 0), (1, 1, 1))                      # the id a refused call must not consume
    ctx.stamp_destroy(ids_before)
    table, expected, names = sets.params_table()
    for fn, k in (("rt_detach_voxels_async", K), ("rt_detach_voxels", HK)):
        assert _rc(ctx, fn, None, k, S) == INVALID
        assert _rc(ctx, fn, None, None, None) == INVALID
        assert _rc(ctx, fn, P, k, None) == INVALID                                       # CAPTURE without stamp_out
        for row, ok, name in zip(table, expected, names):
            if not ok:
                assert _rc(ctx, fn, render._p(np.asarray(row).reshape(1).copy()), k, S) == INVALID, name
        assert stamp[0] == 0xABCD
        for name in ("box beyond the region", "box below the region"):
            empty = np.asarray(table[names.index(name)]).reshape(1).copy()
            stamp[0] = 0xABCD
            assert _rc(ctx, fn, render._p(empty), k, S) == abi.RT_OK and stamp[0] == 0   # an empty clipped box: nothing enqueued
        stamp[0] = 0xABCD
    # the asynchronous call refuses host memory and a misaligned pointer, with an empty clipped box too
    assert _rc(ctx, "rt_detach_voxels_async", P, HK, S) == INVALID
    assert _rc(ctx, "rt_detach_voxels_async", P, C.c_void_p(t_r.data_ptr() + 8), S) == INVALID
    assert b"16-byte aligned" in ctx._lib.rt_last_error(ctx._h)
    empty = np.asarray(table[names.index("box beyond the region")]).reshape(1).copy()
    assert _rc(ctx, "rt_detach_voxels_async", render._p(empty), HK, S) == INVALID
    ctx.sync()
    # a rejected call changes nothing and creates no stamp
    assert t_r.cpu().numpy().tobytes() == res.tobytes() and h_r.tobytes() == res.tobytes() and stamp[0] == 0xABCD
    assert ctx.info().device_bytes == bytes_before
    nxt = ctx.stamp_capture((0, 0, 0), (1, 1, 1))
    assert (nxt >> 10) == (ids_before >> 10) + 1                                         # no serial was spent in between
    ctx.stamp_destroy(nxt)
    _check_world(ctx, case["p"], mats0, mine0, "after the refusals")
    with pytest.raises(ValueError):
        ctx.detach_voxels_async(_p(case["p"]), torch.zeros(48, dtype=torch.uint8))      # a host tensor
    with pytest.raises(ValueError):
        ctx.detach_voxels_async(_p(case["p"]), torch.zeros(64, dtype=torch.uint8, device="cuda"))


def test_the_limit_of_live_stamps_refuses_a_capture_and_not_a_query(base):
    mats0, mine0, ctx = base
    _reset(ctx, mats0, mine0)
    ids = [ctx.stamp_capture((0, 0, 0), (1, 1, 1)) for _ in range(1024)]
    try:
        p = CASES["no anchors"]["p"]
        out = C.c_uint32(5)
        assert ctx._lib.rt_detach_voxels(ctx._h, C.byref(_p(p)), None, C.byref(out)) == abi.RT_ERR_INVALID_ARG and out.value == 5
        assert b"1024 stamps" in ctx._lib.rt_last_error(ctx._h)
        got, stamp = ctx.detach_voxels(_p(ref.with_(p, flags=0)))
        assert stamp is None and int(got["unconverged"]) == 0
    finally:
        for s in ids:
            ctx.stamp_destroy(s)
    _check_world(ctx, CASES["no anchors"]["p"], mats0, mine0, "after the stamp limit")


# ---- rt_bench --collapse RADIUS ---------------------------------------------------------------------------------------------------------
def test_rt_bench_cuts_a_block_loose_and_its_host_path_detaches_the_same_voxels(native_built):
    """The mode exits non-zero unless the host path it times detaches the voxels, with the words, that the device's stamp holds."""
    import json
    import os
    import subprocess
    from tests.conftest import ROOT
    exe = os.path.join(ROOT, "raytrace_amd", "rt_bench")
    r = subprocess.run([exe, "--width", "64", "--height", "64", "--collapse", "8"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["collapse"] == 8 and j["detached"] == j["host_detached"] > 100 and j["supported"] > j["detached"] and j["chunks"] >= 1
    assert 1 <= j["passes"] <= 32 and j["detach_device_ms"] > 0 and j["host_path_ms"] > 0
    b = j["bounds"]
    assert all(b[k] <= b[k + 3] for k in range(3)) and b[5] - b[2] >= 7
    bad = subprocess.run([exe, "--collapse", "2"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--collapse" in bad.stderr
