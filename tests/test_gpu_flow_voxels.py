"""Fluid flow on the GPU (rt_flow_voxels, rt_flow_voxels_async).  Every comparison is bit for bit with tests/flow_voxels_ref.py: the
region's minefield and materials through rt_read_box over the box's chunks and an untouched neighbour, the counts (preloaded with values
that wrap; the reserved words must come back untouched) and the nibble maps (RT_SELFTEST_SCENE_MAPS) after every case.  The named cases of
tests/flow_voxels_sets.py through both calls — the ledge at 1, 3, 14, 15 and 40 ticks and without its source, the room over the chunk
corner (on arbitrary minefield values too), max_level 1 and 13, level_shift 0 and 28, the box the region clips —, more than two tiles on every axis on arbitrary minefield
values at 2 G + 1 ticks, RT_FLOW_TICKS = 1, 2, 4 and 8 on fresh contexts, the extent limit, region 512, single ticks against one call,
two runs of one call, a fixed point, the chain carve -> flow without a host read with a frame and picks on the result, the order against
carves, tile contexts and the other kernels, the accumulation reset and the pending box, every refusal that needs a device and rt_bench
--flood.  That the cases do what their names say is asserted from the restatement in tests/test_flow_voxels_contract.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from raytrace_amd import abi, render
from oracle import pyoracle as po
from tests import adversarial_worlds as aw
from tests import flow_voxels_ref as ref
from tests import flow_voxels_sets as sets
from tests import shape_edits as se
from tests.test_gpu_edit_history import _ctx as _history_ctx
from tests.test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = abi.RT_SELFTEST_SCENE_MAPS
CASES = sets.cases()
COUNTS0 = (0xFFFFFFFF, 7, 0xFFFFFFF0, 3, 0xFFFFFFFE, (0xDEAD, 0xBEEF, 0xF00D))   # what the counters hold before a call: they are added to, and wrap
DEFAULT_G = 4


def _ctx(mats, mine, R=256, W=64, H=40, **kw):
    ctx = render.Context(render.make_config(W, H, region=R, **kw))
    ctx.upload_world(np.asarray(mats).reshape(-1), np.asarray(mine).reshape(-1))
    return ctx


def _reset(ctx, mats, mine):
    ctx.upload_world(np.asarray(mats).reshape(-1), np.asarray(mine).reshape(-1))


def _p(p):
    return abi.RtVoxelFlow.from_buffer_copy(np.asarray(p).tobytes())


def _dev(records):
    records = np.ascontiguousarray(records).reshape(-1)
    t = torch.from_numpy(records.view(np.uint8).reshape(len(records), -1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _host(t, dtype):
    return t.cpu().numpy().view(dtype).reshape(-1)


def _counts0():
    c = np.zeros(1, ref.COUNT_DTYPE)
    c[0] = COUNTS0
    return c


def _hull(p, R):
    """The chunks of the clipped box and one more along x — (origin, extent) in texels."""
    bb = ref.clipped_box(p, R)
    c0, c1 = [int(v) >> 6 for v in bb[0]], [int(v) >> 6 for v in bb[1]]
    k = 0 if c1[0] - c0[0] + 1 < R // 64 else 1                                  # (a box over the region's whole width: along y)
    if c1[k] + 1 < R // 64:
        c1[k] += 1
    else:
        c0[k] -= 1
    return tuple(64 * v for v in c0), tuple(64 * (b - a + 1) for a, b in zip(c0, c1))


def _check_world(ctx, p, want_mats, want_mine, what=""):
    o, e = _hull(p, want_mine.shape[0])
    gm, gf = ctx.read_box(o, e)
    sl = tuple(slice(o[k], o[k] + e[k]) for k in (2, 1, 0))
    assert np.array_equal(gf, want_mine[sl]), what + ": minefield"
    assert np.array_equal(gm, want_mats[sl]), what + ": materials"
    assert ctx.selftest(MAPS) == 0, what


def _flow(ctx, p, call="async", counts=None):
    """One call -> its counts as a COUNT_DTYPE record (the asynchronous call's after sync())."""
    counts = _counts0() if counts is None else np.asarray(counts).reshape(1)
    if call == "async":
        t_c = _dev(counts)
        ctx.flow_voxels_async(_p(p), t_c)
        ctx.sync()
        return _host(t_c, ref.COUNT_DTYPE)[0]
    got = ctx.flow_voxels(_p(p), counts.view(abi.FLOW_COUNT_DTYPE)[0])
    return np.asarray(got).reshape(1).view(ref.COUNT_DTYPE)[0]


def _same_counts(got, want, what=""):
    assert np.asarray(got).tobytes() == np.asarray(want).tobytes(), (what, got, want)


@pytest.fixture(scope="module")
def base(native_built):
    mats, mine = sets.world()
    ctx = _ctx(mats, mine)
    yield mats, mine, ctx
    ctx.destroy()


@pytest.fixture(scope="module")
def arbitrary():
    mats, mine, _, _ = aw.arbitrary_world(256, seed=1)
    return mats, mine


def _case_on(ctx, case, calls=("async", "sync"), what=""):
    mats0, mine0 = sets.case_world(case)
    mats, mine = mats0.copy(), mine0.copy()
    want_c, touched, _ = ref.flow(mats, mine, case["p"], _counts0()[0])
    print(what, "counts", want_c, "touched", touched)
    for call in calls:
        _reset(ctx, mats0, mine0)
        _same_counts(_flow(ctx, case["p"], call), want_c, call)
        _check_world(ctx, case["p"], mats, mine, call)
    return touched


# ---- the named cases through both calls ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_a_case_equals_the_restatement_bit_for_bit(name, base):
    touched = _case_on(base[2], CASES[name], what=name)
    if name == "chunk corner":                                                   # fluid crossed every chunk face: all eight chunks are dirty
        assert len(touched) == 8


def test_without_counts_the_world_changes_alike(base):
    case = CASES["chunk corner"]
    mats0, mine0 = sets.case_world(case)
    mats, mine = mats0.copy(), mine0.copy()
    ref.flow(mats, mine, case["p"])
    for call in ("async", "sync"):
        _reset(base[2], mats0, mine0)
        if call == "async":
            base[2].flow_voxels_async(_p(case["p"]))
        else:
            assert base[2]._lib.rt_flow_voxels(base[2]._h, C.byref(_p(case["p"])), None) == abi.RT_OK
        base[2].sync()
        _check_world(base[2], case["p"], mats, mine, call)


# ---- more than two tiles on every axis, arbitrary minefield values, 2 G + 1 ticks ---------------------------------------------------------------
def test_three_tiles_on_every_axis_on_arbitrary_values(arbitrary):
    mats0, mine0, p = sets.tiles_world(*arbitrary, ticks=2 * DEFAULT_G + 1)
    mats, mine = mats0.copy(), mine0.copy()
    want_c, touched, s = ref.flow(mats, mine, p, _counts0()[0])
    pl = ref.plan(p, 256, DEFAULT_G)
    assert pl["tiles"] == [3, 3, 3] and pl["launches"] == 3 and 2 <= len(touched) <= 8 and int(want_c["active"]) != COUNTS0[3]
    ctx = _ctx(mats0, mine0)
    try:
        _same_counts(_flow(ctx, p), want_c)
        _check_world(ctx, p, mats, mine, "tiles")
        # chunks outside the box keep bytes pack_into would never write; the dirty ones hold its values
        gm, gf = ctx.read_box((0, 64, 0), (192, 128, 128))
        assert np.array_equal(gf, mine[:128, 64:192, :192]) and np.array_equal(gm, mats[:128, 64:192, :192])
        for cx, cy, cz in touched:
            assert gf[64 * cz:64 * cz + 64, 64 * (cy - 1):64 * cy, 64 * cx:64 * cx + 64].max() <= 6
        assert gf[:, :, 128:].max() > 6
    finally:
        ctx.destroy()


def test_the_chunk_corner_on_arbitrary_values_leaves_the_bytes_round_its_chunks(arbitrary):
    """The room over the chunk corner, carved out of a world whose minefield holds values no rebuild would write: the eight chunks of the box
    are dirty and hold pack_into's values, every chunk round them keeps its arbitrary bytes."""
    case = CASES["chunk corner"]
    mats0, mine0 = (a.copy() for a in arbitrary)
    se.apply_shapes(mats0, mine0, se.batch([case["carve"]]))
    sets.place(mats0, mine0, case["voxels"])
    mats, mine = mats0.copy(), mine0.copy()
    want_c, touched, _ = ref.flow(mats, mine, case["p"], _counts0()[0])
    assert len(touched) == 8
    ctx = _ctx(mats0, mine0)
    try:
        _same_counts(_flow(ctx, case["p"]), want_c)
        _check_world(ctx, case["p"], mats, mine, "corner")
        gm, gf = ctx.read_box((0, 0, 0), (192, 192, 192))                            # the 27 chunks round the corner
        assert np.array_equal(gf, mine[:192, :192, :192]) and np.array_equal(gm, mats[:192, :192, :192])
        assert gf[:128, :128, :128].max() <= 6 and np.array_equal(gf[128:], mine0[128:192, :192, :192]) and gf[128:].max() > 6
        assert np.array_equal(gf[:, :, 128:], mine0[:192, :192, 128:192]) and np.array_equal(gf[:, 128:], mine0[:192, 128:192, :192])
    finally:
        ctx.destroy()


def test_every_number_of_ticks_per_launch_gives_equal_bytes(arbitrary, native_built, monkeypatch):
    """RT_FLOW_TICKS is read when a context first plans a flow call, so each value gets a fresh context."""
    mats0, mine0, p = sets.tiles_world(*arbitrary, ticks=9)
    mats, mine = mats0.copy(), mine0.copy()
    want_c, _, _ = ref.flow(mats, mine, p, _counts0()[0])
    for g in sets.GROUPS:
        monkeypatch.setenv("RT_FLOW_TICKS", str(g))
        ctx = _ctx(mats0, mine0)
        try:
            _same_counts(_flow(ctx, p), want_c, g)
            _check_world(ctx, p, mats, mine, "G = %d" % g)
        finally:
            ctx.destroy()


# ---- limits, region 512 ------------------------------------------------------------------------------------------------------------------
def test_an_extent_of_256_is_accepted(base):
    mats0, mine0, ctx = base
    p = ref.params((0, 120, 126), (255, 135, 133), ticks=3, air_material=sets.AIR, fluid_mask=0xFFF00000, fluid_value=0x5A500000)   # random words of the ground pass
    mats, mine = mats0.copy(), mine0.copy()
    want_c, touched, _ = ref.flow(mats, mine, p, _counts0()[0])
    assert int(want_c["changed"]) != COUNTS0[2] and len(touched) >= 2
    _reset(ctx, mats0, mine0)
    _same_counts(_flow(ctx, p), want_c)
    _check_world(ctx, p, mats, mine, "256 x 16 x 8")


def test_region_512_and_the_extent_limit():
    R = 512
    mats, mine, _, _ = aw.arbitrary_world(R, seed=5)
    mats, mine = np.asarray(mats).reshape(R, R, R).copy(), np.asarray(mine).reshape(R, R, R).copy()
    p = ref.params((300, 440, 250), (340, 500, 262), ticks=5, air_material=sets.AIR, fluid_mask=0xF0000000, fluid_value=0x50000000, level_shift=8, max_level=9)
    mats0, mine0 = mats.copy(), mine.copy()
    want_c, touched, _ = ref.flow(mats, mine, p, _counts0()[0])
    assert len(touched) >= 2 and (int(want_c["changed"]) - COUNTS0[2]) & 0xFFFFFFFF > 100
    ctx = _ctx(mats0, mine0, R=R)
    try:
        cnt = _counts0()
        for lo, hi in (((100, 5, 5), (356, 20, 12)), ((0, 0, 0), (256, 15, 7))):     # 257 cells along x
            bad = np.asarray(ref.with_(p, lo=lo, hi=hi)).reshape(1).copy()
            assert ctx._lib.rt_flow_voxels(ctx._h, render._p(bad), render._p(cnt)) == abi.RT_ERR_INVALID_ARG
            assert b"above 256" in ctx._lib.rt_last_error(ctx._h)
        assert cnt.tobytes() == _counts0().tobytes()
        _same_counts(_flow(ctx, p), want_c)
        _check_world(ctx, p, mats, mine, "512")
    finally:
        ctx.destroy()


# ---- determinism, single ticks, fixed points -------------------------------------------------------------------------------------------------
def test_two_runs_of_one_call_give_equal_bits(base):
    case = CASES["chunk corner"]
    mats0, mine0 = sets.case_world(case)
    runs = []
    for _ in range(2):
        _reset(base[2], mats0, mine0)
        got = _flow(base[2], case["p"])
        runs.append(got.tobytes() + b"".join(a.tobytes() for a in base[2].read_box(*_hull(case["p"], 256))))
    assert runs[0] == runs[1]


@pytest.mark.parametrize("name,T", [("random 13 x 11 x 9", 6), ("chunk corner", 7)])
def test_t_calls_of_one_tick_equal_one_call_of_t(name, T, base):
    ctx, case = base[2], CASES[name]
    mats0, mine0 = sets.case_world(case)
    p1, pT = ref.with_(case["p"], ticks=1), ref.with_(case["p"], ticks=T)
    m1, f1, c1 = mats0.copy(), mine0.copy(), _counts0()[0]
    _reset(ctx, mats0, mine0)
    t_c = _dev(_counts0())
    for _ in range(T):
        c1, _, _ = ref.flow(m1, f1, p1, c1)
        ctx.flow_voxels_async(_p(p1), t_c)                                             # T calls enqueued back to back on one count record
    ctx.sync()
    _same_counts(_host(t_c, ref.COUNT_DTYPE)[0], c1, "single ticks")
    _check_world(ctx, p1, m1, f1, "single ticks")
    o, e = _hull(p1, 256)
    steps_m, steps_f = ctx.read_box(o, e)
    mT, fT = mats0.copy(), mine0.copy()
    cT, _, _ = ref.flow(mT, fT, pT, _counts0()[0])
    _reset(ctx, mats0, mine0)
    _same_counts(_flow(ctx, pT), cT, "one call")
    _check_world(ctx, pT, mT, fT, "one call")
    one_m, one_f = ctx.read_box(o, e)
    # the same minefield and the same levels; the word of an unoccupied cell is its own or air_material, and a fluid cell that dried
    # and was wetted again on the way has fluid_word's bits outside the field after the single ticks, its own after the one call
    assert np.array_equal(one_f, steps_f)
    odd = (one_f == 0) & (one_m != steps_m)
    assert ((one_m[odd] ^ steps_m[odd]) & 0xFF00000F == 0).all() and (steps_m[odd] & ~np.uint32(0xF) == sets.WATER).all()


@pytest.mark.parametrize("name", ["ledge", "ledge without its source"])
def test_at_a_fixed_point_nothing_is_active_and_a_second_call_changes_no_byte(name, arbitrary):
    """On arbitrary minefield values: a chunk that was rebuilt without need would show."""
    case = CASES[name]
    mats0, mine0 = (a.copy() for a in arbitrary)
    se.apply_shapes(mats0, mine0, se.batch([se.box(sets.LEDGE_LO, sets.LEDGE_HI, 0x0C0C0C0C, 0)]))
    sets.place(mats0, mine0, case["voxels"])
    mats, mine = mats0.copy(), mine0.copy()
    want_c, _, _ = ref.flow(mats, mine, case["p"], np.zeros(1, ref.COUNT_DTYPE)[0])
    assert int(want_c["active"]) == 0 and int(want_c["chunks"]) == 1
    # the neighbour chunks' arbitrary bytes stand in the hull; a texel of the box's own chunk gets an arbitrary byte back after the call
    ctx = _ctx(mats0, mine0)
    try:
        _same_counts(_flow(ctx, case["p"], counts=np.zeros(1, ref.COUNT_DTYPE)), want_c)
        _check_world(ctx, case["p"], mats, mine, "first")
        again = _flow(ctx, case["p"], counts=np.zeros(1, ref.COUNT_DTYPE))
        assert not np.asarray(again).reshape(1).view(np.uint8).any()                     # active 0, chunks += 0
        _check_world(ctx, case["p"], mats, mine, "second")
    finally:
        ctx.destroy()


# ---- the chain without a host read: carve a dam, flow; a frame and picks on the result -----------------------------------------------------------
DAM_LO, DAM_HI = (96, 64, 128), (135, 95, 137)
POSE = dict(origin=(-12.0, -90.0, 30.0), heading=np.pi / 2, pitch=-0.35, sun=0.3)      # looks at the basin from the south, from above


def _dam():
    """A basin: a wall across x = 110 holds a row of springs on its west side; the carve opens a gap in the wall."""
    voxels = [(110, y, z, sets.FIXED | y) for y in range(64, 96) for z in range(128, 132)]
    voxels += [(106, y, 128, sets.SRC) for y in range(70, 90, 3)]
    carve = se.box((110, 76, 128), (110, 81, 130), 0x0D0D0D0D, 0)
    return sets._case(voxels, ref.params(DAM_LO, DAM_HI, ticks=24, air_material=sets.AIR, **sets.MASK)), carve


def _u(pose, seed=3):
    return po.camera_uniforms(pose["origin"], pose["heading"], pose["pitch"], pose["sun"], seed)


def test_carve_a_dam_then_flow_without_a_host_read_then_a_frame_and_picks(base, blue_noise):
    case, carve = _dam()
    mats0, mine0 = sets.case_world(case)
    mats, mine = mats0.copy(), mine0.copy()
    se.apply_shapes(mats, mine, se.batch([carve]))
    held = mats.copy(), mine.copy()
    want_c, touched, s = ref.flow(mats, mine, case["p"], _counts0()[0])
    assert (s[0, :, 16:] >= 1).any() and (s[0, :, 16:] < ref.SOURCE).all()             # the water is through the gap
    closed = ref.flow(mats0.copy(), mine0.copy(), case["p"])[2]
    assert not (closed[:, :, 15:] % 15 != 0).any()                                      # ... which the wall held before the carve
    W, H, u = 64, 40, _u(POSE)
    cpu, _ = po.render(mats.reshape(-1), mine.reshape(-1), blue_noise, u, W, H, 1, 3)
    old, _ = po.render(held[0].reshape(-1), held[1].reshape(-1), blue_noise, u, W, H, 1, 3)
    assert any(not np.array_equal(old[k], cpu[k]) for k in cpu)                          # the pose does look at what flowed
    ctx = _ctx(mats0, mine0, spp=1, depth=3)
    try:
        ctx.upload_noise(blue_noise)
        ctx.draw_frame(u)                                                                # a frame in flight on the old world
        t_c = _dev(_counts0())
        ctx.edit_shapes(se.batch([carve]))
        ctx.flow_voxels_async(_p(case["p"]), t_c)
        ctx.draw_frame(u)
        xy = np.array([(x, y) for y in range(2, 40, 3) for x in range(2, 64, 3)])
        got = ctx.pick_pixels(u, xy)
        ctx.sync()                                                                       # the first host visit
        _compare(ctx.readback_all(), cpu)
        _same_counts(_host(t_c, ref.COUNT_DTYPE)[0], want_c)
        _check_world(ctx, case["p"], mats, mine, "chain")
    finally:
        ctx.destroy()
    other = _ctx(mats, mine)
    try:
        assert got.tobytes() == other.pick_pixels(u, xy).tobytes()
    finally:
        other.destroy()


# ---- ordering against a carve -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["flow", "carve"])
def test_a_flow_and_a_carve_in_both_orders(base, first):
    ctx = base[2]
    case, carve = _dam()
    p = ref.with_(case["p"], ticks=12)
    mats0, mine0 = sets.case_world(case)
    mats, mine = mats0.copy(), mine0.copy()
    if first == "flow":
        want_c, _, _ = ref.flow(mats, mine, p, _counts0()[0])
        se.apply_shapes(mats, mine, se.batch([carve]))
    else:
        se.apply_shapes(mats, mine, se.batch([carve]))
        want_c, _, _ = ref.flow(mats, mine, p, _counts0()[0])
    _reset(ctx, mats0, mine0)
    t_c = _dev(_counts0())
    if first == "carve":
        ctx.edit_shapes(se.batch([carve]))
    ctx.flow_voxels_async(_p(p), t_c)
    if first == "flow":
        ctx.edit_shapes(se.batch([carve]))
    ctx.sync()
    _same_counts(_host(t_c, ref.COUNT_DTYPE)[0], want_c)
    _check_world(ctx, p, mats, mine, first)


# ---- tile contexts and every RtKernel answer the same --------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(tile_rank=1, tile_world=2), dict(kernel=abi.RT_KERNEL_PATHS), dict(kernel=abi.RT_KERNEL_WAVEFRONT)],
                         ids=["tile 1 of 2", "paths", "wavefront"])
def test_tile_contexts_and_other_kernels_answer_the_same(kw, native_built):
    case = CASES["chunk corner"]
    mats0, mine0 = sets.case_world(case)
    ctx = _ctx(mats0, mine0, **kw)
    try:
        _case_on(ctx, case, ("async",))
    finally:
        ctx.destroy()


# ---- side effects ------------------------------------------------------------------------------------------------------------------
def test_a_call_with_a_box_restarts_the_accumulation_whether_or_not_anything_changes(base, blue_noise):
    mats0, mine0, _ = base
    p = ref.params(sets.LEDGE_LO, sets.LEDGE_HI, ticks=2, air_material=sets.AIR, **sets.MASK)   # air above the floor: nothing to change
    beyond = ref.params((300, 10, 10), (310, 20, 20), **sets.MASK)
    u = [_u(POSE, seed) for seed in range(11, 16)]
    ctx = _ctx(mats0, mine0, spp=1, depth=2, flags=abi.RT_FLAG_CACHE_PRIMARY | abi.RT_FLAG_ACCUMULATE)
    try:
        ctx.upload_noise(blue_noise)
        ctx.draw_frame(u[0])
        ctx.draw_frame(u[1])
        assert ctx.accumulation() == (2, 2)
        ctx.flow_voxels_async(_p(beyond))                                                # an empty clipped box: nothing is reset
        ctx.draw_frame(u[2])
        assert ctx.accumulation() == (3, 3)
        bytes_before = ctx.info().device_bytes
        ctx.flow_voxels_async(_p(p))                                                     # nothing changes; the host cannot know
        ctx.draw_frame(u[3])
        assert ctx.accumulation() == (1, 1)
        # the scratch is the context's: the head and two state arrays of 12 x 3 x 6 cells, counted in device_bytes
        grown = ctx.info().device_bytes - bytes_before
        assert 4 * 512 + 2 * 12 * 3 * 6 <= grown <= 4 * 512 + 2 * 12 * 3 * 6 + (1 << 20)
        assert not np.asarray(ctx.flow_voxels(_p(p))).reshape(1).view(np.uint8).any()
        ctx.draw_frame(u[4])
        assert ctx.accumulation() == (1, 1)
        gm, gf = ctx.read_box((0, 0, 64), (192, 128, 128))
        assert np.array_equal(gf, mine0[64:192, :128, :192]) and np.array_equal(gm, mats0[64:192, :128, :192])
        assert ctx.selftest(MAPS) == 0
    finally:
        ctx.destroy()


def test_a_kept_history_takes_one_pending_box_per_call(procedural_region, blue_noise):
    with _history_ctx(procedural_region, blue_noise) as ctx:
        assert ctx.edit_boxes_pending() == (0, False)
        ctx.flow_voxels_async(_p(ref.params((300, 10, 10), (310, 20, 20), **sets.MASK)))
        assert ctx.edit_boxes_pending() == (0, False)
        ctx.flow_voxels_async(_p(ref.params((60, 60, 100), (70, 70, 140), **sets.MASK)))
        assert ctx.edit_boxes_pending() == (1, False)
        ctx.flow_voxels(_p(ref.params((-5, 60, 100), (3, 70, 140), ticks=3, **sets.MASK)))
        assert ctx.edit_boxes_pending() == (2, False)
        ctx.sync()
        assert ctx.selftest(MAPS) == 0


# ---- refusals that need a device ---------------------------------------------------------------------------------------------------
def _rc(ctx, fn, p, counts):
    return getattr(ctx._lib, fn)(ctx._h, p, counts)


def test_refusals_and_what_they_leave(base):
    ctx, case = base[2], CASES["ledge"]
    mats0, mine0 = sets.case_world(case)
    cnt = _counts0()
    t_c, h_c = _dev(cnt), cnt.copy()
    good = np.asarray(case["p"]).reshape(1).copy()
    P, K, HK = render._p(good), render._dp(t_c), render._p(h_c)
    INVALID, NOT_READY = abi.RT_ERR_INVALID_ARG, abi.RT_ERR_NOT_READY
    with render.Context(render.make_config(64, 40)) as fresh:                 # no world yet
        assert _rc(fresh, "rt_flow_voxels", P, HK) == NOT_READY
        assert _rc(fresh, "rt_flow_voxels_async", P, K) == NOT_READY
        assert _rc(fresh, "rt_flow_voxels_async", None, K) == INVALID
    _reset(ctx, mats0, mine0)
    table, expected, names = sets.params_table()
    for fn, k in (("rt_flow_voxels_async", K), ("rt_flow_voxels", HK)):
        assert _rc(ctx, fn, None, k) == INVALID
        assert _rc(ctx, fn, None, None) == INVALID
        for row, ok, name in zip(table, expected, names):
            if not ok:
                assert _rc(ctx, fn, render._p(np.asarray(row).reshape(1).copy()), k) == INVALID, name
        for name in ("box beyond the region", "box below the region"):
            empty = np.asarray(table[names.index(name)]).reshape(1).copy()
            assert _rc(ctx, fn, render._p(empty), k) == abi.RT_OK                     # an empty clipped box: nothing enqueued
    # the asynchronous call refuses host memory and a misaligned pointer, with an empty clipped box too
    assert _rc(ctx, "rt_flow_voxels_async", P, HK) == INVALID
    assert _rc(ctx, "rt_flow_voxels_async", P, C.c_void_p(t_c.data_ptr() + 8)) == INVALID
    assert b"16-byte aligned" in ctx._lib.rt_last_error(ctx._h)
    empty = np.asarray(table[names.index("box beyond the region")]).reshape(1).copy()
    assert _rc(ctx, "rt_flow_voxels_async", render._p(empty), HK) == INVALID
    ctx.sync()
    # a rejected call changes nothing
    assert t_c.cpu().numpy().tobytes() == cnt.tobytes() and h_c.tobytes() == cnt.tobytes()
    _check_world(ctx, case["p"], mats0, mine0, "after the refusals")
    with pytest.raises(ValueError):
        ctx.flow_voxels_async(_p(case["p"]), torch.zeros(32, dtype=torch.uint8))       # a host tensor
    with pytest.raises(ValueError):
        ctx.flow_voxels_async(_p(case["p"]), torch.zeros(16, dtype=torch.uint8, device="cuda"))


# ---- rt_bench --flood EXTENT [--ticks K] ---------------------------------------------------------------------------------------------------
def test_rt_bench_floods_a_box_and_its_host_path_leaves_the_same_bytes(native_built):
    """The mode exits non-zero unless the host path it times leaves the box bytes the device's calls leave."""
    import json
    import subprocess
    exe = os.path.join(ROOT, "raytrace_amd", "rt_bench")
    r = subprocess.run([exe, "--width", "64", "--height", "64", "--flood", "32"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["flood"] == 32 and j["ticks"] == 8 and j["box"] == [32, 32, 32] and 2 <= j["calls"] <= 64 and j["at_rest"] == 1
    assert j["wetted"] > 32 and j["changed"] >= j["wetted"] and j["chunks"] > 0 and j["host_records"] >= j["wetted"]
    assert j["flow_device_ms"] > 0 and j["host_path_ms"] > 0
    bad = subprocess.run([exe, "--ticks", "2"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--flood" in bad.stderr
