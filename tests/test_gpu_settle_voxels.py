"""Voxel settling on the GPU (rt_settle_voxels, rt_settle_voxels_async).  Every comparison is bit for bit with
tests/settle_voxels_ref.py: the region's minefield and materials through rt_read_box over the box's chunks and an untouched
neighbour, the counts (preloaded with values that wrap) and the nibble maps (RT_SELFTEST_SCENE_MAPS) after every case.  The named
cases of tests/settle_voxels_sets.py through both calls, the six axis / direction pairs on one fixture, the eight-chunk box on arbitrary
minefield values (which show the chunks that were rebuilt and the ones that were not, and that a second call rebuilds none), region
512, single steps against one call, two runs of one call, the chain deposit -> carve -> settle without a host read, a frame and a
pick on the settled world, the order against carves, the accumulation reset and the pending box, and every refusal that needs a
device.  That the cases move what their names say is asserted from the restatement in tests/test_settle_voxels_contract.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from raytrace_amd import abi, render
from oracle import pyoracle as po
from tests import adversarial_worlds as aw
from tests import deposit_particles_ref as dref
from tests import deposit_particles_sets as dsets
from tests import settle_voxels_ref as ref
from tests import settle_voxels_sets as sets
from tests import shape_edits as se
from tests.test_gpu_edit_history import _ctx as _history_ctx
from tests.test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

MAPS = abi.RT_SELFTEST_SCENE_MAPS
CASES = sets.cases()
COUNTS0 = (0xFFFFFFFF, 7, 0xFFFFFFF0, 3)                 # what the counters hold before a call: they are added to, and wrap


def _ctx(mats, mine, R=256, W=64, H=40, **kw):
    ctx = render.Context(render.make_config(W, H, region=R, **kw))
    ctx.upload_world(np.asarray(mats).reshape(-1), np.asarray(mine).reshape(-1))
    return ctx


def _reset(ctx, mats, mine):
    ctx.upload_world(np.asarray(mats).reshape(-1), np.asarray(mine).reshape(-1))


def _p(p):
    return abi.RtVoxelSettle.from_buffer_copy(np.asarray(p).tobytes())


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


def _settle(ctx, p, call="async", counts=None):
    """One call -> its counts as a COUNT_DTYPE record (the asynchronous call's after sync())."""
    counts = _counts0() if counts is None else np.asarray(counts).reshape(1)
    if call == "async":
        t_c = _dev(counts)
        ctx.settle_voxels_async(_p(p), t_c)
        ctx.sync()
        return _host(t_c, ref.COUNT_DTYPE)[0]
    got = ctx.settle_voxels(_p(p), counts.view(abi.SETTLE_COUNT_DTYPE)[0])
    return np.asarray(got).reshape(1).view(ref.COUNT_DTYPE)[0]


def _same_counts(got, want, what=""):
    assert np.asarray(got).tobytes() == np.asarray(want).tobytes(), (what, got, want)


@pytest.fixture(scope="module")
def base(native_built):
    mats, mine = sets.world()
    ctx = _ctx(mats, mine)
    yield mats, mine, ctx
    ctx.destroy()


def _case_on(ctx, case, calls=("async", "sync"), what=""):
    mats0, mine0 = sets.case_world(case)
    mats, mine = mats0.copy(), mine0.copy()
    want_c, touched = ref.settle(mats, mine, case["p"], _counts0()[0])
    print(what, "counts", want_c, "touched", touched)
    for call in calls:
        _reset(ctx, mats0, mine0)
        _same_counts(_settle(ctx, case["p"], call), want_c, call)
        _check_world(ctx, case["p"], mats, mine, call)
    return touched


# ---- the named cases through both calls, the fixture along every axis in both directions ------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_a_case_equals_the_restatement_bit_for_bit(name, base):
    _case_on(base[2], CASES[name], what=name)


@pytest.mark.parametrize("axis,toward", sets.AXES)
def test_the_fixture_along_every_axis_in_both_directions(axis, toward, base):
    assert _case_on(base[2], sets.fixture_case(axis, toward), ("async",), "axis %d toward %d" % (axis, toward))


def test_without_counts_the_world_changes_alike(base):
    case = CASES["chunk boundary"]
    mats0, mine0 = sets.case_world(case)
    mats, mine = mats0.copy(), mine0.copy()
    ref.settle(mats, mine, case["p"])
    for call in ("async", "sync"):
        _reset(base[2], mats0, mine0)
        if call == "async":
            base[2].settle_voxels_async(_p(case["p"]))
        else:
            assert base[2]._lib.rt_settle_voxels(base[2]._h, C.byref(_p(case["p"])), None) == abi.RT_OK
        base[2].sync()
        _check_world(base[2], case["p"], mats, mine, call)
    got = base[2].settle_voxels(_p(case["p"]))                                          # counts from zeros: nothing is left to move
    assert got.tolist() == (0, 0, 0, 0)


def test_two_runs_of_one_call_give_equal_bits(base):
    case = CASES["random 64 x 64"]
    mats0, mine0 = sets.case_world(case)
    runs = []
    for _ in range(2):
        _reset(base[2], mats0, mine0)
        got = _settle(base[2], case["p"])
        runs.append(got.tobytes() + b"".join(a.tobytes() for a in base[2].read_box(*_hull(case["p"], 256))))
    assert runs[0] == runs[1]


@pytest.mark.parametrize("name,T", [("random 64 x 64", 3), ("stack unlimited", 6)])
def test_t_calls_with_max_fall_1_equal_one_call_with_max_fall_t(name, T, base):
    ctx, case = base[2], CASES[name]
    mats0, mine0 = sets.case_world(case)
    p1, pT = ref.with_(case["p"], max_fall=1), ref.with_(case["p"], max_fall=T)
    m1, f1, c1 = mats0.copy(), mine0.copy(), _counts0()[0]
    _reset(ctx, mats0, mine0)
    t_c = _dev(_counts0())
    for _ in range(T):
        c1, _ = ref.settle(m1, f1, p1, c1)
        ctx.settle_voxels_async(_p(p1), t_c)                                           # T calls enqueued back to back on one count record
    ctx.sync()
    _same_counts(_host(t_c, ref.COUNT_DTYPE)[0], c1, "single steps")
    _check_world(ctx, p1, m1, f1, "single steps")
    o, e = _hull(p1, 256)
    steps_m, steps_f = ctx.read_box(o, e)
    mT, fT = mats0.copy(), mine0.copy()
    cT, _ = ref.settle(mT, fT, pT, _counts0()[0])
    _reset(ctx, mats0, mine0)
    _same_counts(_settle(ctx, pT), cT, "one call")
    _check_world(ctx, pT, mT, fT, "one call")
    one_m, one_f = ctx.read_box(o, e)
    # the same voxels in the same cells, the same minefield, the same distance; the word of an unoccupied cell is its own or air_material
    assert np.array_equal(one_f, steps_f) and np.array_equal(one_m[one_f == 0], steps_m[one_f == 0])
    assert int(cT["distance"]) == int(c1["distance"])


# ---- eight chunks on arbitrary minefield values: dirty chunks are rebuilt, clean chunks keep bytes pack_into would never write -----------
def test_eight_chunks_on_arbitrary_values_and_a_second_call_that_rebuilds_nothing():
    mats, mine, _, _ = aw.arbitrary_world(256, seed=1)
    mats, p = sets.eight_chunks_world(mats, mine)
    mine = mine.copy()
    mats0, mine0 = mats.copy(), mine.copy()
    want_c, touched = ref.settle(mats, mine, p, _counts0()[0])
    assert 2 <= len(touched) <= 3 and int(want_c["chunks"]) == (COUNTS0[3] + len(touched)) & 0xFFFFFFFF
    ctx = _ctx(mats0, mine0)
    try:
        _same_counts(_settle(ctx, p), want_c)
        gm, gf = ctx.read_box((0, 0, 0), (192, 128, 128))
        assert np.array_equal(gf, mine[:128, :128, :192]) and np.array_equal(gm, mats[:128, :128, :192])
        assert ctx.selftest(MAPS) == 0
        for cz in range(2):
            for cy in range(2):
                for cx in range(2):
                    sl = (slice(64 * cz, 64 * cz + 64), slice(64 * cy, 64 * cy + 64), slice(64 * cx, 64 * cx + 64))
                    if (cx, cy, cz) in touched:
                        assert gf[sl].max() <= 6 and not np.array_equal(gf[sl], mine0[sl])      # pack_into's values
                    else:
                        assert gf[sl].max() > 6 and np.array_equal(gf[sl], mine0[sl])           # the early exit: not a byte rewritten
        # a second unlimited call: nothing moves, no chunk is rebuilt — the clean chunks' arbitrary bytes would show one that was
        again = _settle(ctx, p, counts=np.zeros(1, ref.COUNT_DTYPE))
        assert again.tolist() == (0, 0, 0, 0)
        gm2, gf2 = ctx.read_box((0, 0, 0), (192, 128, 128))
        assert np.array_equal(gf2, gf) and np.array_equal(gm2, gm) and ctx.selftest(MAPS) == 0
    finally:
        ctx.destroy()


def test_a_call_that_moves_nothing_on_arbitrary_values_changes_no_byte():
    mats, mine, _, _ = aw.arbitrary_world(256, seed=1)
    p = ref.params(*sets.EIGHT_BOX, air_material=sets.AIR, loose_mask=0xFFFFFFFF, loose_value=sets.EIGHT_WORD)    # no voxel is loose
    assert not (mats == sets.EIGHT_WORD).any()
    ctx = _ctx(mats, mine)
    try:
        assert _settle(ctx, p, counts=np.zeros(1, ref.COUNT_DTYPE)).tolist() == (0, 0, 0, 0)
        gm, gf = ctx.read_box((0, 0, 0), (192, 128, 128))
        assert np.array_equal(gf, mine[:128, :128, :192]) and np.array_equal(gm, mats[:128, :128, :192]) and ctx.selftest(MAPS) == 0
    finally:
        ctx.destroy()


# ---- region 512 ----------------------------------------------------------------------------------------------------------------------
def test_region_512_every_voxel_loose_two_cells_a_call():
    R = 512
    mats, mine, _, _ = aw.arbitrary_world(R, seed=5)
    mats, mine = np.asarray(mats).reshape(R, R, R).copy(), np.asarray(mine).reshape(R, R, R).copy()
    mats0, mine0 = mats.copy(), mine.copy()
    p = ref.params((300, 440, 250), (340, 500, 262), 2, sets.AIR)                         # chunks x 4..5, y 6..7, z 3..4
    want_c, touched = ref.settle(mats, mine, p, _counts0()[0])
    assert len(touched) >= 2 and (int(want_c["moved"]) - COUNTS0[0]) & 0xFFFFFFFF > 100
    ctx = _ctx(mats0, mine0, R=R)
    try:
        _same_counts(_settle(ctx, p), want_c)
        _check_world(ctx, p, mats, mine, "512")
    finally:
        ctx.destroy()


# ---- the chain without a host read: deposit -> carve under the pile -> settle -------------------------------------------------------------
def test_deposit_carve_and_settle_without_a_host_read(base):
    mats0, mine0, ctx = base
    states = dsets.resting([(-60, -60, 0), (-60, -60, 1), (-59, -60, 0), (-58, -59, 0), (-58, -59, 2)])     # texels 68.., 68.., 128..
    dp = dref.params((64, 64, 126), (72, 72, 135))
    carve = se.box((66, 66, 120), (70, 70, 127), 0x0BADF00D, 0)
    p = ref.params((64, 64, 118), (72, 72, 135), air_material=sets.AIR)
    mats, mine = mats0.copy(), mine0.copy()
    _, _, want_d, _ = dref.deposit(mats, mine, dp, states)
    se.apply_shapes(mats, mine, se.batch([carve]))
    want_c, touched = ref.settle(mats, mine, p, _counts0()[0])
    assert int(want_d["deposited"]) == 5 and (int(want_c["moved"]) - COUNTS0[0]) & 0xFFFFFFFF == 5 and (mine[120:122, 68, 68] == 0).all()
    _reset(ctx, mats0, mine0)
    t_s, t_d, t_c = _dev(states), _dev(np.zeros(1, dref.COUNT_DTYPE)), _dev(_counts0())
    ctx.deposit_particles_async(abi.RtParticleDeposit.from_buffer_copy(dp.tobytes()), t_s, None, t_d)
    ctx.edit_shapes(se.batch([carve]))
    ctx.settle_voxels_async(_p(p), t_c)
    ctx.sync()                                                                           # the first host visit
    assert _host(t_d, dref.COUNT_DTYPE)[0].tobytes() == np.asarray(want_d).tobytes()
    _same_counts(_host(t_c, ref.COUNT_DTYPE)[0], want_c)
    _check_world(ctx, p, mats, mine, "chain")


# ---- frames and picks ------------------------------------------------------------------------------------------------------------------
POSE = dict(origin=(0.0, -120.0, 22.0), heading=np.pi / 2, pitch=-0.1, sun=0.3)       # looks at the random case's block from the south


def _u(pose, seed=3):
    return po.camera_uniforms(pose["origin"], pose["heading"], pose["pitch"], pose["sun"], seed)


def test_a_frame_drawn_after_the_settle_shows_the_settled_world(blue_noise, native_built):
    case = CASES["random 64 x 64"]
    mats0, mine0 = sets.case_world(case)
    mats, mine = mats0.copy(), mine0.copy()
    ref.settle(mats, mine, case["p"])
    W, H, u = 64, 40, _u(POSE)
    cpu, _ = po.render(mats.reshape(-1), mine.reshape(-1), blue_noise, u, W, H, 1, 3)
    old, _ = po.render(mats0.reshape(-1), mine0.reshape(-1), blue_noise, u, W, H, 1, 3)
    assert any(not np.array_equal(old[k], cpu[k]) for k in cpu)                          # the pose does look at what fell
    ctx = _ctx(mats0, mine0, spp=1, depth=3)
    try:
        ctx.upload_noise(blue_noise)
        ctx.draw_frame(u)                                                                # a frame in flight on the old world
        ctx.settle_voxels_async(_p(case["p"]))
        ctx.draw_frame(u)
        ctx.sync()
        _compare(ctx.readback_all(), cpu)
    finally:
        ctx.destroy()


def test_picks_on_the_settled_world_equal_picks_on_the_restatements_world(base):
    ctx, case = base[2], CASES["random 64 x 64"]
    mats0, mine0 = sets.case_world(case)
    mats, mine = mats0.copy(), mine0.copy()
    ref.settle(mats, mine, case["p"])
    u = _u(POSE)
    xy = np.array([(x, y) for y in range(2, 40, 3) for x in range(2, 64, 3)])
    _reset(ctx, mats0, mine0)
    ctx.settle_voxels_async(_p(case["p"]))
    got = ctx.pick_pixels(u, xy)
    other = _ctx(mats, mine)
    try:
        assert got.tobytes() == other.pick_pixels(u, xy).tobytes()
    finally:
        other.destroy()
    on = (got["kind"] == abi.RT_HIT_SOLID) & ((got["material"] & 0xFF000000) == sets.LOOSE) & (got["texel"][:, 2] >= 130)
    assert on.any()                                                                     # a pick lands on a voxel of the pile


# ---- ordering against a carve -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["settle", "carve"])
def test_a_settle_and_a_carve_in_both_orders(base, first):
    ctx, case = base[2], CASES["stack unlimited"]
    p = case["p"]
    carve = se.box((70, 70, 134), (70, 70, 135), 0x77, 0)                                # two of the stack's voxels before, two others after
    mats0, mine0 = sets.case_world(case)
    mats, mine = mats0.copy(), mine0.copy()
    if first == "settle":
        want_c, _ = ref.settle(mats, mine, p, _counts0()[0])
        se.apply_shapes(mats, mine, se.batch([carve]))
        assert np.nonzero(mine[132:146, 70, 70] == 0)[0].tolist() == [0, 1, 4]
    else:
        se.apply_shapes(mats, mine, se.batch([carve]))
        want_c, _ = ref.settle(mats, mine, p, _counts0()[0])
        assert np.nonzero(mine[132:146, 70, 70] == 0)[0].tolist() == [0, 1, 2]
    _reset(ctx, mats0, mine0)
    t_c = _dev(_counts0())
    if first == "carve":
        ctx.edit_shapes(se.batch([carve]))
    ctx.settle_voxels_async(_p(p), t_c)
    if first == "settle":
        ctx.edit_shapes(se.batch([carve]))
    ctx.sync()
    _same_counts(_host(t_c, ref.COUNT_DTYPE)[0], want_c)
    _check_world(ctx, p, mats, mine, first)


# ---- tile contexts and every RtKernel answer the same --------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(tile_rank=1, tile_world=2), dict(kernel=abi.RT_KERNEL_PATHS), dict(kernel=abi.RT_KERNEL_WAVEFRONT)],
                         ids=["tile 1 of 2", "paths", "wavefront"])
def test_tile_contexts_and_other_kernels_answer_the_same(kw, native_built):
    case = CASES["chunk boundary"]
    mats0, mine0 = sets.case_world(case)
    ctx = _ctx(mats0, mine0, **kw)
    try:
        _case_on(ctx, case, ("async",))
    finally:
        ctx.destroy()


# ---- side effects ------------------------------------------------------------------------------------------------------------------
def test_a_call_with_a_box_restarts_the_accumulation_whether_or_not_anything_moves(base, blue_noise):
    mats0, mine0, _ = base
    p = ref.params(*sets.STACK_BOX, air_material=sets.AIR)                                # air above the floor: nothing to move
    beyond = ref.params((300, 10, 10), (310, 20, 20))
    u = [_u(POSE, seed) for seed in range(11, 16)]
    ctx = _ctx(mats0, mine0, spp=1, depth=2, flags=abi.RT_FLAG_CACHE_PRIMARY | abi.RT_FLAG_ACCUMULATE)
    try:
        ctx.upload_noise(blue_noise)
        ctx.draw_frame(u[0])
        ctx.draw_frame(u[1])
        assert ctx.accumulation() == (2, 2)
        ctx.settle_voxels_async(_p(beyond))                                              # an empty clipped box: nothing is reset
        ctx.draw_frame(u[2])
        assert ctx.accumulation() == (3, 3)
        bytes_before = ctx.info().device_bytes
        ctx.settle_voxels_async(_p(p))                                                   # nothing moves; the host cannot know
        ctx.draw_frame(u[3])
        assert ctx.accumulation() == (1, 1)
        # the scratch is the context's: a flag word per chunk of the box and a spare count record, counted in device_bytes
        grown = ctx.info().device_bytes - bytes_before
        assert 4 * 5 <= grown <= 4 * 5 + (1 << 20)
        assert ctx.settle_voxels(_p(p)).tolist() == (0, 0, 0, 0)
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
        ctx.settle_voxels_async(_p(ref.params((300, 10, 10), (310, 20, 20))))
        assert ctx.edit_boxes_pending() == (0, False)
        ctx.settle_voxels_async(_p(ref.params((60, 60, 100), (70, 70, 140), 1)))
        assert ctx.edit_boxes_pending() == (1, False)
        ctx.settle_voxels(_p(ref.params((-5, 60, 100), (3, 70, 140), 1, axis=0, toward=1)))
        assert ctx.edit_boxes_pending() == (2, False)
        ctx.sync()
        assert ctx.selftest(MAPS) == 0


# ---- refusals that need a device ---------------------------------------------------------------------------------------------------
def _rc(ctx, fn, p, counts):
    return getattr(ctx._lib, fn)(ctx._h, p, counts)


def test_refusals_and_what_they_leave(base):
    ctx, case = base[2], CASES["stack unlimited"]
    mats0, mine0 = sets.case_world(case)
    cnt = _counts0()
    t_c, h_c = _dev(cnt), cnt.copy()
    good = np.asarray(case["p"]).reshape(1).copy()
    P, K, HK = render._p(good), render._dp(t_c), render._p(h_c)
    INVALID, NOT_READY = abi.RT_ERR_INVALID_ARG, abi.RT_ERR_NOT_READY
    with render.Context(render.make_config(64, 40)) as fresh:                 # no world yet
        assert _rc(fresh, "rt_settle_voxels", P, HK) == NOT_READY
        assert _rc(fresh, "rt_settle_voxels_async", P, K) == NOT_READY
        assert _rc(fresh, "rt_settle_voxels_async", None, K) == INVALID
    _reset(ctx, mats0, mine0)
    table, expected, names = sets.params_table()
    for fn, k in (("rt_settle_voxels_async", K), ("rt_settle_voxels", HK)):
        assert _rc(ctx, fn, None, k) == INVALID
        assert _rc(ctx, fn, None, None) == INVALID
        for row, ok, name in zip(table, expected, names):
            if not ok:
                assert _rc(ctx, fn, render._p(np.asarray(row).reshape(1).copy()), k) == INVALID, name
        for name in ("box beyond the region", "box below the region"):
            empty = np.asarray(table[names.index(name)]).reshape(1).copy()
            assert _rc(ctx, fn, render._p(empty), k) == abi.RT_OK                     # an empty clipped box: nothing enqueued
    # the asynchronous call refuses host memory and a misaligned pointer, with an empty clipped box too
    assert _rc(ctx, "rt_settle_voxels_async", P, HK) == INVALID
    assert _rc(ctx, "rt_settle_voxels_async", P, C.c_void_p(t_c.data_ptr() + 8)) == INVALID
    assert b"16-byte aligned" in ctx._lib.rt_last_error(ctx._h)
    empty = np.asarray(table[names.index("box beyond the region")]).reshape(1).copy()
    assert _rc(ctx, "rt_settle_voxels_async", render._p(empty), HK) == INVALID
    ctx.sync()
    # a rejected call changes nothing
    assert t_c.cpu().numpy().tobytes() == cnt.tobytes() and h_c.tobytes() == cnt.tobytes()
    _check_world(ctx, case["p"], mats0, mine0, "after the refusals")
    with pytest.raises(ValueError):
        ctx.settle_voxels_async(_p(case["p"]), torch.zeros(16, dtype=torch.uint8))     # a host tensor
    with pytest.raises(ValueError):
        ctx.settle_voxels_async(_p(case["p"]), torch.zeros(32, dtype=torch.uint8, device="cuda"))


# ---- rt_bench --debris RADIUS --settle T --fall K --------------------------------------------------------------------------------------
def test_rt_bench_lets_the_rubble_fall_and_its_host_path_moves_the_same_voxels(native_built):
    """The mode exits non-zero unless the host path it times moves what the device's counts say."""
    import json
    import os
    import subprocess
    from tests.conftest import ROOT
    exe = os.path.join(ROOT, "raytrace_amd", "rt_bench")
    r = subprocess.run([exe, "--width", "64", "--height", "64", "--debris", "6", "--settle", "20", "--fall", "2"], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["debris"] == 6 and j["settle"] == 20 and j["fall"] == 2 and j["particles"] > 100
    assert j["moved"] == j["host_moved"] > 1000 and j["distance"] == j["host_distance"] >= j["moved"] and j["chunks"] > 0
    assert j["settle_device_ms"] > 0 and j["host_path_ms"] > 0
    bad = subprocess.run([exe, "--fall", "2"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--fall" in bad.stderr
