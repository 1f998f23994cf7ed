"""Particle deposits on the GPU (rt_deposit_particles, rt_deposit_particles_async).  Every comparison is bit for bit with
tests/deposit_particles_ref.py: the whole state array — a byte pattern in the fields no rule touches — the draw records, the counts,
and the region's minefield and materials through rt_read_box over the box's chunks and an untouched neighbour; the nibble maps
(RT_SELFTEST_SCENE_MAPS) after every case.  The named cases of tests/deposit_particles_sets.py through both calls, the eight-chunk
case on arbitrary minefield values (which show the chunks that were rebuilt and the ones that were not), the debris chain without a
host visit, frames and picks on the new world, the order against steps and carves, two runs of one call, region 512, the
accumulation reset and the pending box, and every refusal that needs a device.  That the cases deposit what their names say is
asserted from the restatement in tests/test_deposit_particles_contract.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from raytrace_amd import abi, render
from oracle import pyoracle as po
from tests import adversarial_worlds as aw
from tests import deposit_particles_ref as ref
from tests import deposit_particles_sets as sets
from tests import emit_particles_ref as eref
from tests import particle_step_ref as psr
from tests import shape_edits as se
from tests.test_gpu_edit_history import _ctx as _history_ctx
from tests.test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

MAPS = abi.RT_SELFTEST_SCENE_MAPS
CASES = sets.cases()
COUNTS0 = (7, 0xFFFFFFFF, 2, 3)                          # what the counters hold before a call: they are added to, and wrap


def _ctx(mats, mine, R=256, W=64, H=40, **kw):
    ctx = render.Context(render.make_config(W, H, region=R, **kw))
    ctx.upload_world(np.asarray(mats).reshape(-1), np.asarray(mine).reshape(-1))
    return ctx


def _reset(ctx, mats, mine):
    ctx.upload_world(np.asarray(mats).reshape(-1), np.asarray(mine).reshape(-1))


def _p(p):
    return abi.RtParticleDeposit.from_buffer_copy(np.asarray(p).tobytes())


def _dev(records):
    records = np.ascontiguousarray(records).reshape(-1)
    if len(records) == 0:
        return torch.zeros((0, records.dtype.itemsize), dtype=torch.uint8, device="cuda")
    t = torch.from_numpy(records.view(np.uint8).reshape(len(records), -1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _host(t, dtype):
    return t.cpu().numpy().view(dtype).reshape(-1)


def _same(got, want, what=""):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.dtype.itemsize == want.dtype.itemsize and len(got) == len(want), what
    if got.tobytes() != want.tobytes():
        for i in range(len(want)):
            assert got[i].tobytes() == want[i].tobytes(), (what, i, got[i], want[i])


def _counts0():
    c = np.zeros(1, ref.COUNT_DTYPE)
    c[0] = COUNTS0
    return c


def _hull(p, R, touched):
    """The chunks of the clipped box and one more along x — (origin, extent) in texels, and whether it holds an untouched chunk."""
    bb = ref.clipped_box(p, R)
    c0, c1 = [int(v) >> 6 for v in bb[0]], [int(v) >> 6 for v in bb[1]]
    if c1[0] + 1 < R // 64:
        c1[0] += 1
    else:
        c0[0] -= 1
    n = (c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1)
    return tuple(64 * v for v in c0), tuple(64 * (b - a + 1) for a, b in zip(c0, c1)), n > len(touched)


def _check_world(ctx, p, want_mats, want_mine, touched, what=""):
    R = want_mine.shape[0]
    o, e, spare = _hull(p, R, touched)
    assert spare
    gm, gf = ctx.read_box(o, e)
    sl = tuple(slice(o[k], o[k] + e[k]) for k in (2, 1, 0))
    assert np.array_equal(gf, want_mine[sl]), what + ": minefield"
    assert np.array_equal(gm, want_mats[sl]), what + ": materials"
    assert ctx.selftest(MAPS) == 0, what


def _async(ctx, p, states, draw, counts=True):
    t_s, t_d = _dev(states), None if draw is None else _dev(draw)
    t_c = _dev(_counts0()) if counts else None
    ctx.deposit_particles_async(_p(p), t_s, t_d, t_c)
    ctx.sync()
    return (_host(t_s, ref.STATE_DTYPE), None if draw is None else _host(t_d, ref.DRAW_DTYPE), _host(t_c, ref.COUNT_DTYPE) if counts else None)


@pytest.fixture(scope="module")
def base(native_built):
    mats, mine = sets.world()
    ctx = _ctx(mats, mine)
    yield mats, mine, ctx
    ctx.destroy()


# ---- the named cases through both calls --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_a_case_equals_the_restatement_bit_for_bit(name, base):
    mats0, mine0, ctx = base
    case = CASES[name]
    p, states, draw = case["p"], case["states"], sets.draw_of(case["states"])
    mats, mine = mats0.copy(), mine0.copy()
    want_s, want_d, want_c, touched = ref.deposit(mats, mine, p, states, draw, _counts0()[0])
    print(name, "counts", want_c, "touched", touched)
    for call in ("async", "sync"):
        _reset(ctx, mats0, mine0)
        if call == "async":
            got_s, got_d, got_c = _async(ctx, p, states, draw)
        else:
            got_s, got_d, got_c = ctx.deposit_particles(_p(p), states.view(abi.PARTICLE_STATE_DTYPE), draw.view(abi.PARTICLE_DTYPE),
                                                        _counts0().view(abi.DEPOSIT_COUNT_DTYPE)[0])
            ctx.sync()
        _same(got_s, want_s, call + " states")
        _same(got_d, want_d, call + " draw")
        _same(np.asarray(got_c).reshape(1), want_c.reshape(1), call + " counts")
        _check_world(ctx, p, mats, mine, touched, call)
    _reset(ctx, mats0, mine0)


def test_without_draw_and_counts_the_world_and_the_flags_change_alike(base):
    mats0, mine0, ctx = base
    case = CASES["count 65"]
    mats, mine = mats0.copy(), mine0.copy()
    want_s, _, _, touched = ref.deposit(mats, mine, case["p"], case["states"])
    got_s, _, _ = _async(ctx, case["p"], case["states"], None, counts=False)
    _same(got_s, want_s, "states")
    _check_world(ctx, case["p"], mats, mine, touched)
    _reset(ctx, mats0, mine0)
    got_s, got_d, got_c = ctx.deposit_particles(_p(case["p"]), case["states"].view(abi.PARTICLE_STATE_DTYPE))
    _same(got_s, want_s, "states of the synchronous call")
    assert got_d is None and got_c.tolist() == tuple(int(case["expect"][k]) for k in ("deposited", "voxels", "occupied", "outside"))
    _reset(ctx, mats0, mine0)


def test_two_runs_of_one_call_give_equal_bits(base):
    mats0, mine0, ctx = base
    case = CASES["shared"]
    runs = []
    for _ in range(2):
        _reset(ctx, mats0, mine0)
        got = _async(ctx, case["p"], case["states"], sets.draw_of(case["states"]))
        o, e, _ = _hull(case["p"], 256, [])
        runs.append(b"".join(a.tobytes() for a in got) + b"".join(a.tobytes() for a in ctx.read_box(o, e)))
    _reset(ctx, mats0, mine0)
    assert runs[0] == runs[1]


# ---- eight chunks on arbitrary minefield values: two are rebuilt, six keep bytes pack_into would never write ------------------------
def test_eight_chunks_on_arbitrary_values_rebuilds_two_and_leaves_six():
    mats, mine, _, _ = aw.arbitrary_world(256, seed=1)
    mats0, mine0 = mats.copy(), mine.copy()
    case = sets.eight_chunks_case(mine0)
    want_s, want_d, want_c, touched = ref.deposit(mats, mine, case["p"], case["states"], sets.draw_of(case["states"]), _counts0()[0])
    assert touched == [(0, 0, 0), (1, 1, 1)]
    ctx = _ctx(mats0, mine0)
    try:
        got_s, got_d, got_c = _async(ctx, case["p"], case["states"], sets.draw_of(case["states"]))
        _same(got_s, want_s, "states")
        _same(got_d, want_d, "draw")
        _same(got_c, want_c.reshape(1), "counts")
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
    finally:
        ctx.destroy()


# ---- the chain without a host visit --------------------------------------------------------------------------------------------------
def test_emit_carve_ticks_deposit_and_one_more_step_without_a_host_visit():
    c = sets.chain_reference()
    lr, n = sets.CHAIN_LR, sets.CHAIN_CAPACITY
    ctx = _ctx(*c["world"])
    try:
        t_ring, t_cur, t_draw, t_cnt = _dev(c["ring0"]), _dev(c["cursor0"]), _dev(np.zeros(n, ref.DRAW_DTYPE)), _dev(np.zeros(1, ref.COUNT_DTYPE))
        step = render.make_particle_step(lr=lr, **sets.CHAIN_STEP)
        ctx.emit_particles_async(sets.chain_emitters().view(abi.EMIT_DTYPE), lr, t_ring, n, t_cur)
        ctx.edit_shapes(se.batch([sets.CHAIN_BLAST]))
        for _ in range(sets.CHAIN_TICKS):
            ctx.step_particles_async(step, t_ring, t_ring, t_draw)
        ctx.deposit_particles_async(_p(sets.CHAIN_DEPOSIT), t_ring, t_draw, t_cnt)        # behind the steps, without a sync
        ctx.sync()                                                                       # the first host visit
        _same(_host(t_cur, eref.CURSOR_DTYPE), np.asarray(c["cursor"]).reshape(1), "cursor")
        _same(_host(t_ring, ref.STATE_DTYPE), c["deposited"], "ring after the deposit")
        _same(_host(t_draw, ref.DRAW_DTYPE), c["deposited_draw"], "draw records after the deposit")
        _same(_host(t_cnt, ref.COUNT_DTYPE), c["counts"].reshape(1), "counts")
        ctx.step_particles_async(step, t_ring, t_ring, t_draw)                           # the step sees the new voxels
        ctx.sync()
        _same(_host(t_ring, ref.STATE_DTYPE), c["last"], "ring after one more step")
        _same(_host(t_draw, ref.DRAW_DTYPE), c["last_draw"], "draw records after one more step")
        live = (c["deposited"]["flags"] & (psr.DEAD | psr.INVALID)) == 0
        assert (live & ((c["last"]["flags"] & psr.DEAD) != 0)).any()                      # a particle left in a new voxel died
        _check_world(ctx, sets.CHAIN_DEPOSIT, *c["world_after"], c["touched"], "chain")
    finally:
        ctx.destroy()


# ---- frames and picks --------------------------------------------------------------------------------------------------------------
FRAME_POSE = dict(origin=(-70.0, -100.0, 6.0), heading=np.pi / 2, pitch=-0.5, sun=0.3)
PICK_POSE = dict(origin=(-59.5, -64.0, 3.0), heading=np.pi / 2, pitch=-0.6, sun=0.3)


def _u(pose, seed=3):
    return po.camera_uniforms(pose["origin"], pose["heading"], pose["pitch"], pose["sun"], seed)


def test_a_frame_drawn_after_the_deposit_shows_the_voxels(base, blue_noise):
    mats0, mine0, _ = base
    case = CASES["count 257"]
    mats, mine = mats0.copy(), mine0.copy()
    ref.deposit(mats, mine, case["p"], case["states"])
    W, H, u = 64, 40, _u(FRAME_POSE)
    cpu, _ = po.render(mats.reshape(-1), mine.reshape(-1), blue_noise, u, W, H, 1, 3)
    old, _ = po.render(mats0.reshape(-1), mine0.reshape(-1), blue_noise, u, W, H, 1, 3)
    assert any(not np.array_equal(old[k], cpu[k]) for k in cpu)                          # the pose does look at the deposit
    ctx = _ctx(mats0, mine0, spp=1, depth=3)
    try:
        ctx.upload_noise(blue_noise)
        ctx.draw_frame(u)                                                                # a frame in flight on the old world
        t_s = _dev(case["states"])
        ctx.deposit_particles_async(_p(case["p"]), t_s)
        ctx.draw_frame(u)
        ctx.sync()
        _compare(ctx.readback_all(), cpu)
    finally:
        ctx.destroy()


def test_a_pick_on_a_deposited_voxel_returns_the_winners_material(base):
    mats0, mine0, ctx = base
    case = CASES["shared"]
    mats, mine = mats0.copy(), mine0.copy()
    ref.deposit(mats, mine, case["p"], case["states"])
    u = _u(PICK_POSE)
    xy = np.array([(x, y) for y in range(8, 32, 2) for x in range(20, 44, 2)])
    _reset(ctx, mats0, mine0)
    ctx.deposit_particles_async(_p(case["p"]), _dev(case["states"]))
    got = ctx.pick_pixels(u, xy)
    other = _ctx(mats, mine)
    try:
        assert got.tobytes() == other.pick_pixels(u, xy).tobytes()
    finally:
        other.destroy()
    _reset(ctx, mats0, mine0)
    on = (got["kind"] == abi.RT_HIT_SOLID) & (got["texel"] == (68, 68, 128)).all(axis=1)
    assert on.any() and (got["material"][on] == case["states"]["material"][sets.SHARED_WINNERS[0]]).all()


# ---- ordering against a carve of the same box ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["deposit", "carve"])
def test_a_deposit_and_a_carve_of_the_same_box_in_both_orders(base, first):
    mats0, mine0, ctx = base
    case = CASES["count 64"]
    p = case["p"]
    carve = se.box(tuple(int(v) for v in p["lo"]), tuple(int(v) for v in p["hi"]), 0x77, 0)
    mats, mine = mats0.copy(), mine0.copy()
    if first == "deposit":
        want_s, _, want_c, _ = ref.deposit(mats, mine, p, case["states"])
        se.apply_shapes(mats, mine, se.batch([carve]))
        assert not (mine[120:136, 30:71, 20:101] == 0).any()                              # the carve took the deposit with the floor
    else:
        se.apply_shapes(mats, mine, se.batch([carve]))
        want_s, _, want_c, _ = ref.deposit(mats, mine, p, case["states"])
        assert int(want_c["occupied"]) == 0 and int(want_c["deposited"]) > case["expect"]["deposited"]   # the sunk records find air now
    _reset(ctx, mats0, mine0)
    t_s, t_c = _dev(case["states"]), _dev(np.zeros(1, ref.COUNT_DTYPE))
    if first == "carve":
        ctx.edit_shapes(se.batch([carve]))
    ctx.deposit_particles_async(_p(p), t_s, None, t_c)
    if first == "deposit":
        ctx.edit_shapes(se.batch([carve]))
    ctx.sync()
    _same(_host(t_s, ref.STATE_DTYPE), want_s, "states")
    _same(_host(t_c, ref.COUNT_DTYPE), want_c.reshape(1), "counts")
    _check_world(ctx, p, mats, mine, [], first)
    _reset(ctx, mats0, mine0)


# ---- tile contexts and every RtKernel answer the same ------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(tile_rank=1, tile_world=2), dict(kernel=abi.RT_KERNEL_PATHS), dict(kernel=abi.RT_KERNEL_WAVEFRONT)],
                         ids=["tile 1 of 2", "paths", "wavefront"])
def test_tile_contexts_and_other_kernels_answer_the_same(kw):
    mats0, mine0 = sets.world()
    case = CASES["seam"]
    p, states, draw = case["p"], case["states"], sets.draw_of(case["states"])
    mats, mine = mats0.copy(), mine0.copy()
    want_s, want_d, want_c, touched = ref.deposit(mats, mine, p, states, draw, _counts0()[0])
    ctx = _ctx(mats0, mine0, **kw)
    try:
        got_s, got_d, got_c = _async(ctx, p, states, draw)
        _same(got_s, want_s, "states")
        _same(got_d, want_d, "draw")
        _same(got_c, want_c.reshape(1), "counts")
        _check_world(ctx, p, mats, mine, touched)
    finally:
        ctx.destroy()


# ---- region 512 --------------------------------------------------------------------------------------------------------------------
def test_region_512_under_a_scrolled_window():
    R, lr = 512, (72, -40, 24)
    mats, mine, _, _ = aw.arbitrary_world(R, seed=5)
    mats, mine = np.asarray(mats).reshape(R, R, R).copy(), np.asarray(mine).reshape(R, R, R).copy()
    mats0, mine0 = mats.copy(), mine.copy()
    lo, hi = (300, 440, 250), (340, 500, 262)                                             # across the seam y = 472, chunks y 6..7
    z, y, x = np.nonzero(mine0[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] != 0)
    pick = np.arange(0, len(z), max(1, len(z) // 700))[:700]
    texels = np.stack([x[pick] + lo[0], y[pick] + lo[1], z[pick] + lo[2]], axis=1).astype(np.int64)
    texels = np.concatenate([texels, texels[:40]])                                       # forty texels twice
    v = eref.world_voxels(texels, lr, R)
    p = ref.params(lo, hi, lr=lr)
    states = sets.resting(v)
    want_s, want_d, want_c, touched = ref.deposit(mats, mine, p, states, sets.draw_of(states), _counts0()[0])
    assert int(want_c["deposited"]) - COUNTS0[0] == len(v) and len(touched) >= 2
    ctx = _ctx(mats0, mine0, R=R)
    try:
        got_s, got_d, got_c = _async(ctx, p, states, sets.draw_of(states))
        _same(got_s, want_s, "states")
        _same(got_d, want_d, "draw")
        _same(got_c, want_c.reshape(1), "counts")
        _check_world(ctx, p, mats, mine, touched, "512")
    finally:
        ctx.destroy()


# ---- side effects ------------------------------------------------------------------------------------------------------------------
def test_a_call_with_a_box_restarts_the_accumulation_whether_or_not_it_deposits(base, blue_noise):
    mats0, mine0, _ = base
    case = CASES["nothing"]
    t_s = _dev(case["states"])
    beyond = ref.params((300, 10, 10), (310, 20, 20))
    u = [_u(FRAME_POSE, seed) for seed in range(11, 16)]
    ctx = _ctx(mats0, mine0, spp=1, depth=2, flags=abi.RT_FLAG_CACHE_PRIMARY | abi.RT_FLAG_ACCUMULATE)
    try:
        ctx.upload_noise(blue_noise)
        ctx.draw_frame(u[0])
        ctx.draw_frame(u[1])
        assert ctx.accumulation() == (2, 2)
        ctx.deposit_particles_async(_p(beyond), t_s)                                     # an empty clipped box: nothing is reset
        ctx.deposit_particles_async(_p(case["p"]), t_s[:0])                              # count == 0: nothing is reset
        ctx.draw_frame(u[2])
        assert ctx.accumulation() == (3, 3)
        bytes_before = ctx.info().device_bytes
        ctx.deposit_particles_async(_p(case["p"]), t_s)                                  # nothing deposits; the host cannot know
        ctx.draw_frame(u[3])
        assert ctx.accumulation() == (1, 1)
        # the scratch is the context's: a claim word per texel of the clipped box (16^3 here), counted in device_bytes
        grown = ctx.info().device_bytes - bytes_before
        assert 4 * 16 ** 3 <= grown <= 4 * 16 ** 3 + (1 << 20)
        ctx.sync()
        gm, gf = ctx.read_box((0, 0, 64), (192, 128, 128))
        assert np.array_equal(gf, mine0[64:192, :128, :192]) and np.array_equal(gm, mats0[64:192, :128, :192])
        assert ctx.selftest(MAPS) == 0
    finally:
        ctx.destroy()


def test_a_kept_history_takes_one_pending_box_per_call(procedural_region, blue_noise):
    case = CASES["nothing"]
    with _history_ctx(procedural_region, blue_noise) as ctx:
        t_s = _dev(case["states"])
        assert ctx.edit_boxes_pending() == (0, False)
        ctx.deposit_particles_async(_p(ref.params((300, 10, 10), (310, 20, 20))), t_s)
        assert ctx.edit_boxes_pending() == (0, False)
        ctx.deposit_particles_async(_p(case["p"]), t_s)
        assert ctx.edit_boxes_pending() == (1, False)
        ctx.deposit_particles(_p(CASES["clipped"]["p"]), CASES["clipped"]["states"].view(abi.PARTICLE_STATE_DTYPE))
        assert ctx.edit_boxes_pending() == (2, False)
        ctx.sync()
        assert ctx.selftest(MAPS) == 0


# ---- refusals that need a device ---------------------------------------------------------------------------------------------------
def _rc(ctx, fn, p, states, draw, count, counts):
    return getattr(ctx._lib, fn)(ctx._h, p, states, draw, count, counts)


def test_refusals_and_what_they_leave(base):
    mats0, mine0, ctx = base
    case = CASES["count 63"]
    states, draw, cnt = case["states"], sets.draw_of(case["states"]), _counts0()
    t_s, t_d, t_c = _dev(states), _dev(draw), _dev(cnt)
    h_s, h_d, h_c = states.copy(), draw.copy(), cnt.copy()
    good = np.asarray(case["p"]).reshape(1).copy()
    P, S, D, K = render._p(good), render._dp(t_s), render._dp(t_d), render._dp(t_c)
    HS, HD, HK = render._p(h_s), render._p(h_d), render._p(h_c)
    INVALID, NOT_READY = abi.RT_ERR_INVALID_ARG, abi.RT_ERR_NOT_READY
    with render.Context(render.make_config(64, 40)) as fresh:                 # no world yet
        assert _rc(fresh, "rt_deposit_particles", P, HS, HD, 63, HK) == NOT_READY
        assert _rc(fresh, "rt_deposit_particles_async", P, S, D, 63, K) == NOT_READY
    _reset(ctx, mats0, mine0)
    table, expected, names = sets.params_table()
    for fn, s, d, k in (("rt_deposit_particles_async", S, D, K), ("rt_deposit_particles", HS, HD, HK)):
        assert _rc(ctx, fn, P, None, None, 0, None) == abi.RT_OK
        assert _rc(ctx, fn, None, s, d, 63, k) == INVALID
        assert _rc(ctx, fn, None, None, None, 0, None) == INVALID
        assert _rc(ctx, fn, P, None, d, 63, k) == INVALID
        assert _rc(ctx, fn, P, s, d, (1 << 20) + 1, k) == INVALID
        for row, ok, name in zip(table, expected, names):
            if not ok:
                assert _rc(ctx, fn, render._p(np.asarray(row).reshape(1).copy()), s, d, 63, k) == INVALID, name
        empty = np.asarray(table[names.index("box beyond the region")]).reshape(1).copy()
        assert _rc(ctx, fn, render._p(empty), s, d, 63, k) == abi.RT_OK               # an empty clipped box: nothing enqueued
    # overlaps: the draw records inside the states, the counts inside the draw records
    assert _rc(ctx, "rt_deposit_particles_async", P, S, C.c_void_p(t_s.data_ptr() + 64), 63, K) == INVALID
    assert _rc(ctx, "rt_deposit_particles_async", P, S, D, 63, C.c_void_p(t_d.data_ptr() + 32)) == INVALID
    assert _rc(ctx, "rt_deposit_particles", P, HS, C.c_void_p(h_s.ctypes.data + 64), 60, HK) == INVALID
    assert b"overlap" in ctx._lib.rt_last_error(ctx._h)
    # the asynchronous call refuses host memory and a misaligned pointer
    assert _rc(ctx, "rt_deposit_particles_async", P, HS, D, 63, K) == INVALID
    assert _rc(ctx, "rt_deposit_particles_async", P, S, HD, 63, K) == INVALID
    assert _rc(ctx, "rt_deposit_particles_async", P, S, D, 63, HK) == INVALID
    assert _rc(ctx, "rt_deposit_particles_async", P, C.c_void_p(t_s.data_ptr() + 8), None, 32, K) == INVALID
    ctx.sync()
    # a rejected call changes nothing
    assert t_s.cpu().numpy().tobytes() == states.tobytes() and t_d.cpu().numpy().tobytes() == draw.tobytes() and t_c.cpu().numpy().tobytes() == cnt.tobytes()
    assert h_s.tobytes() == states.tobytes() and h_d.tobytes() == draw.tobytes() and h_c.tobytes() == cnt.tobytes()
    gm, gf = ctx.read_box((0, 0, 64), (128, 128, 128))
    assert np.array_equal(gf, mine0[64:192, :128, :128]) and np.array_equal(gm, mats0[64:192, :128, :128])
    with pytest.raises(ValueError):
        ctx.deposit_particles_async(_p(case["p"]), torch.zeros((63, 64), dtype=torch.uint8))     # a host tensor


def test_the_2_24_limit_passes_at_2_24_and_refuses_one_plane_more(base):
    """At R = 256 the whole region is 2^24 texels and passes; one plane more, at R = 512, is refused."""
    mats0, mine0, ctx = base
    states = sets.resting([(-60, -60, 0)])
    (logr, lo, hi) = sets.LIMIT_BOXES[0]
    assert logr == 8
    mats, mine = mats0.copy(), mine0.copy()
    want_s, _, want_c, touched = ref.deposit(mats, mine, ref.params(lo, hi), states)
    _reset(ctx, mats0, mine0)
    got_s, _, got_c = ctx.deposit_particles(_p(ref.params(lo, hi)), states.view(abi.PARTICLE_STATE_DTYPE))
    _same(got_s, want_s, "states")
    assert got_c.tolist() == (1, 1, 0, 0) and touched == [(1, 1, 2)]
    gm, gf = ctx.read_box((0, 0, 64), (192, 128, 128))
    assert np.array_equal(gf, mine[64:192, :128, :192]) and np.array_equal(gm, mats[64:192, :128, :192])
    assert ctx.selftest(MAPS) == 0
    _reset(ctx, mats0, mine0)
    with render.Context(render.make_config(64, 40, region=512)) as big:
        big.generate_world(1)
        (logr, lo, hi) = sets.LIMIT_BOXES[2]
        assert logr == 9
        with pytest.raises(render.RtError) as err:
            big.deposit_particles(_p(ref.params(lo, hi)), states.view(abi.PARTICLE_STATE_DTYPE))
        assert err.value.code == abi.RT_ERR_INVALID_ARG and "2^24" in str(err.value)


# ---- rt_bench --debris RADIUS --settle T ---------------------------------------------------------------------------------------------
def test_rt_bench_settles_debris_and_its_host_path_deposits_the_same_voxels(native_built):
    """The mode exits non-zero unless the host path it times deposits what the device's counts say."""
    import json
    import os
    import subprocess
    from tests.conftest import ROOT
    exe = os.path.join(ROOT, "raytrace_amd", "rt_bench")
    r = subprocess.run([exe, "--width", "64", "--height", "64", "--debris", "6", "--settle", "40"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["debris"] == 6 and j["settle"] == 40 and j["particles"] > 100
    assert j["voxels"] == j["host_voxels"] > 0 and j["deposited"] >= j["voxels"]
    assert j["deposit_device_ms"] > 0 and j["tick_device_ms"] > j["deposit_device_ms"] and j["host_path_ms"] > 0
    bad = subprocess.run([exe, "--settle", "5"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--settle" in bad.stderr
