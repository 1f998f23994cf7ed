"""Particle emitters on the GPU (rt_emit_particles, rt_emit_particles_async).  Every comparison is bit for bit with
tests/emit_particles_ref.py: the whole ring — a byte pattern before the call, so the untouched slots count — and the cursor.  The
named cases of tests/emit_particles_sets.py through both calls, two calls chained on the device's cursor, the debris recipe (emit,
carve, five ticks) without a host visit, the order of an emit against a carve, region 512, two runs of one call, every refusal that
needs a device, and the absence of side effects.  That the cases emit what their names say is asserted from the restatement in
tests/test_emit_particles_contract.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from raytrace_amd import abi, render
from tests import adversarial_worlds as aw
from tests import emit_particles_ref as ref
from tests import emit_particles_sets as sets
from tests import particle_step_ref as psr
from tests import shape_edits as se
from tests import sweep_ref as sr

pytestmark = pytest.mark.gpu

CASES = sets.cases()


def _ctx(mats, mine, R=256, W=64, H=40, **kw):
    ctx = render.Context(render.make_config(W, H, region=R, **kw))
    ctx.upload_world(np.asarray(mats).reshape(-1), np.asarray(mine).reshape(-1))
    return ctx


def _ring(capacity):
    """A ring of `capacity` records holding a byte pattern."""
    return ((np.arange(capacity * 64, dtype=np.uint32) * 37 + 11) % 251).astype(np.uint8).view(ref.STATE_DTYPE)


def _cursor(next, emitted=11, dropped=0xFFFFFFF0, reserved=0):
    c = np.zeros(1, dtype=ref.CURSOR_DTYPE)
    c[0] = (next, emitted, dropped, reserved)
    return c


def _dev(records):
    t = torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(len(records), -1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _same(got, want, what=""):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.dtype.itemsize == want.dtype.itemsize and len(got) == len(want), what
    if got.tobytes() != want.tobytes():
        for i in range(len(want)):
            assert got[i].tobytes() == want[i].tobytes(), (what, i, got[i], want[i])


def _emitters(case):
    return case["emitters"].view(abi.EMIT_DTYPE)


def _async(ctx, case, ring, cur):
    """The asynchronous call on device copies of `ring` and `cur` -> (ring, cursor) as the restatement's dtypes."""
    t_ring, t_cur = _dev(ring), _dev(cur)
    ctx.emit_particles_async(_emitters(case), case["lr"], t_ring, case["max_emit"], t_cur)
    ctx.sync()
    return t_ring.cpu().numpy().view(ref.STATE_DTYPE).reshape(-1), t_cur.cpu().numpy().view(ref.CURSOR_DTYPE).reshape(-1)


@pytest.fixture(scope="module")
def base(native_built):
    mats, mine = sets.world()
    ctx = _ctx(mats, mine)
    yield mats, mine, ctx
    ctx.destroy()


# ---- the named cases through both calls --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_a_case_equals_the_restatement_bit_for_bit(name, base):
    mats, mine, ctx = base
    case = CASES[name]
    ring, cur = _ring(case["capacity"]), _cursor(case["next"], reserved=0x55)
    N, want_ring, want_cur = ref.emit(mats, mine, case["emitters"], case["lr"], ring, case["max_emit"], cur[0])
    print(name, "N", N, "cursor", want_cur)
    assert (N == 0) == case["empty"]
    got_ring, got_cur = _async(ctx, case, ring, cur)
    _same(got_ring, want_ring, "ring")
    _same(got_cur, want_cur.reshape(1), "cursor")
    if case["next"] < case["capacity"]:                      # the synchronous call, on a cursor it accepts
        cur = _cursor(case["next"])
        N2, want_ring, want_cur = ref.emit(mats, mine, case["emitters"], case["lr"], ring, case["max_emit"], cur[0], device=False)
        assert N2 == N
        got_ring, got_cur = ctx.emit_particles(_emitters(case), case["lr"], ring.view(abi.PARTICLE_STATE_DTYPE), case["max_emit"],
                                               cur.view(abi.EMIT_CURSOR_DTYPE)[0])
        _same(got_ring, want_ring, "ring of the synchronous call")
        _same(np.asarray(got_cur).reshape(1), want_cur.reshape(1), "cursor of the synchronous call")


def test_density_37_keeps_a_strict_subset_of_density_256(base):
    mats, mine, ctx = base
    rings = {}
    for name in ("density 37", "density 256"):
        case = CASES[name]
        rings[name], cur = _async(ctx, case, _ring(case["capacity"]), _cursor(0, 0, 0))
        rings[name] = rings[name][:int(cur[0]["emitted"])]
    few, all_ = ({r["material"] for r in rings[n]} for n in ("density 37", "density 256"))   # (every voxel's word is different)
    assert 0 < len(few) < len(all_) == 1152 and few < all_


def test_two_calls_chained_on_the_device_cursor_without_a_sync(base):
    mats, mine, ctx = base
    first, second = CASES["sphere"], CASES["overlap"]
    ring, cur = _ring(200), _cursor(190)                     # the first call wraps; the second is cut by the ring's size
    _, want_ring, want_cur = ref.emit(mats, mine, first["emitters"], first["lr"], ring, 200, cur[0])
    N2, want_ring, want_cur = ref.emit(mats, mine, second["emitters"], second["lr"], want_ring, 150, want_cur)
    assert N2 > 150 and int(want_cur["dropped"]) == (0xFFFFFFF0 + N2 - 150) & 0xFFFFFFFF     # (the counter wraps)
    t_ring, t_cur = _dev(ring), _dev(cur)
    ctx.emit_particles_async(_emitters(first), first["lr"], t_ring, 200, t_cur)
    ctx.emit_particles_async(_emitters(second), second["lr"], t_ring, 150, t_cur)
    ctx.sync()
    _same(t_ring.cpu().numpy().view(ref.STATE_DTYPE).reshape(-1), want_ring, "ring")
    _same(t_cur.cpu().numpy().view(ref.CURSOR_DTYPE).reshape(-1), want_cur.reshape(1), "cursor")


def test_two_runs_of_one_call_give_equal_bits(base):
    mats, mine, ctx = base
    case = CASES["256 tiny"]
    a = _async(ctx, case, _ring(case["capacity"]), _cursor(case["next"]))
    b = _async(ctx, case, _ring(case["capacity"]), _cursor(case["next"]))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- the debris recipe: emit, carve, step — and the order of an emit against a carve -------------------------------------------------
def test_emit_carve_and_five_ticks_without_a_host_visit():
    mats, mine = (a.copy() for a in sets.world())
    lr = (0, 0, 0)
    blast = se.sphere((121, 121, 245), 121, material=0, solid=0)             # radius 5.5 round voxel (60, 60, 122)
    emitters = ref.batch([sets._e(blast, density=64, life_min=0.5, life_span=1.0, speed=9.0, spread=2.0)])
    kw = dict(dt=1.0 / 60.0, accel=(0.0, 0.0, -32.0), damping=1.0, restitution=0.5, friction=0.75, rest_speed=0.25, sweeps=3)
    ring = np.zeros(512, dtype=ref.STATE_DTYPE)
    ring["flags"], ring["material"] = psr.DEAD, np.arange(512)              # every slot inactive: the step copies what the emit leaves
    cur = _cursor(500, 0, 0)
    N, want_ring, want_cur = ref.emit(mats, mine, emitters, lr, ring, 512, cur[0])
    assert 100 <= N <= 400
    first = (500 + np.arange(N)) % 512
    ctx = _ctx(mats, mine)
    try:
        t_ring, t_cur, stepped = _dev(ring), _dev(cur), _dev(_ring(512))
        late_ring, late_cur = _dev(_ring(64)), _dev(_cursor(0, 0, 0))
        p = render.make_particle_step(lr=lr, **kw)
        ctx.emit_particles_async(emitters.view(abi.EMIT_DTYPE), lr, t_ring, 512, t_cur)
        ctx.edit_shapes(se.batch([blast]))                                   # the carve waits for the emit (ev_query)
        ctx.emit_particles_async(emitters.view(abi.EMIT_DTYPE), lr, late_ring, 64, late_cur)   # ... and this emit for the carve
        ctx.step_particles_async(p, t_ring, stepped, None)                   # the whole ring, first into a second buffer
        for _ in range(4):
            ctx.step_particles_async(p, stepped, stepped, None)
        ctx.sync()                                                           # the first host visit
        _same(t_ring.cpu().numpy().view(ref.STATE_DTYPE).reshape(-1), want_ring, "the emit before the carve sees the voxels it removes")
        _same(t_cur.cpu().numpy().view(ref.CURSOR_DTYPE).reshape(-1), want_cur.reshape(1), "cursor")
        assert late_cur.cpu().numpy().view(ref.CURSOR_DTYPE).reshape(-1)[0].tolist() == (0, 0, 0, 0)
        _same(late_ring.cpu().numpy().view(ref.STATE_DTYPE).reshape(-1), _ring(64), "the emit after the carve finds none of them")
        se.apply_shapes(mats, mine, se.batch([blast]))
        occ = sr.Occupancy(mats, mine, lr, 256)
        history = psr.run(occ, psr.Params(**kw), want_ring, 5)               # (raises if a live particle is ever EMBEDDED)
        got = stepped.cpu().numpy().view(ref.STATE_DTYPE).reshape(-1)
        _same(got, history[-1][0], "tick 5")
        assert not (got[first]["flags"] & (psr.DEAD | psr.INVALID)).any()    # lives are 0.5 s at least: nobody dies in five ticks
        assert (got[first]["lo"] != want_ring[first]["lo"]).any(axis=1).all()   # ... and everybody has moved
    finally:
        ctx.destroy()


# ---- tile contexts and every RtKernel answer the same ------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(tile_rank=1, tile_world=2), dict(kernel=abi.RT_KERNEL_PATHS), dict(kernel=abi.RT_KERNEL_WAVEFRONT)],
                         ids=["tile 1 of 2", "paths", "wavefront"])
def test_tile_contexts_and_other_kernels_answer_the_same(kw):
    mats, mine = sets.world()
    case = CASES["seam"]
    ring, cur = _ring(case["capacity"]), _cursor(case["next"])
    N, want_ring, want_cur = ref.emit(mats, mine, case["emitters"], case["lr"], ring, case["max_emit"], cur[0])
    ctx = _ctx(mats, mine, **kw)
    try:
        got_ring, got_cur = _async(ctx, case, ring, cur)
        sync_ring, sync_cur = ctx.emit_particles(_emitters(case), case["lr"], ring.view(abi.PARTICLE_STATE_DTYPE), case["max_emit"],
                                                 cur.view(abi.EMIT_CURSOR_DTYPE)[0])
    finally:
        ctx.destroy()
    assert N > 0
    for r, c in ((got_ring, got_cur), (sync_ring, np.asarray(sync_cur).reshape(1))):
        _same(r, want_ring, "ring")
        _same(c, want_cur.reshape(1), "cursor")


# ---- region 512, a scrolled window -----------------------------------------------------------------------------------------------
def test_region_512_under_a_scrolled_window():
    R, lr = 512, (72, -40, 24)
    mats, mine, _, _ = aw.arbitrary_world(R, seed=5)
    mats, mine = np.asarray(mats).reshape(R, R, R), np.asarray(mine).reshape(R, R, R)
    shapes = [se.sphere((2 * 300 + 1, 2 * 472 + 1, 2 * 255 + 1), 625), se.box((500, 0, 130), (520, 9, 139))]   # one over the seam y = 472
    emitters = ref.batch([sets._e(s, origin=(10.0, 20.0, 30.0), seed=i) for i, s in enumerate(shapes)])
    ring, cur = _ring(2048), _cursor(2040)
    N, want_ring, want_cur = ref.emit(mats, mine, emitters, lr, ring, 2048, cur[0])
    assert 50 <= N <= 2048
    ctx = _ctx(mats, mine, R=R)
    try:
        got_ring, got_cur = _async(ctx, dict(emitters=emitters, lr=lr, max_emit=2048), ring, cur)
    finally:
        ctx.destroy()
    _same(got_ring, want_ring, "ring")
    _same(got_cur, want_cur.reshape(1), "cursor")


# ---- refusals that need a device, and side effects -------------------------------------------------------------------------------
def _rc(ctx, fn, emitters, count, lr, states, capacity, max_emit, cursor):
    return getattr(ctx._lib, fn)(ctx._h, emitters, count, render._lr3(lr), states, capacity, max_emit, cursor)


def test_refusals_and_what_they_leave(base):
    mats, mine, ctx = base
    case = CASES["box 5x4x3"]
    em = _emitters(case)
    ring, cur = _ring(64), _cursor(3)
    t_ring, t_cur = _dev(ring), _dev(cur)
    h_ring, h_cur = ring.copy(), cur.copy()
    E, S, K, HS, HK = render._p(em), render._dp(t_ring), render._dp(t_cur), render._p(h_ring), render._p(h_cur)
    INVALID, NOT_READY = abi.RT_ERR_INVALID_ARG, abi.RT_ERR_NOT_READY
    with render.Context(render.make_config(64, 40)) as fresh:                 # no world yet
        assert _rc(fresh, "rt_emit_particles", E, 1, (0, 0, 0), HS, 64, 64, HK) == NOT_READY
        assert _rc(fresh, "rt_emit_particles", E, 0, (0, 0, 0), None, 0, 0, None) == abi.RT_OK
    for fn, s, k in (("rt_emit_particles_async", S, K), ("rt_emit_particles", HS, HK)):
        assert _rc(ctx, fn, E, 0, (0, 0, 0), None, 0, 0, None) == abi.RT_OK
        assert _rc(ctx, fn, None, 1, (0, 0, 0), s, 64, 64, k) == INVALID
        assert _rc(ctx, fn, E, 1, (0, 0, 0), None, 64, 64, k) == INVALID
        assert _rc(ctx, fn, E, 1, (0, 0, 0), s, 64, 64, None) == INVALID
        assert _rc(ctx, fn, E, 1, (0, 0, 0), s, 64, 0, k) == INVALID             # max_emit 0
        assert _rc(ctx, fn, E, 1, (0, 0, 0), s, 64, 65, k) == INVALID            # max_emit above capacity
        assert _rc(ctx, fn, E, 1, (0, 0, 0), s, (1 << 20) + 1, 64, k) == INVALID
        assert _rc(ctx, fn, E, 257, (0, 0, 0), s, 64, 64, k) == INVALID
        assert _rc(ctx, fn, E, 1, (2 ** 22 - 255, 0, 0), s, 64, 64, k) == INVALID
        bad = em.copy()
        bad["density"] = 0
        assert _rc(ctx, fn, render._p(bad), 1, (0, 0, 0), s, 64, 64, k) == INVALID
        assert b"emitter 0" in ctx._lib.rt_last_error(ctx._h)
        # more than 2^18 bricks: four emitters over the whole region
        whole = ref.batch([sets._e(se.box((0, 0, 0), (255, 255, 255)))] * 5).view(abi.EMIT_DTYPE)
        assert _rc(ctx, fn, render._p(whole), 5, (0, 0, 0), s, 64, 64, k) == INVALID
        assert b"2^18" in ctx._lib.rt_last_error(ctx._h)
    # the asynchronous call refuses host memory and a misaligned pointer; the synchronous one a cursor outside the ring or with reserved set
    assert _rc(ctx, "rt_emit_particles_async", E, 1, (0, 0, 0), HS, 64, 64, K) == INVALID
    assert _rc(ctx, "rt_emit_particles_async", E, 1, (0, 0, 0), S, 64, 64, HK) == INVALID
    assert _rc(ctx, "rt_emit_particles_async", E, 1, (0, 0, 0), C.c_void_p(t_ring.data_ptr() + 8), 32, 32, K) == INVALID
    for c in (_cursor(64), _cursor(3, reserved=1)):
        assert _rc(ctx, "rt_emit_particles", E, 1, (0, 0, 0), HS, 64, 64, render._p(c)) == INVALID
    ctx.sync()
    # a rejected call writes nothing
    assert t_ring.cpu().numpy().tobytes() == ring.tobytes() and t_cur.cpu().numpy().tobytes() == cur.tobytes()
    assert h_ring.tobytes() == ring.tobytes() and h_cur.tobytes() == cur.tobytes()
    with pytest.raises(ValueError):
        ctx.emit_particles_async(em, (0, 0, 0), torch.zeros((64, 64), dtype=torch.uint8), 64, t_cur)     # a host tensor


def test_a_call_changes_no_plane_and_device_bytes_count_the_scratch(base, blue_noise):
    mats, mine, ctx = base
    u = render.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, 0.0, 0.0, 1)
    ctx.upload_noise(blue_noise)
    ctx.draw_frame(u)
    ctx.sync()
    before = ctx.readback_all()
    bytes_before = ctx.info().device_bytes
    case = CASES["density 256"]
    _async(ctx, case, _ring(case["capacity"]), _cursor(0))
    # 20480 bricks: five rounds of the scan (4096 items each), and of scratch; the whole ring and the cursor against the restatement
    wide = dict(emitters=ref.batch([sets._e(se.box((0, 0, 112), (255, 255, 131)), density=64)]), lr=(0, 0, 0), max_emit=1 << 19)
    ring, cur = _ring(1 << 19), _cursor(77)
    N, want_ring, want_cur = ref.emit(mats, mine, wide["emitters"], wide["lr"], ring, wide["max_emit"], cur[0])
    assert ref.brick_boxes(wide["emitters"], 256)[1] == 20480 and 200000 < N < (1 << 19)
    got_ring, got_cur = _async(ctx, wide, ring, cur)
    assert got_ring.tobytes() == want_ring.tobytes() and got_cur.tobytes() == want_cur.tobytes()
    after = ctx.readback_all()
    for name in before:
        assert np.array_equal(before[name], after[name], equal_nan=True), name
    # masks and particle numbers, 12 bytes per brick; the block replaces an earlier call's, which held 1024 bricks at the most here
    assert ctx.info().device_bytes - bytes_before >= 12 * (20480 - 1024)
    assert ctx.info().device_bytes - bytes_before <= 16 * 20480 + (1 << 20)
