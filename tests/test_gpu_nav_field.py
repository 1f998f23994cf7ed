"""Navigation fields on the GPU (rt_nav_*).  Every comparison is bit for bit with tests/nav_field_ref.py: rt_nav_read's two arrays,
the result record (added and merged onto starting values that wrap), and the sampled steps, through both call variants; after every
build the world bytes and the nibble maps (RT_SELFTEST_SCENE_MAPS) are untouched.  The named cases of tests/nav_field_sets.py share
one region; then arbitrary minefield values, generated terrain, region 512, two runs of one call, a rebuild with another lo, a build
after an edit, the 64 fields, the samples' edges, the walk along `next`, the refusals that need a device and a frame round a build.
That the cases do what their names say is asserted from the restatement in tests/test_nav_field_contract.py."""
import numpy as np
import pytest
import torch

from raytrace_amd import abi, render
from oracle import pyoracle as po
from tests import adversarial_worlds as aw
from tests import nav_field_ref as ref
from tests import nav_field_sets as sets

pytestmark = pytest.mark.gpu

MAPS = abi.RT_SELFTEST_SCENE_MAPS
CASES = sets.placed(dict(sets.cases(), **sets.big_cases()))
RES0 = ref.result0(0xFFFFFFF0, 0xFFFFFFFE, 5, 0xFFFFFFFF, 0xFFFFFFFD, 7, (11, 13))


def _ctx(mats, mine, R=256, W=64, H=40, **kw):
    ctx = render.Context(render.make_config(W, H, region=R, **kw))
    ctx.upload_world(np.asarray(mats).reshape(-1), np.asarray(mine).reshape(-1))
    return ctx


def _dev(records):
    records = np.ascontiguousarray(records).reshape(-1)
    t = torch.from_numpy(records.view(np.uint8).reshape(len(records), -1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _host(t, dtype):
    return t.cpu().numpy().view(dtype).reshape(-1)


def _p(p):
    return abi.make_nav_build(p["lo"], p["max_dist"], p["height"], p["max_climb"], p["max_drop"], p["goal_snap"])


def _build(ctx, field, p, goals, call, res0=RES0):
    """One build -> its result as a ref.RESULT_DTYPE record (the asynchronous call's after sync())."""
    goals = abi.make_nav_goals(goals)
    if call == "async":
        t_r = _dev(np.asarray(res0).reshape(1))
        ctx.nav_build_async(field, _p(p), _dev(goals) if goals.size else None, t_r)
        ctx.sync()
        return _host(t_r, ref.RESULT_DTYPE)[0]
    got = ctx.nav_build(field, _p(p), goals, np.asarray(res0).reshape(1).view(abi.NAV_RESULT_DTYPE)[0])
    return np.asarray(got).reshape(1).view(ref.RESULT_DTYPE)[0]


def _sample(ctx, field, agents, call):
    agents = np.asarray(agents, dtype=ref.AGENT_DTYPE).reshape(-1)
    if call == "async":
        t_s = torch.full((max(len(agents), 1), 32), 0xA5, dtype=torch.uint8, device="cuda")[:len(agents)]
        ctx.nav_sample_async(field, _dev(agents), t_s)
        ctx.sync()
        return _host(t_s, ref.STEP_DTYPE)
    return ctx.nav_sample(field, agents.view(abi.NAV_AGENT_DTYPE)).view(ref.STEP_DTYPE)


def _same(got, want, what):
    dist, move, res = got
    assert np.array_equal(dist, want[0]), what + ": dist at %s" % np.argwhere(dist != want[0])[:4].tolist()
    assert np.array_equal(move, want[1]), what + ": move at %s" % np.argwhere(move != want[1])[:4].tolist()
    assert np.asarray(res).tobytes() == np.asarray(want[2]).tobytes(), (what, res, want[2])


def _run(ctx, occ, p, goals, call, what, mine=None, field=None):
    """A build of the box in a field of its own (or `field`), compared with the restatement; the world is read back when `mine`
    (the region as uploaded) is given.  Returns (dist, move) of the restatement."""
    want = ref.build_dilate(occ, p, goals, RES0)
    f = field if field is not None else ctx.nav_create(occ.shape[::-1])
    try:
        res = _build(ctx, f, p, goals, call)
        assert ctx.nav_info(f) == (occ.shape[::-1], tuple(p["lo"]), True)
        _same(ctx.nav_read(f) + (res,), want, what)
        assert ctx.selftest(MAPS) == 0, what
        if mine is not None:
            lo, e = p["lo"], occ.shape[::-1]
            got = ctx.read_box(lo, e)[1]
            assert np.array_equal(got, mine[lo[2]:lo[2] + e[2], lo[1]:lo[1] + e[1], lo[0]:lo[0] + e[0]]), what + ": world bytes"
    finally:
        if field is None:
            ctx.nav_destroy(f)
    return want[0], want[1]


@pytest.fixture(scope="module")
def base(native_built):
    mats, mine = sets.world(CASES)
    ctx = _ctx(mats, mine)
    yield mats, mine, ctx
    ctx.destroy()


# ---- the named cases, through both calls -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_a_case_equals_the_restatement_bit_for_bit(name, base):
    mats, mine, ctx = base
    c = CASES[name]
    p, goals = sets.params_of(c), sets.goals_of(c)
    assert np.array_equal(ref.box_occupied(mine, c["lo"], sets.ext_of(c)), c["occ"])
    for call in ("sync", "async"):
        _run(ctx, c["occ"], p, goals, call, "%s %s" % (name, call), mine=mine)


def test_two_runs_have_equal_bytes_and_a_rebuild_with_another_lo_leaves_no_stale_cell(base):
    mats, mine, ctx = base
    a, b = CASES["several goals"], CASES["no goal"]
    f = ctx.nav_create(sets.ext_of(a))
    try:
        first = None
        for _ in range(2):
            res = _build(ctx, f, sets.params_of(a), sets.goals_of(a), "async")
            got = tuple(x.tobytes() for x in ctx.nav_read(f)) + (res.tobytes(),)
            assert first is None or got == first
            first = got
        # the same field over another box, where nothing is reached, then over a box with fewer reachable cells
        _run(ctx, b["occ"], sets.params_of(b), sets.goals_of(b), "sync", "rebuild: no goal", field=f)
        p = ref.params(a["lo"], 3)
        _run(ctx, a["occ"], p, sets.goals_of(a)[:1], "async", "rebuild: max_dist 3", field=f)
    finally:
        ctx.nav_destroy(f)


def test_a_build_after_an_edit_sees_the_edit(base):
    mats, mine, ctx = base
    c = CASES["max_dist is the farthest cell"]
    lo = c["lo"]
    wall = (lo[0] + 10, lo[1], lo[2] + 1)
    try:
        ctx.edit_shapes([render.box_shape(wall, (wall[0], wall[1], wall[2] + 1), material=0x00707070, solid=True)])
        occ = c["occ"].copy()
        occ[1:3, 0, 10] = True
        d, _ = _run(ctx, occ, sets.params_of(c), sets.goals_of(c), "async", "walled")
        assert d[1, 0, 9] == 9 and d[1, 0, 11] == ref.UNREACHED
    finally:
        ctx.upload_world(mats.reshape(-1), mine.reshape(-1))
    _run(ctx, c["occ"], sets.params_of(c), sets.goals_of(c), "sync", "restored", mine=mine)


def test_64_fields_live_and_the_65th(base):
    ctx = base[2]
    before = ctx.info().device_bytes
    ids = [ctx.nav_create((3 + i % 5, 4, 2 + i % 3)) for i in range(64)]
    try:
        assert len(set(ids)) == 64 and 0 not in ids and ctx.info().device_bytes > before
        with pytest.raises(render.RtError) as e:
            ctx.nav_create((4, 4, 4))
        assert e.value.code == abi.RT_ERR_INVALID_ARG
        assert ctx.nav_info(ids[7]) == ((5, 4, 3), (0, 0, 0), False)
    finally:
        for i in ids:
            ctx.nav_destroy(i)
    assert ctx.info().device_bytes == before
    with pytest.raises(render.RtError):
        ctx.nav_info(ids[0])
    ctx.nav_destroy(ctx.nav_create((256, 256, 1)))


# ---- the samples ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stairs of rise 1 under max_climb 1", "cliff of 3 under max_drop 3", "goals duplicated, snapped and dropped"])
def test_samples_equal_the_restatement(name, base):
    ctx = base[2]
    c = CASES[name]
    p, goals, ext = sets.params_of(c), sets.goals_of(c), sets.ext_of(c)
    dist, move, _ = ref.build_dilate(c["occ"], p, goals)
    f = ctx.nav_create(ext)
    try:
        _build(ctx, f, p, goals, "sync")
        batches = [sets.every_cell_agents(c["lo"], ext), sets.every_cell_agents(c["lo"], ext, 8, 2), sets.odd_agents(c["lo"], ext)]
        assert any(len(b) % 64 for b in batches)
        for i, agents in enumerate(batches):
            want = ref.sample_array(dist, move, c["lo"], agents)
            for call in ("sync", "async"):
                got = _sample(ctx, f, agents, call)
                assert got.tobytes() == want.tobytes(), (name, i, call, np.flatnonzero(got != want)[:4].tolist())
        assert len(_sample(ctx, f, np.zeros(0, ref.AGENT_DTYPE), "sync")) == 0
        ctx.nav_sample_async(f, torch.zeros((0, 16), dtype=torch.uint8, device="cuda"), torch.zeros((0, 32), dtype=torch.uint8, device="cuda"))
    finally:
        ctx.nav_destroy(f)


def test_following_next_reaches_a_goal_in_dist_moves(base):
    ctx = base[2]
    c = CASES["serpentine maze re-enters tiles"]
    f = ctx.nav_create(sets.ext_of(c))
    try:
        _build(ctx, f, sets.params_of(c), sets.goals_of(c), "async")
        dist, move = ctx.nav_read(f)
    finally:
        ctx.nav_destroy(f)
    reached = np.argwhere(dist != ref.UNREACHED)
    assert len(reached) > 400
    # every reached cell's move leads to a cell one nearer: so the walk from it has exactly dist moves
    for z, y, x in reached:
        d = int(dist[z, y, x])
        if d == 0:
            assert move[z, y, x] == ref.NO_MOVE
            continue
        m = int(move[z, y, x])
        dx, dy = ref.STEPS_H[m & 3]
        assert int(dist[z + (m >> 2) - 8, y + dy, x + dx]) == d - 1
    far = reached[np.argmax(dist[tuple(reached.T)])]
    walk = ref.follow(dist, move, (far[2], far[1], far[0]))
    assert len(walk) == 450 and dist[walk[-1][2], walk[-1][1], walk[-1][0]] == 0


# ---- worlds of their own ----------------------------------------------------------------------------------------------------------------
def test_arbitrary_minefield_values():
    mats, mine, _, _ = aw.arbitrary_world(256, seed=3)
    mats, mine = np.asarray(mats).reshape(256, 256, 256), np.asarray(mine).reshape(256, 256, 256)
    lo, ext = (37, 61, 90), (45, 47, 24)
    occ = ref.box_occupied(mine, lo, ext)
    p = ref.params(lo, 200, height=1, max_climb=2, max_drop=8, goal_snap=8)
    st = np.argwhere(~occ[1:] & occ[:-1])
    goals = np.array([[x, y, z + 1 + 3] for z, y, x in st[:: max(1, len(st) // 40)]]) + np.array(lo)
    ctx = _ctx(mats, mine)
    try:
        d, _ = _run(ctx, occ, p, goals, "async", "arbitrary", mine=mine)
        assert np.count_nonzero(d != ref.UNREACHED) > 100
    finally:
        ctx.destroy()


def test_generated_terrain(procedural_region):
    mats, mine = (np.asarray(a).reshape(256, 256, 256) for a in procedural_region)
    surface = int(np.argmax(mine[:, 128, 128] != 0))   # the first unoccupied texel above (128, 128, 0)
    lo, ext = (80, 80, max(0, min(192, surface - 32))), (96, 96, 64)
    occ = ref.box_occupied(mine, lo, ext)
    p = ref.params(lo, 64, goal_snap=8)
    goals = np.array([[128, 128, min(255, surface + 4)], [90, 170, lo[2] + 63]])
    ctx = _ctx(mats, mine)
    try:
        d, _ = _run(ctx, occ, p, goals, "sync", "terrain", mine=mine)
        print("terrain: reached", np.count_nonzero(d != ref.UNREACHED))
        assert np.count_nonzero(d != ref.UNREACHED) > 50
    finally:
        ctx.destroy()


def test_region_512():
    R = 512
    mats, mine, _, _ = aw.arbitrary_world(R, seed=5)
    mats, mine = np.asarray(mats).reshape(R, R, R).copy(), np.asarray(mine).reshape(R, R, R).copy()
    c = CASES["stairs of rise 1 under max_climb 1"]
    ex, ey, ez = sets.ext_of(c)
    for lo in ((250, 255, 253), (R - ex, R - ey, R - ez)):
        box = mine[lo[2]:lo[2] + ez, lo[1]:lo[1] + ey, lo[0]:lo[0] + ex]
        box[...] = np.where(c["occ"], 0, np.maximum(box, 1))
    ctx = _ctx(mats, mine, R=R)
    try:
        for lo in ((250, 255, 253), (R - ex, R - ey, R - ez)):
            p = dict(sets.params_of(c), lo=lo)
            _run(ctx, c["occ"], p, np.asarray(c["goals"]) + np.array(lo), "async", "512 at %s" % (lo,), mine=mine)
    finally:
        ctx.destroy()


# ---- refusals that need a device, and the frame ------------------------------------------------------------------------------------------
def test_refusals(base):
    mats, mine, ctx = base
    c = CASES["several goals"]
    p, goals, ext = sets.params_of(c), abi.make_nav_goals(sets.goals_of(c)), sets.ext_of(c)
    f = ctx.nav_create(ext)
    lib, h = ctx._lib, ctx._h
    res = np.asarray(RES0).reshape(1).copy()
    try:
        def refused(rc, code=abi.RT_ERR_INVALID_ARG):
            assert rc == code, rc
            assert res.tobytes() == np.asarray(RES0).tobytes()
        pg, pr = goals.ctypes.data, res.ctypes.data
        ok = _p(p)
        import ctypes as C
        # a field never built
        refused(lib.rt_nav_sample(h, f, None, 0, None), abi.RT_ERR_NOT_READY)
        refused(lib.rt_nav_read(h, f, None, None), abi.RT_ERR_NOT_READY)
        refused(lib.rt_nav_build(h, f, None, pg, 2, pr))
        refused(lib.rt_nav_build(h, f + 1, C.byref(ok), pg, 2, pr))
        refused(lib.rt_nav_build(h, 0, C.byref(ok), pg, 2, pr))
        refused(lib.rt_nav_build(h, f, C.byref(ok), None, 2, pr))
        refused(lib.rt_nav_build(h, f, C.byref(ok), pg, 4097, pr))
        for field, v in (("max_dist", 0), ("max_dist", 4097), ("height", 0), ("height", 5), ("max_climb", 3), ("max_drop", 9), ("goal_snap", 9)):
            bad = _p(p)
            setattr(bad, field, v)
            refused(lib.rt_nav_build(h, f, C.byref(bad), pg, 2, pr))
        bad = _p(p)
        bad.reserved[2] = 1
        refused(lib.rt_nav_build(h, f, C.byref(bad), pg, 2, pr))
        for lo in ((-1, 0, 0), (256 - ext[0] + 1, 0, 0), (0, 0, 256 - ext[2] + 1)):
            bad = _p(dict(p, lo=lo))
            refused(lib.rt_nav_build(h, f, C.byref(bad), pg, 2, pr))
        # device pointers: a host address, a misaligned device address
        t = torch.zeros(64, dtype=torch.uint8, device="cuda")
        refused(lib.rt_nav_build_async(h, f, C.byref(ok), C.c_void_p(pg), 2, None))
        refused(lib.rt_nav_build_async(h, f, C.byref(ok), C.c_void_p(t.data_ptr()), 2, C.c_void_p(t.data_ptr() + 4)))
        assert ctx.nav_info(f)[2] is False
        with pytest.raises(ValueError):
            ctx.nav_build_async(f, ok, torch.zeros(16, dtype=torch.uint8), None)
        # built: the samples' own refusals
        _build(ctx, f, p, goals, "sync")
        agents = np.zeros(4, abi.NAV_AGENT_DTYPE)
        steps = np.zeros(4, abi.NAV_STEP_DTYPE)
        refused(lib.rt_nav_sample(h, f, None, 4, steps.ctypes.data))
        refused(lib.rt_nav_sample(h, f, agents.ctypes.data, 4, None))
        refused(lib.rt_nav_sample(h, f, agents.ctypes.data, (1 << 20) + 1, steps.ctypes.data))
        refused(lib.rt_nav_sample(h, f ^ 1, agents.ctypes.data, 4, steps.ctypes.data))
        refused(lib.rt_nav_sample_async(h, f, C.c_void_p(agents.ctypes.data), 4, C.c_void_p(t.data_ptr())))
        refused(lib.rt_nav_sample_async(h, f, C.c_void_p(t.data_ptr() + 8), 1, C.c_void_p(t.data_ptr() + 16)))
        assert not steps.view(np.uint8).any()
    finally:
        ctx.nav_destroy(f)
    with pytest.raises(render.RtError):
        ctx.nav_destroy(f)
    # no world resident
    empty = render.Context(render.make_config(64, 40))
    try:
        g = empty.nav_create(ext)
        with pytest.raises(render.RtError) as e:
            empty.nav_build(g, _p(p), goals)
        assert e.value.code == abi.RT_ERR_NOT_READY
    finally:
        empty.destroy()


def test_a_frame_drawn_before_and_after_a_build_has_equal_planes(procedural_region, blue_noise):
    mats, mine = (np.asarray(a).reshape(256, 256, 256) for a in procedural_region)
    ctx = _ctx(mats, mine, W=128, H=72, flags=abi.RT_FLAG_ACCUMULATE)
    try:
        ctx.upload_noise(blue_noise)
        pose = aw.POSES[0]
        u = po.camera_uniforms(pose["origin"], pose["heading"], pose["pitch"], pose["sun"], 3, (0, 0, 0))
        ctx.draw_frame(u)
        before = [ctx.readback(i).tobytes() for i in range(abi.RT_BUF_COUNT)]
        frames = ctx.accumulation()
        f = ctx.nav_create((64, 64, 64))
        ctx.nav_build(f, abi.make_nav_build((96, 96, 100), 64, goal_snap=8), np.array([[128, 128, 160]]))
        assert ctx.accumulation() == frames
        after = [ctx.readback(i).tobytes() for i in range(abi.RT_BUF_COUNT)]
        assert before == after
        ctx.reset_accumulation()
        ctx.draw_frame(u)
        assert [ctx.readback(i).tobytes() for i in range(abi.RT_BUF_COUNT)] == before
        ctx.nav_destroy(f)
    finally:
        ctx.destroy()
