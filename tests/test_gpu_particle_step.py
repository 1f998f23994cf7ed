"""Particle simulation on the GPU (rt_step_particles, rt_step_particles_async).  Every comparison is bit for bit on whole 64-byte
states and 32-byte draw records with tests/particle_step_ref.py, which calls tests/sweep_ref.py for every sub-sweep: counts round the
workgroup edges, eight ticks chained on the device and in place, region 512 with a scrolled window and an arbitrary minefield, the
invalid and inactive table, draw == NULL, rt_sweep_boxes itself on the same boxes, edits between ticks, the device chain into
rt_draw_particles_async, every refusal, and the absence of side effects.  What the sets hold is asserted from the restatement
(tests/test_particle_step_contract.py does the same without a GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from raytrace_amd import abi, render
from tests import adversarial_worlds as aw
from tests import draw_particles_ref
from tests import draw_particles_sets
from tests import particle_step_ref as ref
from tests import particle_step_sets as sets
from tests import sweep_ref as sr

pytestmark = pytest.mark.gpu

COUNTS = [1, 63, 64, 65, 255, 256, 257, 2000]
f32 = np.float32
KW = dict(dt=sets.DT, accel=sets.GRAVITY, damping=1.0, restitution=0.5, friction=0.75, rest_speed=0.25)


def _params(occ, sweeps, **kw):
    """(the call's RtParticleStep, the restatement's Params) of one configuration."""
    kw = dict(KW, **kw)
    return render.make_particle_step(lr=occ.lr, sweeps=sweeps, **kw), ref.Params(sweeps=sweeps, **kw)


def _ctx(mats, mine, R=256, W=64, H=40, **kw):
    ctx = render.Context(render.make_config(W, H, region=R, **kw))
    ctx.upload_world(np.asarray(mats).reshape(-1), np.asarray(mine).reshape(-1))
    return ctx


def _same(got, want, what=""):
    """GPU records against the restatement's, byte for byte."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.dtype.itemsize == want.dtype.itemsize and len(got) == len(want)
    if got.tobytes() != want.tobytes():
        for i in range(len(want)):
            assert got[i].tobytes() == want[i].tobytes(), (what, i, got[i], want[i])


def _dev(records):
    return torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(len(records), -1).copy()).cuda()


def _fill(n, width):
    t = torch.full((n, width), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def _states(t):
    return t.cpu().numpy().view(ref.STATE_DTYPE).reshape(-1)


def _draws(t):
    return t.cpu().numpy().view(ref.DRAW_DTYPE).reshape(-1)


@pytest.fixture(scope="module")
def terrain(procedural_region):
    """The procedural region at lr = 0, its set with the table's records spread through it, one context, and the restated tick for
    sub-sweep budgets 1 and 4, computed once."""
    mats, mine = procedural_region
    occ = sr.Occupancy(mats, mine, (0, 0, 0), 256)
    states, kinds = sets.with_table(*sets.world_set(occ, 1))
    want = {sweeps: ref.step(occ, _params(occ, sweeps)[1], states) for sweeps in (1, 4)}
    n = sets.census(states, want[4][2], want[4][0])
    assert min(n[k] for k in n if k.startswith("blocked") or k in ("free", "contacts 2", "contacts 3", "died of age", "invalid")) >= 8, n
    assert sorted(set(int(f) & 3 for f in states["flags"])) == [0, 1, 2, 3]               # each response
    ctx = _ctx(mats, mine)
    yield occ, states, kinds, want, ctx
    ctx.destroy()


# ---- counts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweeps", [1, 4])
@pytest.mark.parametrize("count", COUNTS)
def test_counts_equal_the_restatement(count, sweeps, terrain):
    occ, states, kinds, want, ctx = terrain
    idx = np.arange(count) % len(states) if count > len(states) else np.arange(count) + (len(states) - count) // 2
    p, _ = _params(occ, sweeps)
    a, b, draw = _dev(states[idx]), _fill(count, 64), _fill(count, 32)
    ctx.step_particles_async(p, a, b, draw)                  # (the set holds invalid records: the device marks them)
    ctx.sync()
    _same(_states(b), want[sweeps][0][idx], "states")
    _same(_draws(draw), want[sweeps][1][idx], "draw records")
    _same(_states(a), states[idx], "the input")
    # the synchronous call on the records it accepts
    ok = np.array([ref.inactive(s) or ref.valid(s) for s in states[idx]])
    out, drw = ctx.step_particles(p, states[idx][ok].view(abi.PARTICLE_STATE_DTYPE))
    _same(out, want[sweeps][0][idx][ok], "states of the synchronous call")
    _same(drw, want[sweeps][1][idx][ok], "draw records of the synchronous call")


def test_an_empty_batch_is_ok_and_enqueues_nothing(terrain):
    occ, states, kinds, want, ctx = terrain
    out, draw = ctx.step_particles(_params(occ, 3)[0], states[:0].view(abi.PARTICLE_STATE_DTYPE))
    assert out.size == 0 and draw.size == 0


# ---- ticks chained on the device ----------------------------------------------------------------------------------------------------
def test_eight_ticks_chained_on_the_device_and_in_place(terrain):
    occ, states, kinds, want, ctx = terrain
    p, rp = _params(occ, 3)
    states = states.copy()
    ages = [i for i, k in enumerate(kinds) if k in ("air", "rest", "nook", "corner")][::3]
    states["life"][ages] = f32(5.5 * sets.DT)                # these die of age in the sixth tick
    history = ref.run(occ, rp, states, 8)
    assert sum(len(h) for _, _, logs in history for h in logs) < 10000
    dead = [int(((h[0]["flags"] & ref.DEAD) != 0).sum()) for h in history]
    assert dead[4] < dead[5] and dead[0] > 0 and dead[7] < len(states) // 2
    assert sum(len(h) for h in history[7][2]) > 50 and history[7][0]["lo"].tobytes() != history[6][0]["lo"].tobytes()   # still moving
    a, b, draw = _dev(states), _fill(len(states), 64), _fill(len(states), 32)
    inplace, draw2 = _dev(states), _fill(len(states), 32)
    for _ in range(8):                                       # no host visit between the ticks
        ctx.step_particles_async(p, a, b, draw)
        ctx.step_particles_async(p, inplace, inplace, draw2)
        a, b = b, a
    ctx.sync()
    _same(_states(a), history[-1][0], "tick 8")
    _same(_draws(draw), history[-1][1], "tick 8's draw records")
    _same(_states(b), history[-2][0], "tick 7, in the other buffer")
    _same(_states(inplace), history[-1][0], "in place")
    _same(_draws(draw2), history[-1][1], "in place, draw records")


# ---- region 512, a scrolled window, a minefield that bounds no distance ---------------------------------------------------------------
def test_region_512_across_the_seam_of_a_scrolled_arbitrary_world():
    R, lr = 512, (72, -40, 24)
    mats, mine, _, _ = aw.arbitrary_world(R, seed=5)
    occ = sr.Occupancy(mats, mine, lr, R)
    states, kinds = sets.with_table(*sets.world_set(occ, 3))
    p, rp = _params(occ, 4)
    history = ref.run(occ, rp, states, 2)
    n = sets.census(states, history[0][2], history[0][0], sets.seam_planes(occ))
    assert n["straddles seam"] >= 24 and min(n[k] for k in n if k.startswith("blocked")) >= 8, n
    across = [i for i, k in enumerate(kinds) if k == "seam"]
    assert sum(any(h["kind"] == sr.BLOCKED for h in history[0][2][i]) for i in across) >= 8
    texels = [h["texel"] for _, _, logs in history for hits in logs for h in hits if h["kind"] == sr.BLOCKED]
    assert (np.max(texels, axis=0) >= 256).all()             # texels beyond what region 256 addresses
    assert len(np.unique(mine)) > 16                         # values that bound no distance
    with _ctx(mats, mine, R=R) as ctx:
        a, b, draw = _dev(states), _fill(len(states), 64), _fill(len(states), 32)
        ctx.step_particles_async(p, a, b, draw)
        ctx.step_particles_async(p, b, a, draw)
        ctx.sync()
        _same(_states(b), history[0][0], "tick 1")
        _same(_states(a), history[1][0], "tick 2")
        _same(_draws(draw), history[1][1], "tick 2's draw records")


# ---- the invalid and inactive table ---------------------------------------------------------------------------------------------------
def test_the_table_is_copied_through_marked_and_not_drawn(terrain):
    occ, states, kinds, want, ctx = terrain
    table, verdicts, names = sets.record_table()
    p, rp = _params(occ, 2)
    w_out, w_draw, _ = ref.step(occ, rp, table)
    for rec, o, d, verdict in zip(table, w_out, w_draw, verdicts):
        if verdict != "valid":
            assert o["lo"].tobytes() == rec["lo"].tobytes() and o["velocity"].tobytes() == rec["velocity"].tobytes() and d["half"] == 0
            assert int(o["flags"]) == int(rec["flags"]) | (ref.INVALID if verdict == "invalid" else 0)
    a, b, draw = _dev(table), _fill(len(table), 64), _fill(len(table), 32)
    ctx.step_particles_async(p, a, b, draw)
    ctx.sync()
    _same(_states(b), w_out, "table")
    _same(_draws(draw), w_draw, "table's draw records")
    # the synchronous call refuses the whole batch for one active invalid record and writes nothing
    bad = names.index("NaN velocity")
    batch = np.concatenate([states[:40], table[bad:bad + 1], states[40:60]])
    out, drw = np.full(len(batch) * 64, 0x5A, np.uint8), np.full(len(batch) * 32, 0x5A, np.uint8)
    rc = ctx._lib.rt_step_particles(ctx.handle, C.byref(p), batch.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                    drw.ctypes.data_as(C.c_void_p), len(batch))
    assert rc == abi.RT_ERR_INVALID_ARG and (out == 0x5A).all() and (drw == 0x5A).all()
    # ... while inactive records pass it
    accepted = states[[ref.inactive(s) or ref.valid(s) for s in states]]
    quiet = np.concatenate([accepted[:40], table[[i for i, v in enumerate(verdicts) if v == "inactive"]]])
    got, _ = ctx.step_particles(p, quiet.view(abi.PARTICLE_STATE_DTYPE))
    _same(got, ref.step(occ, rp, quiet)[0], "inactive records in the synchronous call")


# ---- draw == NULL ---------------------------------------------------------------------------------------------------------------------
def test_without_draw_records(terrain):
    occ, states, kinds, want, ctx = terrain
    p, _ = _params(occ, 4)
    a, b = _dev(states), _fill(len(states), 64)
    ctx.step_particles_async(p, a, b, None)
    ctx.sync()
    _same(_states(b), want[4][0], "async, draw == NULL")
    ok = states[[not ref.inactive(s) and ref.valid(s) for s in states]]
    out = np.zeros(len(ok), dtype=ref.STATE_DTYPE)
    rc = ctx._lib.rt_step_particles(ctx.handle, C.byref(p), ok.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), None, len(ok))
    assert rc == abi.RT_OK
    _same(out, ref.step(occ, _params(occ, 4)[1], ok)[0], "sync, draw == NULL")


# ---- the library's own sweeps -----------------------------------------------------------------------------------------------------------
def test_one_sub_sweep_ends_where_rt_sweep_boxes_ends(terrain):
    occ, states, kinds, want, ctx = terrain
    p, rp = _params(occ, 1)
    live = states[[not ref.inactive(s) and ref.valid(s) for s in states]]
    v = ((live["velocity"] + (np.float32(rp.accel) * rp.dt)[None]) * rp.damping).astype(f32)
    m = np.clip((v * rp.dt).astype(f32), f32(-64), f32(64))
    moving = (m != 0).any(axis=1)
    hits = ctx.sweep_boxes(np.stack([live["lo"], live["hi"], m], axis=1)[moving])
    out, _ = ctx.step_particles(p, live.view(abi.PARTICLE_STATE_DTYPE))
    assert moving.sum() > 200 and set(np.unique(hits["kind"])) == {abi.RT_SWEEP_FREE, abi.RT_SWEEP_BLOCKED}
    assert out["lo"][moving].tobytes() == hits["lo"].tobytes() and out["hi"][moving].tobytes() == hits["hi"].tobytes()
    assert out["lo"][~moving].tobytes() == live["lo"][~moving].tobytes()
    blocked = hits["kind"] == abi.RT_SWEEP_BLOCKED
    assert (((out["flags"][moving] >> 16) & 7)[blocked] == 1 << hits["axis"][blocked]).all() and not (out["flags"][moving][~blocked] & ref.CONTACT).any()


# ---- edits between ticks ------------------------------------------------------------------------------------------------------------------
def test_edits_between_ticks_carve_the_floor_and_bury_particles(terrain):
    """Resting particles; rt_edit_shapes carves the cells under them: they fall on the next tick; a fill onto them kills them
    (EMBEDDED -> DEAD) — all enqueued without a host wait, each tick against the restatement on the world as edited so far."""
    occ, states, kinds, want, _ = terrain
    rest = states[[i for i, k in enumerate(kinds) if k == "rest"]].copy()
    rest["flags"] = ref.SLIDE
    assert len(rest) >= 8
    p, rp = _params(occ, 3)
    t1 = ref.step(occ, rp, rest)
    assert t1[0]["lo"].tobytes() == rest["lo"].tobytes()                                 # at rest
    carve = [(t, t, False, 0) for cells in sets.floor_texels(occ, rest) for t in cells]
    occ2 = sets.edited(occ, carve)
    t2 = ref.step(occ2, rp, t1[0])
    assert (t2[0]["lo"][:, 2] < t1[0]["lo"][:, 2]).all() and not (t2[0]["flags"] & ref.DEAD).any()   # every one falls
    word = 0x00FACADE
    fill = [(occ.texel([int(np.floor(s["lo"][a])) for a in range(3)]),) * 2 + (True, word) for s in t2[0]]
    occ3 = sets.edited(occ2, fill)
    t3 = ref.step(occ3, rp, t2[0])
    assert all(hits[0]["kind"] == sr.EMBEDDED and hits[0]["material"] == word for hits in t3[2]) and (t3[0]["flags"] & ref.DEAD).all()
    assert (t3[1]["half"] == 0).all() and (t2[1]["half"] > 0).all()
    with _ctx(occ.materials, occ.minefield) as ctx:
        a, b, c, d = _dev(rest), _fill(len(rest), 64), _fill(len(rest), 64), _fill(len(rest), 64)
        draws = [_fill(len(rest), 32) for _ in range(3)]
        ctx.step_particles_async(p, a, b, draws[0])
        ctx.edit_shapes([render.box_shape(lo, hi, material=w, solid=s) for lo, hi, s, w in carve])
        ctx.step_particles_async(p, b, c, draws[1])
        ctx.edit_shapes([render.box_shape(lo, hi, material=w, solid=s) for lo, hi, s, w in fill])
        ctx.step_particles_async(p, c, d, draws[2])
        ctx.sync()
        for k, (got, want_k) in enumerate(zip((b, c, d), (t1, t2, t3))):
            _same(_states(got), want_k[0], "tick %d" % (k + 1))
            _same(_draws(draws[k]), want_k[1], "tick %d's draw records" % (k + 1))


# ---- the device chain into the draw ---------------------------------------------------------------------------------------------------------
def test_step_then_draw_on_the_device_equals_the_restated_draw(procedural_region, blue_noise):
    W, H, nlights = 72, 40, 7
    mats, mine = procedural_region
    occ = sr.Occupancy(mats, mine, (0, 0, 0), 256)
    u = po.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 5, (0, 0, 0))
    cloud = draw_particles_sets.cloud(u, 600, seed=23, far=120.0, nlights=nlights)
    lights = draw_particles_sets.some_lights(nlights)
    box = np.minimum(cloud["half"], f32(0.25))[:, None]
    rng = np.random.default_rng(4)
    states = np.zeros(len(cloud), dtype=ref.STATE_DTYPE)
    states["lo"], states["hi"], states["half"] = cloud["center"] - box, cloud["center"] + box, cloud["half"]
    states["velocity"] = rng.uniform(-6, 6, (len(cloud), 3))
    states["material"], states["emission"], states["light"] = cloud["material"], cloud["emission"], cloud["light"]
    states["flags"] = np.arange(len(cloud)) % 4
    states["life"] = np.where(np.arange(len(cloud)) % 3 == 0, f32(sets.DT * 0.5), f32(np.inf))       # a third dies this tick
    p, rp = _params(occ, 3)
    w_states, w_draw, _ = ref.step(occ, rp, states)
    dead = (w_states["flags"] & ref.DEAD) != 0
    assert dead.sum() >= 200 and (~dead).sum() >= 300 and (w_draw["half"][dead] == 0).all()
    ctx = render.Context(render.make_config(W, H, spp=1, depth=2, flags=abi.RT_FLAG_CACHE_PRIMARY))
    try:
        ctx.upload_world(mats, mine)
        ctx.upload_noise(blue_noise)
        planes = lambda: {abi.BUFFER_NAMES[b]: ctx.readback(b) for b in range(abi.RT_BUF_COUNT)}
        ctx.draw_frame(u)
        ctx.sync()
        before = planes()
        restate = lambda recs: dict(draw_particles_ref.draw_particles({k: v for k, v in before.items() if k != "final_bgra8"}, u,
                                                                      recs.view(abi.PARTICLE_DTYPE), lights, W, H), final_bgra8=before["final_bgra8"])
        want = restate(w_draw)
        alive = restate(w_draw[~dead])
        ghosts = w_draw.copy()
        ghosts["half"] = states["half"]
        assert all(want[k].tobytes() == alive[k].tobytes() for k in want)                 # dead particles leave no pixel ...
        assert restate(ghosts)["depth_f32"].tobytes() != want["depth_f32"].tobytes()      # ... though some were in sight
        assert np.count_nonzero(want["depth_f32"] != before["depth_f32"]) > 50
        a, b, draw, dl = _dev(states), _fill(len(states), 64), _fill(len(states), 32), _dev(lights)
        ctx.step_particles_async(p, a, b, draw)                                            # no host read between the two
        ctx.draw_particles_async(u, draw, dl)
        ctx.sync()
        got = planes()
        for k in want:
            assert got[k].tobytes() == want[k].tobytes(), k
        _same(_states(b), w_states)
        ctx.draw_frame(u)                                                                  # a frame drawn later carries nothing over
        ctx.sync()
        again = planes()
        for k in before:
            assert again[k].tobytes() == before[k].tobytes(), k
    finally:
        ctx.destroy()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(terrain):
    occ, states, kinds, want, ctx = terrain
    lib = render._lib.amd()
    good = states[[not ref.inactive(s) and ref.valid(s) for s in states]][:4].copy()
    out, drw = np.full(4 * 64, 0x5A, np.uint8), np.full(4 * 32, 0x5A, np.uint8)
    p_in, p_out, p_draw = (x.ctypes.data_as(C.c_void_p) for x in (good, out, drw))
    p, rp = _params(occ, 3)
    pp = C.byref(p)
    with render.Context(render.make_config(64, 40)) as bare:                              # no world resident
        assert lib.rt_step_particles(bare.handle, pp, p_in, p_out, p_draw, 4) == abi.RT_ERR_NOT_READY
        assert lib.rt_step_particles(bare.handle, pp, p_in, p_out, p_draw, 0) == abi.RT_OK
    h = ctx.handle
    assert lib.rt_step_particles(h, None, None, None, None, 0) == abi.RT_OK
    assert lib.rt_step_particles_async(h, None, None, None, None, 0) == abi.RT_OK
    buf = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    d_in, d_out, d_draw = C.c_void_p(base), C.c_void_p(base + 1024), C.c_void_p(base + 2048)
    for fn, (i, o, d) in ((lib.rt_step_particles, (p_in, p_out, p_draw)), (lib.rt_step_particles_async, (d_in, d_out, d_draw))):
        assert fn(h, pp, i, o, d, (1 << 20) + 1) == abi.RT_ERR_INVALID_ARG
        assert fn(h, None, i, o, d, 4) == abi.RT_ERR_INVALID_ARG
        assert fn(h, pp, None, o, d, 4) == abi.RT_ERR_INVALID_ARG
        assert fn(h, pp, i, None, d, 4) == abi.RT_ERR_INVALID_ARG
        for name, kw, ok in sets.params_table():                                          # bad parameters
            if not ok:
                q = abi.RtParticleStep()
                q.dt, q.damping, q.restitution, q.friction, q.rest_speed, q.sweeps = (kw[k] for k in ("dt", "damping", "restitution", "friction", "rest_speed", "sweeps"))
                q.accel[:] = kw["accel"]
                assert fn(h, C.byref(q), i, o, d, 4) == abi.RT_ERR_INVALID_ARG, name
    assert lib.rt_step_particles_async(h, pp, p_in, p_out, p_draw, 4) == abi.RT_ERR_INVALID_ARG          # host addresses
    assert lib.rt_step_particles_async(h, pp, d_in, d_out, p_draw, 4) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_step_particles_async(h, pp, C.c_void_p(base + 4), d_out, d_draw, 1) == abi.RT_ERR_INVALID_ARG      # misaligned
    assert lib.rt_step_particles_async(h, pp, d_in, C.c_void_p(base + 1032), d_draw, 1) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_step_particles_async(h, pp, d_in, d_out, C.c_void_p(base + 2056), 1) == abi.RT_ERR_INVALID_ARG
    # overlapping but unequal in / out, and a draw range that reaches into either
    assert lib.rt_step_particles_async(h, pp, d_in, C.c_void_p(base + 64), d_draw, 4) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_step_particles_async(h, pp, C.c_void_p(base + 128), d_in, d_draw, 4) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_step_particles_async(h, pp, d_in, d_out, C.c_void_p(base + 128), 4) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_step_particles_async(h, pp, d_in, d_out, C.c_void_p(base + 1024 + 240), 4) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_step_particles(h, pp, p_in, C.c_void_p(good.ctypes.data + 64), p_draw, 4) == abi.RT_ERR_INVALID_ARG
    with pytest.raises(ValueError, match="overlap"):
        ctx.step_particles_async(p, buf[:256].view(4, 64), buf[64:320].view(4, 64), None)
    ctx.sync()
    assert not buf.any().item() and (out == 0x5A).all() and (drw == 0x5A).all()                            # a rejected call writes nothing
    got, _ = ctx.step_particles(p, good.view(abi.PARTICLE_STATE_DTYPE))
    _same(got, ref.step(occ, rp, good)[0])


# ---- no side effects ------------------------------------------------------------------------------------------------------------------------
def test_a_step_changes_no_counter_accumulation_or_history(procedural_region, blue_noise):
    mats, mine = procedural_region
    occ = sr.Occupancy(mats, mine, (0, 0, 0), 256)
    u = po.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 5, (0, 0, 0))
    states, _ = sets.world_set(occ, 1, per=4)
    flags = abi.RT_FLAG_ACCUMULATE | abi.RT_FLAG_REPROJECT | abi.RT_FLAG_CACHE_PRIMARY
    ctx = render.Context(render.make_config(72, 40, spp=1, depth=2, flags=flags))
    try:
        ctx.upload_world(mats, mine)
        ctx.upload_noise(blue_noise)
        for _ in range(3):
            ctx.draw_frame(u)
        ctx.sync()
        planes = [ctx.readback(b).tobytes() for b in range(abi.RT_BUF_COUNT)]
        counters, acc, history = bytes(ctx.counters()), ctx.accumulation(), ctx.read_history()
        a, draw = _dev(states), _fill(len(states), 32)
        ctx.step_particles_async(_params(occ, 3)[0], a, a, draw)
        ctx.step_particles(_params(occ, 3)[0], states.view(abi.PARTICLE_STATE_DTYPE))
        ctx.sync()
        assert bytes(ctx.counters()) == counters and ctx.accumulation() == acc and np.array_equal(ctx.read_history(), history)
        assert [ctx.readback(b).tobytes() for b in range(abi.RT_BUF_COUNT)] == planes
        assert len(np.unique(history)) >= 1 and acc[0] >= 1
    finally:
        ctx.destroy()
