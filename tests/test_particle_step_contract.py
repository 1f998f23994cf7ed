"""The particle-simulation rules without a GPU: properties of the restatement (tests/particle_step_ref.py) that follow from the
contract, and what the input sets of the GPU test hold, asserted from the restatement alone."""
import numpy as np
import pytest

from raytrace_amd import world
from tests import adversarial_worlds as aw
from tests import particle_step_ref as ref
from tests import particle_step_sets as sets
from tests import sweep_ref as sr

f32 = np.float32
SEAM_LR = (40, -24, 16)
EACH = ["free", "contacts 2", "contacts 3", "died of age"] + ["blocked %s%s" % (a, d) for a in "xyz" for d in "+-"]


def params(**kw):
    base = dict(dt=sets.DT, accel=sets.GRAVITY, damping=1.0, restitution=0.5, friction=0.75, rest_speed=0.25, sweeps=4)
    base.update(kw)
    return ref.Params(**base)


@pytest.fixture(scope="module")
def terrain(procedural_region):
    mats, mine = procedural_region
    occ = sr.Occupancy(mats, mine, (0, 0, 0), 256)
    states, kinds = sets.world_set(occ, 1)
    return occ, states, kinds


@pytest.fixture(scope="module")
def scrolled():
    mats, mine, _, _ = aw.arbitrary_world(256, seed=3)
    occ = sr.Occupancy(mats, mine, SEAM_LR, 256)
    states, kinds = sets.world_set(occ, 2)
    return occ, states, kinds


def _of(states, kinds, kind):
    return states[[i for i, k in enumerate(kinds) if k == kind]]


def test_a_free_tick_is_the_plain_ballistic_arithmetic(terrain):
    occ, states, kinds = terrain
    p = params(damping=0.9375)
    air = _of(states, kinds, "air")
    out, draw, logs = ref.step(occ, p, air)
    assert len(air) >= 8
    for s, o, d, hits in zip(air, out, draw, logs):
        assert [h["kind"] for h in hits] == [sr.FREE]
        for k in range(3):
            v = f32(f32(s["velocity"][k] + f32(p.accel[k] * p.dt)) * p.damping)
            m = f32(v * p.dt)
            assert abs(m) < 64 and o["velocity"][k] == v
            assert o["lo"][k] == f32(s["lo"][k] + m) and o["hi"][k] == f32(s["hi"][k] + m)
            assert d["center"][k] == f32(f32(o["lo"][k] + o["hi"][k]) * f32(0.5))
        assert int(o["flags"]) == int(s["flags"]) and o["life"] == np.inf and d["half"] == s["half"]


def test_a_particle_at_rest_keeps_its_box_bits(terrain):
    occ, states, kinds = terrain
    rest = _of(states, kinds, "rest")
    assert len(rest) >= 8
    for response in (ref.SLIDE, ref.STICK, ref.BOUNCE):
        cur = rest.copy()
        cur["flags"] = response
        p = params(rest_speed=4.0)          # a tick's fall from rest reaches 32 / 16 = 2 units per second
        for _ in range(6):
            nxt, _, logs = ref.step(occ, p, cur)
            assert nxt["lo"].tobytes() == rest["lo"].tobytes() and nxt["hi"].tobytes() == rest["hi"].tobytes()
            assert all(hits and hits[0]["kind"] == sr.BLOCKED and hits[0]["t"] == 0 and hits[0]["axis"] == 2 for hits in logs)
            assert (nxt["velocity"] == 0).all() and ((nxt["flags"] & ref.CONTACT) == 0x40000).all()
            cur = nxt


def test_a_bounce_without_accel_never_gains_speed_on_the_blocked_axis(terrain):
    occ, states, kinds = terrain
    sel = np.array([k.startswith("face") or k in ("edge", "corner", "nook") for k in kinds])
    cur = states[sel].copy()
    cur["flags"] = ref.BOUNCE
    p = params(accel=(0, 0, 0), restitution=1.0, friction=1.0, rest_speed=0.0)
    bounces = 0
    for _ in range(6):
        nxt, _, logs = ref.step(occ, p, cur)
        for c, n, hits in zip(cur, nxt, logs):
            for a in range(3):
                assert abs(n["velocity"][a]) <= abs(c["velocity"][a])
            bounces += sum(h["kind"] == sr.BLOCKED for h in hits)
        cur = nxt
    assert bounces >= 100


def test_one_sub_sweep_with_slide_is_one_sweep_plus_the_arithmetic(terrain):
    occ, states, kinds = terrain
    cur = states.copy()
    cur["flags"] = ref.SLIDE
    p = params(sweeps=1)
    out, _, _ = ref.step(occ, p, cur)
    blocked = 0
    for s, o in zip(cur, out):
        v = [f32(f32(s["velocity"][k] + f32(p.accel[k] * p.dt)) * p.damping) for k in range(3)]
        m = [min(max(f32(v[k] * p.dt), f32(-64)), f32(64)) for k in range(3)]
        if all(x == 0 for x in m):
            continue
        h = sr.sweep(occ, s["lo"], s["hi"], m)
        assert h["kind"] in (sr.FREE, sr.BLOCKED)
        assert np.float32(h["lo"]).tobytes() == o["lo"].tobytes() and np.float32(h["hi"]).tobytes() == o["hi"].tobytes()
        if h["kind"] == sr.BLOCKED:
            blocked += 1
            v[h["axis"]] = f32(0)
            assert int(o["flags"]) & ref.CONTACT == 0x10000 << h["axis"]
        assert np.float32(v).tobytes() == o["velocity"].tobytes()
    assert blocked >= 50


def test_slide_with_three_sub_sweeps_is_move_and_slide(terrain):
    occ, states, kinds = terrain
    cur = states.copy()
    cur["flags"] = ref.SLIDE
    p = params(accel=(0, 0, 0), sweeps=3)
    out, _, logs = ref.step(occ, p, cur)
    several = 0
    for s, o, hits in zip(cur, out, logs):
        m = [f32(s["velocity"][k] * p.dt) for k in range(3)]
        if all(x == 0 for x in m):
            assert not hits
            continue
        lo, hi, want = sr.move_and_slide(occ, s["lo"], s["hi"], m, 3)
        assert np.float32(lo).tobytes() == o["lo"].tobytes() and np.float32(hi).tobytes() == o["hi"].tobytes()
        assert sr.pack(want).tobytes() == sr.pack(hits).tobytes()
        several += len(want) >= 2
    assert several >= 30


@pytest.mark.parametrize("which", ["terrain", "scrolled"])
def test_the_closing_property_holds_over_fifty_ticks(which, request):
    occ, states, kinds = request.getfixturevalue(which)
    cur = states.copy()
    cur["flags"] = np.where(cur["flags"] == ref.DIE, ref.BOUNCE, cur["flags"])       # nobody leaves early
    cur["life"] = np.inf
    history = ref.run(occ, params(sweeps=3), cur, 50)                               # raises LiveParticleEmbedded if it fails
    last = history[-1][0]
    assert not (last["flags"] & (ref.DEAD | ref.INVALID)).any()
    assert sum(len(hits) for _, _, logs in history for hits in logs) >= 5000


@pytest.mark.parametrize("which", ["terrain", "scrolled"])
def test_every_set_holds_what_its_name_claims(which, request):
    occ, states, kinds = request.getfixturevalue(which)
    full, names = sets.with_table(states, kinds)
    out, _, logs = ref.step(occ, params(), full)
    n = sets.census(full, logs, out, sets.seam_planes(occ))
    for key in EACH:
        assert n[key] >= 8, (key, n)
    assert n["invalid"] >= 8 and 0 < n["inactive on input"] and n["inactive on input"] + n["invalid"] <= len(full) // 10
    assert sum(ref.inactive(s) for s in full) <= len(full) // 10
    assert n["embedded"] == 0                                                       # nobody starts inside a voxel
    if which == "scrolled":
        assert n["straddles seam"] >= 24 and all(v != 0 for v in occ.lr)
        across = [i for i, k in enumerate(names) if k == "seam"]
        assert sum(any(h["kind"] == sr.BLOCKED for h in logs[i]) for i in across) >= 8
    # EMBEDDED after an edit: a fill onto the resting particles
    rest = _of(states, kinds, "rest")
    boxes = [(occ.texel([int(np.floor(s["lo"][a])) for a in range(3)]),) * 2 + (True, 0x00FACADE) for s in rest]
    out2, _, logs2 = ref.step(sets.edited(occ, boxes), params(), rest)
    assert sets.census(rest, logs2, out2)["embedded"] >= 8 and (out2["flags"] & ref.DEAD).all()


def test_the_table_is_judged_as_it_is_labelled():
    table, verdicts, names = sets.record_table()
    for rec, verdict, name in zip(table, verdicts, names):
        got = "inactive" if ref.inactive(rec) else ("valid" if ref.valid(rec) else "invalid")
        assert got == verdict, name
    for name, kw, ok in sets.params_table():
        assert ref.params_valid(ref.Params(**kw)) == ok, name
    occ = sr.Occupancy(np.zeros(256 ** 3, np.uint32), np.ones(256 ** 3, np.uint8))     # an empty world
    out, draw, logs = ref.step(occ, params(), table)
    for rec, o, d, verdict, hits in zip(table, out, draw, verdicts, logs):
        if verdict == "inactive":
            assert o.tobytes() == rec.tobytes() and d["half"] == 0 and not hits
        elif verdict == "invalid":
            want = rec.copy()
            want["flags"] |= ref.INVALID
            assert o.tobytes() == want.tobytes() and d["half"] == 0 and not hits
        else:
            assert not int(o["flags"]) & ref.INVALID
        assert d["material"] == rec["material"] and d["light"] == rec["light"] and d["reserved"] == 0
