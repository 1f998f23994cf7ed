"""The rules of rt_deposit_particles without a GPU: every candidate clause switched off one at a time, the target's floor on negatives
and on integers, both sides of the window's bound and of the box's faces, the lowest index winning a shared texel, the counts the
named cases of tests/deposit_particles_sets.py promise, the parameter table, and the debris chain — emit, carve, STICK ticks, deposit,
one more step — in the restatements alone, with the properties the GPU test of the same chain relies on."""
import numpy as np
import pytest

from tests import deposit_particles_ref as ref
from tests import deposit_particles_sets as sets
from tests import particle_step_ref as psr

R = 256
f32 = np.float32
BOX = ref.params((60, 60, 120), (75, 75, 135))          # world voxels -68..-53 in x and y, -8..7 in z under lr = 0
SPOT = (-60, -60, 0)                                    # air just above the floor, inside BOX
CASES = sets.cases()


def _world():
    return tuple(a.copy() for a in sets.world())


def _run(p, states, draw=True, counts=None):
    mats, mine = _world()
    before = mine.copy()
    s, d, c, touched = ref.deposit(mats, mine, p, states, sets.draw_of(states) if draw else None, counts)
    return s, d, c, touched, mats, mine, before


def _counts(c):
    return tuple(int(c[k]) for k in ("deposited", "voxels", "occupied", "outside"))


def test_a_resting_record_deposits_and_only_its_flags_and_half_change():
    states = sets.resting([SPOT])
    s, d, c, touched, mats, mine, before = _run(BOX, states)
    assert _counts(c) == (1, 1, 0, 0) and touched == [(1, 1, 2)]
    want = states.copy()
    want["flags"] |= psr.DEAD
    assert s.tobytes() == want.tobytes()
    want_d = sets.draw_of(states)
    want_d["half"] = 0
    assert d.tobytes() == want_d.tobytes() and d["half"].view(np.uint32)[0] == 0          # +0.0f
    assert mine[128, 68, 68] == 0 and before[128, 68, 68] != 0 and mats[128, 68, 68] == states["material"][0]
    assert (mine != before).any() and np.array_equal(mine[:, :, :64], before[:, :, :64])   # other chunks keep their bytes


def _off(name):
    s = sets.resting([SPOT])
    if name == "dead":
        s["flags"] |= psr.DEAD
    elif name == "invalid":
        s["flags"] |= psr.INVALID
    elif name == "no contact":
        s["flags"] &= ~np.uint32(psr.CONTACT)
    elif name == "speed just over":
        s["velocity"][0, 1] = np.nextafter(f32(0.25), f32(1))
    elif name == "nan velocity":
        s["velocity"][0, 2] = np.nan
    elif name == "lo at 2^22 + 1":
        s["lo"][0, 0] = f32(2 ** 22 + 1)
    elif name == "hi infinite":
        s["hi"][0, 2] = np.inf
    return s


@pytest.mark.parametrize("name", ["dead", "invalid", "no contact", "speed just over", "nan velocity", "lo at 2^22 + 1", "hi infinite"])
def test_each_candidate_clause_switched_off_stops_the_deposit(name):
    p = ref.params(BOX["lo"], BOX["hi"], max_speed=0.25)
    on = sets.resting([SPOT])
    on["velocity"][0, 1] = -0.25                          # at the threshold: still a candidate
    assert _counts(_run(p, on)[2]) == (1, 1, 0, 0)
    states = _off(name)
    s, d, c, touched, mats, mine, before = _run(p, states)
    assert _counts(c) == (0, 0, 0, 0) and touched == [] and np.array_equal(mine, before)
    assert s.tobytes() == states.tobytes() and d.tobytes() == sets.draw_of(states).tobytes()


def test_the_target_is_the_floor_of_the_centre_on_integers_and_negatives():
    def rec(lo, hi):
        s = sets.resting([SPOT])
        s["lo"][0], s["hi"][0] = lo, hi
        return s[0]
    assert ref.target(rec((-60.5, -60.5, -0.5), (-59.5, -59.5, 0.5))) == (-60, -60, 0)          # centred exactly on an integer
    assert ref.target(rec((-1.0, -1.0, -1.0), (0.0, 0.0, 0.0))) == (-1, -1, -1)                 # centre -0.5: floor, not truncation
    assert ref.target(rec((-0.25, 0.0, 0.75), (0.0, 0.25, 1.0))) == (-1, 0, 0)
    # one rounding for the sum, one for the half: 2^22 and the float below it sum to 2^23 - 0.25 -> 2^23 (ties to even) -> 2^22
    top = f32(2 ** 22)
    assert ref.target(rec((np.nextafter(top, f32(0)),) * 3, (top,) * 3)) == (2 ** 22,) * 3
    # on the world: a box centred on the integer -60 lands in voxel -60, one centred on -60.5 in voxel -61
    s = sets.resting([SPOT, SPOT])
    s["lo"][0, 0], s["hi"][0, 0] = -60.125, -59.875
    s["lo"][1, 0], s["hi"][1, 0] = -60.625, -60.375
    _, _, c, _, _, mine, _ = _run(BOX, s)
    assert _counts(c) == (2, 2, 0, 0) and mine[128, 68, 68] == 0 and mine[128, 68, 67] == 0


def test_a_target_on_each_side_of_the_window_bound_and_of_the_box_faces():
    lr = sets.LR_SEAM                                      # window x: [-88, 168)
    p = ref.params((0, 120, 120), (255, 135, 140), lr=lr)
    s = sets.resting([(-88, 0, 8), (-89, 0, 8), (167, 0, 8), (168, 0, 8)])
    what = ref.outcomes(sets.world()[1], p, s)
    assert what == [(40, 128, 136), "outside", (39, 128, 136), "outside"]
    # the box's faces, lr = 0: per axis the box's first and last texel are inside (the floor's texels count as occupied, not outside)
    for k in range(3):
        for t, inside in ((int(BOX["lo"][k]), True), (int(BOX["lo"][k]) - 1, False), (int(BOX["hi"][k]), True), (int(BOX["hi"][k]) + 1, False)):
            v = list(SPOT)
            v[k] = t - 128
            got = ref.outcomes(sets.world()[1], BOX, sets.resting([v]))[0]
            assert got is not None and (got != "outside") == inside, (k, t, got)


def test_five_records_into_one_texel_in_shuffled_order_the_lowest_index_wins_and_all_die():
    order = [3, 0, 4, 2, 1]
    s = sets.resting([SPOT] * 5)
    s["material"] = [0xB0 + j for j in order]              # record i carries a word that tells its place in `order`
    s2, d, c, touched, mats, mine, _ = _run(BOX, s)
    assert _counts(c) == (5, 1, 0, 0)
    assert mats[128, 68, 68] == 0xB3                       # record 0's word, whatever order the records were made in
    assert (s2["flags"] & psr.DEAD).all() and (d["half"] == 0).all()
    shuffled = s[[4, 2, 0, 3, 1]]
    assert _run(BOX, shuffled)[4][128, 68, 68] == shuffled["material"][0]


@pytest.mark.parametrize("name", list(CASES))
def test_a_named_case_gives_the_counts_its_name_promises(name):
    case = CASES[name]
    s, d, c, touched, mats, mine, before = _run(case["p"], case["states"], counts=(7, 0xFFFFFFFF, 2, 3))
    e = case["expect"]
    assert _counts(c) == ((7 + e["deposited"]) & 0xFFFFFFFF, (0xFFFFFFFF + e["voxels"]) & 0xFFFFFFFF, 2 + e["occupied"], 3 + e["outside"])
    assert int((s["flags"] & psr.DEAD != 0).sum()) - int((case["states"]["flags"] & psr.DEAD != 0).sum()) == e["deposited"]
    assert int(((mine == 0) & (before != 0)).sum()) == e["voxels"]
    assert (len(touched) == 0) == (e["voxels"] == 0)
    if e["voxels"] == 0:
        assert np.array_equal(mine, before)


def test_the_shared_case_puts_its_winners_where_the_waves_are():
    case = CASES["shared"]
    _, _, _, _, mats, _, _ = _run(case["p"], case["states"])
    for t, i in sets.SHARED_WINNERS.items():
        x, y, z = (v + 128 for v in sets.SHARED_TEXELS[t])
        assert mats[z, y, x] == case["states"]["material"][i]
    assert sets.SHARED_WINNERS[0] // 64 == (300 - 1) // 64 and sets.SHARED_WINNERS[1] // 64 == 0     # the last wave, the first wave


def test_the_eight_chunk_case_touches_two_chunks():
    from tests import adversarial_worlds as aw
    mats, mine, _, _ = aw.arbitrary_world(R, seed=1)
    mats, mine = mats.copy(), mine.copy()
    case = sets.eight_chunks_case(mine)
    before = mine.copy()
    assert len(ref.box_chunks(ref.clipped_box(case["p"], R))) == 8
    _, _, c, touched = ref.deposit(mats, mine, case["p"], case["states"])
    assert _counts(c) == (7, 6, 0, 0) and touched == [(0, 0, 0), (1, 1, 1)]
    # on arbitrary minefield values the rebuild is observable: the touched chunks change beyond the deposited voxels
    assert int((mine[:64, :64, :64] != before[:64, :64, :64]).sum()) > 3
    assert np.array_equal(mine[:64, :64, 64:128], before[:64, :64, 64:128])


def test_the_parameter_table_and_the_clipped_boxes():
    table, expected, names = sets.params_table()
    got = [ref.valid(p, R) for p in table]
    assert got == expected.tolist(), [n for n, g, w in zip(names, got, expected) if g != w]
    assert ref.clipped_box(table[names.index("box beyond the region")], R) is None
    bb = ref.clipped_box(table[names.index("box across a face")], R)
    assert bb[0].tolist() == [0, 30, 120] and bb[1].tolist() == [20, 50, 140] and ref.box_texels(bb) == 21 * 21 * 21
    assert len(ref.box_chunks(bb)) == 2 and ref.box_chunks(bb)[0] == (0, 0, 1)
    texels = [ref.box_texels(ref.clipped_box(ref.params(lo, hi), 1 << logr)) for logr, lo, hi in sets.LIMIT_BOXES]
    assert texels == [1 << 24, (1 << 24) + 1, 256 * 256 * 257]


def test_the_debris_chain_in_the_restatements_deposits_shares_and_leaves_one_to_die():
    c = sets.chain_reference()
    assert c["N"] == 125 and int(c["cursor"]["next"]) == (150 + 125) % sets.CHAIN_CAPACITY
    dep, voxels, occupied, outside = _counts(c["counts"])
    assert voxels >= 8 and dep > voxels and occupied + outside >= 1           # deposits, a shared texel, a candidate turned away
    assert (dep, voxels, occupied, outside) == (30, 15, 0, 20)
    assert c["touched"] == [(0, 0, 2), (0, 1, 2)]                      # the block straddles y = 64
    mine0, mine1 = c["world"][1], c["world_after"][1]
    assert int(((mine1 == 0) & (mine0 != 0)).sum()) == 15 and (mine1[128, 60:65, 60:63] == 0).all()
    # a live particle left overlapping a deposited voxel dies at the extra step; the others above it come to rest on the new voxels
    live_before = (c["deposited"]["flags"] & (psr.DEAD | psr.INVALID)) == 0
    died = live_before & ((c["last"]["flags"] & psr.DEAD) != 0)
    assert 1 <= int(died.sum()) and (c["last"]["life"][died] > 0).all()
    rested = live_before & ~died & ((c["last"]["flags"] & psr.CONTACT) != 0)
    assert int(rested.sum()) >= 1 and (c["last"]["lo"][rested, 2] >= 0).all()
