"""rt_flow_voxels' rules without a GPU, judged on the restatement (tests/flow_voxels_ref.py): its two statements of the tick — a loop per
cell over explicit neighbours and whole-array shifts — agree on every case of tests/flow_voxels_sets.py, the ledge fixture gives the rows
the header's example names, T calls of one tick equal one call of T on every occupied cell and on the whole minefield (they may differ in
the words of unoccupied cells, and in the tag bits of a cell that dried and was wetted again on the way), a world whose source was
removed dries within the ticks its case names, a fixed point reports active = 0 and a further call changes no byte, and the parameter
tables carry the verdicts their rows name."""
import numpy as np
import pytest

from tests import adversarial_worlds as aw
from tests import flow_voxels_ref as ref
from tests import flow_voxels_sets as sets

CASES = sets.cases()


def _flow(case, tick=ref.tick_shifts, p=None):
    mats, mine = sets.case_world(case)
    cnt, touched, s = ref.flow(mats, mine, case["p"] if p is None else p, tick=tick)
    return mats, mine, cnt, touched, s


@pytest.mark.parametrize("name", list(CASES))
def test_the_two_restatements_agree(name):
    a, b = _flow(CASES[name], ref.tick_cells), _flow(CASES[name], ref.tick_shifts)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes() and a[3] == b[3] and np.array_equal(a[4], b[4])
    assert int(a[2]["changed"]) > 0                                              # every case does something


def test_the_two_restatements_agree_tick_by_tick_on_a_tile_sized_slice_of_the_arbitrary_world():
    mats, mine, _, _ = aw.arbitrary_world(256, seed=1)
    mats, mine, p = sets.tiles_world(mats, mine, 3)
    sl = tuple(slice(sets.TILES_LO[k], sets.TILES_LO[k] + (20, 18, 17)[k]) for k in (2, 1, 0))
    s, _ = ref.seed(mats[sl], mine[sl], p)
    assert {int(v) for v in np.unique(s)} == set(range(16)) - set(range(8, 14))    # empty, strengths 0..7 (raw 8..14 are 7), source, fixed
    for _ in range(3):
        a, b = ref.tick_cells(s, 7), ref.tick_shifts(s, 7)
        assert np.array_equal(a, b) and not np.array_equal(a, s)
        s = a


def test_the_ledge_gives_the_rows_of_the_example():
    _, mine, cnt, touched, s = _flow(CASES["ledge"])
    assert s[4, 1].tolist() == sets.LEDGE_RUN and s[0, 1].tolist() == sets.LEDGE_FLOOR
    assert s[1:4, :, 4].tolist() == [[7, 7, 7]] * 3                              # the fall: max_level all the way down
    assert s[0, 0].tolist() == sets.LEDGE_FLOOR and s[4, 0].tolist() == [7, 6, 5, 4, 3, 0, 0, 0, 0, 0, 0, 0]
    assert touched == [(1, 1, 2)] and int(cnt["chunks"]) == 1 and int(cnt["dried"]) == 0
    assert int(cnt["wetted"]) == int(((s >= 1) & (s < ref.SOURCE)).sum()) == int(cnt["changed"])
    assert int(cnt["active"]) == 0                                               # LEDGE_TICKS is the fixed point ...
    assert int(_flow(CASES["ledge"], p=ref.with_(CASES["ledge"]["p"], ticks=sets.LEDGE_TICKS - 1))[2]["active"]) > 0   # ... and no tick sooner


def test_a_wetted_cell_gets_fluid_word_and_a_fluid_cell_keeps_its_own_bits():
    case = CASES["random 13 x 11 x 9"]
    mats0, mine0 = sets.case_world(case)
    mats, mine, cnt, _, s = _flow(case)
    bb = ref.clipped_box(case["p"], 256)
    sl = ref.box_slices(bb)
    s0, flowing0 = ref.seed(mats0[sl], mine0[sl], case["p"])
    flows = (s >= 1) & (s < ref.SOURCE)
    assert ((mats[sl][flows] & 0xF) == s[flows]).all() and (mine[sl][flows] == 0).all()
    assert (mats[sl][flows & ~flowing0] & ~np.uint32(0xF) == sets.WATER).all()
    assert ((mats[sl] ^ mats0[sl])[flows & flowing0] & ~np.uint32(0xF) == 0).all() and (flows & flowing0).any()
    dried = flowing0 & ~flows
    assert dried.any() and (mats[sl][dried] == sets.AIR).all() and (mine[sl][dried] != 0).all()
    keep = ~flows & ~dried
    assert np.array_equal(mats[sl][keep], mats0[sl][keep]) and np.array_equal(mine[sl][keep] == 0, mine0[sl][keep] == 0)
    assert {int(v) for v in np.unique((mats0[sl][flowing0] & 0xF))} >= {0, 8, 14}   # strength 0, raw levels above max_level, the value 14
    # nothing outside the box but the minefield bytes of the dirty chunk
    out = np.ones(mats.shape, bool)
    out[sl] = False
    assert np.array_equal(mats[out], mats0[out])


@pytest.mark.parametrize("name,T", [("ledge", 9), ("random 13 x 11 x 9", 6), ("ledge without its source", 7)])
def test_t_calls_of_one_tick_equal_one_call_of_t(name, T):
    case = CASES[name]
    p1, pT = ref.with_(case["p"], ticks=1), ref.with_(case["p"], ticks=T)
    m1, f1 = sets.case_world(case)
    c1 = None
    for _ in range(T):
        c1, _, s1 = ref.flow(m1, f1, p1, c1)
    mT, fT, cT, _, sT = _flow(case, p=pT)
    assert np.array_equal(s1, sT) and np.array_equal(f1, fT)
    # every occupied cell holds the same word — but for a fluid cell that dried and was wetted again on the way: the one call keeps the
    # bits of its own word outside FIELD, the single ticks gave it fluid_word's; the level agrees
    odd = (fT == 0) & (m1 != mT)
    assert ((m1[odd] ^ mT[odd]) & 0xFF00000F == 0).all() and (m1[odd] & ~np.uint32(0xF) == sets.WATER).all() and (mT[odd] >> 24 == 0x5A).all()
    assert odd.any() == (name == "random 13 x 11 x 9")
    assert int(c1["active"]) >= int(cT["active"])                                # added up over the single ticks
    if name != "ledge":                                                          # a cell that was wet on the way holds air_material after the single ticks
        assert set(np.unique(m1[(m1 != mT) & (fT != 0)]).tolist()) == {sets.AIR}


def test_without_its_source_the_ledge_dries_within_the_ticks_the_case_names():
    case = CASES["ledge without its source"]
    mats0, mine0 = sets.case_world(case)
    mats, mine, cnt, touched, s = _flow(case)
    assert not ((s >= 1) & (s <= ref.SOURCE)).any() and int(cnt["active"]) == 0 and int(cnt["wetted"]) == 0
    assert int(cnt["dried"]) == int(cnt["changed"]) == int(((mats0 >> 24 == 0x5A) & (mine0 == 0))[ref.box_slices(ref.clipped_box(case["p"], 256))].sum()) > 30
    wet = _flow(case, p=ref.with_(case["p"], ticks=sets.DRY_TICKS // 2))[4]
    assert ((wet >= 1) & (wet < ref.SOURCE)).any()                               # it takes its time: half the ticks leave fluid


@pytest.mark.parametrize("name", ["ledge", "ledge, forty ticks", "ledge without its source"])
def test_at_a_fixed_point_nothing_is_active_and_a_further_call_changes_no_byte(name):
    mats, mine, cnt, _, s = _flow(CASES[name])
    assert int(cnt["active"]) == 0
    m2, f2 = mats.copy(), mine.copy()
    again, touched, s2 = ref.flow(m2, f2, CASES[name]["p"])
    assert again.tobytes() == np.zeros(1, ref.COUNT_DTYPE).tobytes() and touched == [] and np.array_equal(s, s2)
    assert np.array_equal(m2, mats) and np.array_equal(f2, mine)


def test_three_hundred_random_boxes_reach_a_fixed_point():
    rng = np.random.default_rng(12)
    slowest = 0
    for _ in range(300):
        ext = rng.integers(1, 14, 3)
        s = rng.choice([0, 0, 0, 0, 15, 15, 14] + list(range(1, 8)), size=tuple(ext)).astype(np.int64)
        for t in range(200):
            n = ref.tick_shifts(s, 7)
            if np.array_equal(n, s):
                break
            s = n
        else:
            raise AssertionError("no fixed point in 200 ticks")
        slowest = max(slowest, t)
    print("slowest", slowest)


def test_the_parameter_tables_carry_their_verdicts():
    table, expected, names = sets.params_table()
    got = [ref.valid(p, 256) for p in table]
    assert got == expected.tolist(), [n for n, g, w in zip(names, got, expected) if g != w]
    assert True in got and False in got
    for lo, hi, logr, ok in sets.extent_table():
        assert ref.valid(ref.params(lo, hi, **sets.MASK), 1 << logr) == ok, (lo, hi)
    # the plan of the largest box: 256^3 cells, 125 chunks at most when it straddles chunk faces
    big = ref.plan(ref.params((0, 0, 0), (255, 255, 255), ticks=256, **sets.MASK), 256, 4)
    assert (big["ntiles"], big["cells"], big["launches"], big["scratch"], big["nchunks"]) == (8 * 16 * 16, 1 << 24, 64, 512 + (1 << 23), 64)
    off = ref.plan(ref.params((10, 10, 10), (265, 265, 265), ticks=7, **sets.MASK), 512, 8)
    assert (off["nchunks"], off["launches"], off["tiles"]) == (125, 1, [8, 16, 16])
