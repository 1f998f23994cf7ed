"""The rules of rt_settle_voxels without a GPU, in the restatements alone: the closed form (tests/settle_voxels_ref.py `settle`) and
the sweeps (`settle_naive`) agree on every case and on every axis and direction, each named case of tests/settle_voxels_sets.py moves
what its name says, T calls with max_fall = 1 equal one with max_fall = T, a second unlimited call moves nothing, vacated cells hold
air_material while refilled cells hold the arriving word and untouched air keeps its own, nothing outside the box changes but the
minefield of the dirty chunks, and the parameter table's verdicts."""
import numpy as np
import pytest

from tests import adversarial_worlds as aw
from tests import settle_voxels_ref as ref
from tests import settle_voxels_sets as sets

R = 256
CASES = sets.cases()
ALL = dict(CASES, **{"fixture axis %d toward %d" % at: sets.fixture_case(*at) for at in sets.AXES})


def _counts(c):
    return dict((k, int(c[k])) for k in ("moved", "falling", "distance", "chunks"))


@pytest.fixture(scope="module")
def runs():
    """Per case: the world before, the world after `settle`, its counts and touched chunks, and `settle_naive`'s answer — computed once."""
    out = {}
    for name, case in ALL.items():
        mats0, mine0 = sets.case_world(case)
        mats, mine = mats0.copy(), mine0.copy()
        cnt, touched = ref.settle(mats, mine, case["p"])
        out[name] = dict(before=(mats0, mine0), after=(mats, mine), counts=_counts(cnt), touched=touched, naive=ref.settle_naive(mats0, mine0, case["p"]))
    return out


@pytest.mark.parametrize("name", list(ALL))
def test_the_closed_form_and_the_sweeps_agree(name, runs):
    r, p = runs[name], ALL[name]["p"]
    occ, words, counts, dirty = r["naive"]
    sl = ref.box_slices(ref.clipped_box(p, R))
    mats, mine = r["after"]
    assert np.array_equal(mine[sl] == 0, occ) and np.array_equal(mats[sl], words)
    assert r["counts"] == counts and r["touched"] == dirty


@pytest.mark.parametrize("name", list(CASES))
def test_a_case_moves_what_its_name_says(name, runs):
    if CASES[name]["expect"]:
        assert runs[name]["counts"] == CASES[name]["expect"]
    else:
        assert runs[name]["counts"]["moved"] > 1000 and runs[name]["counts"]["falling"] > 0     # the random case: checked against the sweeps


@pytest.mark.parametrize("name", list(ALL))
def test_only_the_box_and_the_dirty_chunks_minefield_change(name, runs):
    r, p = runs[name], ALL[name]["p"]
    (mats0, mine0), (mats, mine) = r["before"], r["after"]
    sl = ref.box_slices(ref.clipped_box(p, R))
    outside = np.ones(mine.shape, bool)
    outside[sl] = False
    assert np.array_equal(mats[outside], mats0[outside])
    assert np.array_equal((mine == 0)[outside], (mine0 == 0)[outside])
    clean = np.ones(mine.shape, bool)
    for cx, cy, cz in r["touched"]:
        clean[64 * cz:64 * cz + 64, 64 * cy:64 * cy + 64, 64 * cx:64 * cx + 64] = False
    assert np.array_equal(mine[clean], mine0[clean])
    assert ((mine == 0) & sl_mask(sl, mine.shape)).sum() == ((mine0 == 0) & sl_mask(sl, mine.shape)).sum()    # no voxel is lost or made


def sl_mask(sl, shape):
    m = np.zeros(shape, bool)
    m[sl] = True
    return m


def test_the_named_voxels_land_where_the_rules_say(runs):
    mats, mine = runs["stack unlimited"]["after"]
    assert [int(w) & 0xFF for w in mats[132:137, 70, 70]] == [0, 1, 2, 3, 4] and (mine[132:137, 70, 70] == 0).all() and (mine[137:146, 70, 70] != 0).all()
    mats, mine = runs["stack fall 1"]["after"]
    assert np.nonzero(mine[132:146, 70, 70] == 0)[0].tolist() == [1, 2, 5, 8, 9]
    mats, mine = runs["stack fall 3"]["after"]
    assert np.nonzero(mine[132:146, 70, 70] == 0)[0].tolist() == [0, 1, 3, 6, 7]
    mats, mine = runs["split by a fixed voxel"]["after"]
    assert np.nonzero(mine[132:146, 70, 70] == 0)[0].tolist() == [0, 4, 5, 6, 7] and mats[136, 70, 70] == sets.FIXED | 8
    mats, mine = runs["onto texel 0"]["after"]
    assert mine[140, 70, 0] == 0 and mats[140, 70, 0] == sets.LOOSE and mine[140, 70, 5] != 0
    mats, mine = runs["outside the region"]["after"]
    assert mine[255, 66, 3] == 0 and mine[254, 66, 3] == 0 and mine[253, 68, 0] == 0 and (mine[248:253, 64:71, 0:11] != 0).all()
    # the chunk boundary: a voxel leaves chunk z = 1 for chunk z = 0, its neighbour stays in chunk z = 1
    (mats0, mine0), (mats, mine) = runs["chunk boundary"]["before"], runs["chunk boundary"]["after"]
    assert runs["chunk boundary"]["touched"] == [(1, 1, 0), (1, 1, 1)]
    assert (mine[60:62, 101, 101] == 0).all() and (mine[62:71, 101, 101] != 0).all() and mine[67, 101, 102] == 0 and mine[70, 101, 102] != 0
    # the columns beside a box one column wide stay in the air
    (mats0, mine0), (mats, mine) = runs["one column"]["before"], runs["one column"]["after"]
    assert mine[132, 70, 71] == 0 and mine[140, 70, 71] != 0
    for x, y in ((70, 70), (72, 70), (71, 71)):
        assert mine[140, y, x] == 0 and np.array_equal(mine0[:, y, x] == 0, mine[:, y, x] == 0)


def test_vacated_cells_hold_air_material_refilled_cells_the_arriving_word_and_air_keeps_its_own(runs):
    (mats0, mine0), (mats, mine) = runs["stack falls by less than its height"]["before"], runs["stack falls by less than its height"]["after"]
    col, col0 = mats[132:146, 70, 70], mats0[132:146, 70, 70]
    assert [int(w) for w in col[0:4]] == [sets.LOOSE | i for i in range(4)]          # 134 and 135 were vacated and refilled
    assert [int(w) for w in col[4:6]] == [sets.AIR, sets.AIR]                          # 136 and 137 were vacated for good
    assert np.array_equal(col[6:], col0[6:]) and not (col0[6:] == sets.AIR).any()      # air that stays air keeps its own word
    assert (mine[132:136, 70, 70] == 0).all() and (mine[136:146, 70, 70] != 0).all()


def test_the_mask_selects_and_0_0_takes_every_occupied_voxel(runs):
    a, b = runs["split by a fixed voxel"], runs["split, every voxel loose"]
    assert a["counts"]["moved"] == 3 and b["counts"]["moved"] == 5
    assert b["after"][0][133, 70, 70] == sets.FIXED | 8                                # the fixed voxel fell with the rest, second from below
    assert np.nonzero(b["after"][1][132:146, 70, 70] == 0)[0].tolist() == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("name", ["stack unlimited", "split by a fixed voxel", "random 64 x 64", "fixture axis 1 toward 1"])
def test_t_calls_with_max_fall_1_equal_one_call_with_max_fall_t(name):
    case = ALL[name]
    for T in (1, 2, 5):
        mats, mine = sets.case_world(case)
        cnt, _ = ref.settle(mats, mine, ref.with_(case["p"], max_fall=T))
        m1, f1 = sets.case_world(case)
        c1 = None
        for _ in range(T):
            falling_before = 0 if c1 is None else int(c1["falling"])
            c1, _ = ref.settle(m1, f1, ref.with_(case["p"], max_fall=1), c1)
        # the same voxels in the same cells with the same minefield; the word of an unoccupied cell is its own or air_material either
        # way (the single steps leave air_material in every cell a voxel passed, the one call in the cells voxels started from)
        mats0, _ = sets.case_world(case)
        occ = mine == 0
        assert np.array_equal(mine, f1) and np.array_equal(mats[occ], m1[occ])
        for m in (mats, m1):
            assert ((m == mats0) | (m == sets.AIR))[~occ].all()
        assert int(c1["moved"]) >= int(cnt["moved"]) and int(c1["distance"]) == int(cnt["distance"])
        assert int(c1["falling"]) - falling_before == int(cnt["falling"])                # the last call's own answer


@pytest.mark.parametrize("name", list(ALL))
def test_a_second_unlimited_call_moves_nothing(name):
    case = ALL[name]
    mats, mine = sets.case_world(case)
    p = ref.with_(case["p"], max_fall=ref.UNLIMITED)
    cnt, _ = ref.settle(mats, mine, p)
    assert int(cnt["falling"]) == 0
    m2, f2 = mats.copy(), mine.copy()
    cnt2, touched = ref.settle(m2, f2, p)
    assert _counts(cnt2) == dict(moved=0, falling=0, distance=0, chunks=0) and touched == []
    assert np.array_equal(m2, mats) and np.array_equal(f2, mine)


def test_the_order_inside_a_column_is_kept_and_targets_are_distinct():
    case = CASES["random 64 x 64"]
    mats, mine = sets.case_world(case)
    m = ref.moves(mats, mine, case["p"])
    assert len(set(map(tuple, m["dst"].tolist()))) == len(m["dst"])
    key = m["src"][:, 0] * 1024 + m["src"][:, 1]
    for k in np.unique(key)[:200]:
        s, d = m["src"][key == k, 2], m["dst"][key == k, 2]
        assert (np.argsort(s) == np.argsort(d)).all()


def test_the_eight_chunk_world_moves_voxels_in_two_chunks_only():
    mats, mine, _, _ = aw.arbitrary_world(256, seed=1)
    mats, p = sets.eight_chunks_world(mats, mine)
    mine = mine.copy()
    mine0 = mine.copy()
    assert mine0.max() > 6
    cnt, touched = ref.settle(mats, mine, p)
    # (a voxel of chunk (1, 1, 1) may fall on into (1, 1, 0); the other five chunks hold no loose voxel)
    assert {(0, 0, 0), (1, 1, 1)} <= set(touched) <= {(0, 0, 0), (1, 1, 1), (1, 1, 0)} and int(cnt["chunks"]) == len(touched) and int(cnt["moved"]) >= 8
    assert mine[:64, :64, :64].max() <= 6 and mine[64:128, 64:128, 64:128].max() <= 6 and np.array_equal(mine[:64, :64, 64:128], mine0[:64, :64, 64:128])


def test_counts_wrap_and_an_empty_box_changes_nothing():
    case = CASES["stack unlimited"]
    mats, mine = sets.case_world(case)
    cnt, _ = ref.settle(mats, mine, case["p"], (0xFFFFFFFE, 7, 0xFFFFFFF0, 0xFFFFFFFF))
    assert _counts(cnt) == dict(moved=3, falling=7, distance=4, chunks=0)
    mats0, mine0 = mats.copy(), mine.copy()
    cnt, touched = ref.settle(mats, mine, ref.params((300, 10, 10), (310, 20, 20)), (1, 2, 3, 4))
    assert _counts(cnt) == dict(moved=1, falling=2, distance=3, chunks=4) and touched == [] and np.array_equal(mats, mats0) and np.array_equal(mine, mine0)


def test_the_parameter_table_has_the_verdicts_its_names_promise():
    table, expected, names = sets.params_table()
    got = [ref.valid(p, R) for p in table]
    assert got == expected.tolist(), [n for n, g, w in zip(names, got, expected) if g != w]
    assert len(set(names)) == len(names) and not all(got) and any(got)
    assert ref.clipped_box(table[names.index("box beyond the region")], R) is None
    lo, hi = ref.clipped_box(table[names.index("clipped at both faces")], R)
    assert lo.tolist() == [0, 250, 100] and hi.tolist() == [3, 255, 101]
