"""The contract of rt_detach_voxels as the two restatements of tests/detach_voxels_ref.py state it — no device.  On every case of
tests/detach_voxels_sets.py the global flood fill and the chunk-pass process give the same supported set; the counts, bounds and dirty
chunks are what the cases' names say; a carve equals tests/voxel_edits.py with one record per detached voxel; a pass limit below the
pass count reports unconverged and changes nothing."""
import numpy as np
import pytest

from tests import detach_voxels_ref as ref
from tests import detach_voxels_sets as sets
from tests import voxel_edits as ve

CASES = sets.cases()


def _sets_of(case):
    mats, mine = sets.case_world(case)
    bb = ref.clipped_box(case["p"], sets.R)
    occ, anc = ref.occupancy_and_anchors(mats, mine, case["p"], bb)
    return mats, mine, bb, occ, anc


@pytest.mark.parametrize("name", list(CASES))
def test_the_flood_fill_and_the_chunk_passes_give_the_same_set(name):
    case = CASES[name]
    mats, mine, bb, occ, anc = _sets_of(case)
    flood = ref.supported_flood(occ, anc)
    passes, p = ref.supported_passes(occ, anc, bb)
    assert passes is not None and np.array_equal(flood, passes), name
    assert not (flood & ~occ).any() and (flood & anc).sum() == anc.sum()
    # one more definition of the pass count's lower end: a box inside one chunk ends with pass 1 or 2
    if len(ref.box_chunks(bb)) == 1:
        assert p == (1 if np.array_equal(flood, anc) else 2)
    res, stamp, dirty = ref.detach(mats.copy(), mine.copy(), case["p"])
    res_f, stamp_f, dirty_f = ref.detach(mats.copy(), mine.copy(), case["p"], supported=ref.by_flood)
    assert res.tobytes() == res_f.tobytes() and dirty == dirty_f and all(np.array_equal(a, b) for a, b in zip(stamp, stamp_f))
    print(name, res, dirty)
    for key, want in case["expect"].items():
        assert int(res[key]) == want, (name, key, int(res[key]), want)
    det = occ & ~flood
    assert int(res["detached"]) == det.sum() and int(res["supported"]) == flood.sum() and int(res["detached"]) + int(res["supported"]) == occ.sum()
    if det.any():
        z, y, x = np.nonzero(det)
        lo = [int(v.min()) + int(bb[0][k]) for k, v in enumerate((x, y, z))]
        hi = [int(v.max()) + int(bb[0][k]) for k, v in enumerate((x, y, z))]
        assert res["lo"].tolist() == lo and res["hi"].tolist() == hi
        assert len(dirty) == int(res["chunks"]) >= 1 and set(dirty) <= set(ref.box_chunks(bb))
    else:
        assert res["lo"].tolist() == [ref.INT32_MAX] * 3 and res["hi"].tolist() == [ref.INT32_MIN] * 3 and dirty == []


def test_the_cases_cover_what_their_names_say():
    assert int(ref.detach(*sets.case_world(CASES["re-enters a chunk twice"]), CASES["re-enters a chunk twice"]["p"])[0]["passes"]) >= 4
    _, _, bb, occ, anc = _sets_of(CASES["random 40 % over eight chunks"])
    sup = ref.supported_flood(occ, anc)
    assert len(ref.box_chunks(bb)) == 8 and 0.3 < occ.mean() < 0.5 and (occ & ~sup).sum() > 1000 and sup.sum() > 10000
    # the corner and the edge: the free body does touch the anchored one, diagonally only
    for name in ("touch at a corner", "touch along an edge"):
        v = np.asarray(CASES[name]["voxels"])[:, :3]
        a, b = v[:16], v[16:]
        d = np.abs(a[:, None, :] - b[None, :, :])
        assert d.max(axis=2).min() == 1 and d.sum(axis=2).min() >= 2


@pytest.mark.parametrize("name", ["inside one chunk off the word grid", "straddles three faces", "random 40 % over eight chunks", "outside the region"])
def test_a_carve_equals_one_voxel_edit_per_detached_voxel_and_the_stamp_holds_them(name):
    case = CASES[name]
    mats0, mine0, bb, occ, anc = _sets_of(case)
    det = occ & ~ref.supported_flood(occ, anc)
    z, y, x = np.nonzero(det)
    xyz = np.stack([x + int(bb[0][0]), y + int(bb[0][1]), z + int(bb[0][2])], axis=1)
    want_m, want_f = mats0.copy(), mine0.copy()
    touched = ve.apply_edits(want_m, want_f, xyz, np.full(len(xyz), sets.AIR, np.uint32), np.zeros(len(xyz), bool))
    for flags in (ref.CARVE, ref.CARVE | ref.CAPTURE, ref.CAPTURE, 0):
        mats, mine = mats0.copy(), mine0.copy()
        res, stamp, dirty = ref.detach(mats, mine, ref.with_(case["p"], flags=flags | (int(case["p"]["flags"]) & ref.ANCHOR_MATERIAL)))
        changed = flags & ref.CARVE
        assert np.array_equal(mats, want_m if changed else mats0) and np.array_equal(mine, want_f if changed else mine0)
        assert dirty == sorted(touched) and int(res["chunks"]) == len(touched)
        assert (stamp is not None) == bool(flags & ref.CAPTURE)
        if stamp is not None:
            sl = ref.box_slices(bb)
            assert stamp[0].shape == occ.shape and np.array_equal(stamp[1] == ref.SOLID, det) and np.array_equal(stamp[1] != ref.ABSENT, det)
            assert np.array_equal(stamp[0][det], mats0[sl][det]) and not stamp[0][~det].any()


def test_a_pass_limit_below_the_pass_count_is_unconverged_and_changes_nothing():
    case = CASES["re-enters a chunk twice"]
    mats0, mine0 = sets.case_world(case)
    start = ref.result0(5, 6, 0xFFFFFFFE, 0xFFFFFFFF, (1, 2, 3), 9, (4, 5, 6))
    full, _, _ = ref.detach(mats0.copy(), mine0.copy(), case["p"], start)
    n = (int(full["passes"]) - int(start["passes"])) & 0xFFFFFFFF
    assert n == case["expect"]["passes"] and int(full["unconverged"]) == 0xFFFFFFFF
    mats, mine = mats0.copy(), mine0.copy()
    exact, _, _ = ref.detach(mats, mine, ref.with_(case["p"], max_passes=n), start)
    assert exact.tobytes() == full.tobytes()
    mats, mine = mats0.copy(), mine0.copy()
    res, stamp, dirty = ref.detach(mats, mine, ref.with_(case["p"], max_passes=n - 1), start)
    assert np.array_equal(mats, mats0) and np.array_equal(mine, mine0) and dirty == []
    assert (int(res["passes"]), int(res["unconverged"])) == ((0xFFFFFFFE + n - 1) & 0xFFFFFFFF, 0)          # both wrap
    assert [int(res[k]) for k in ("detached", "supported", "chunks")] == [5, 6, 9] and res["lo"].tolist() == [1, 2, 3] and res["hi"].tolist() == [4, 5, 6]
    assert not stamp[0].any() and not stamp[1].any()


def test_the_result_is_added_to_and_merged():
    case = CASES["inside one chunk off the word grid"]
    mats, mine = sets.case_world(case)
    plain, _, _ = ref.detach(mats.copy(), mine.copy(), case["p"])
    start = ref.result0(0xFFFFFFF0, 7, 3, 1, (0, 200, 140), 0xFFFFFFFF, (10, 300, 149), 77)
    res, _, _ = ref.detach(mats.copy(), mine.copy(), case["p"], start)
    assert int(res["detached"]) == (0xFFFFFFF0 + int(plain["detached"])) & 0xFFFFFFFF and int(res["supported"]) == 7 + int(plain["supported"])
    assert int(res["chunks"]) == int(plain["chunks"]) - 1 and int(res["passes"]) == 3 + int(plain["passes"]) and int(res["unconverged"]) == 1
    assert res["lo"].tolist() == [0, int(plain["lo"][1]), 140] and res["hi"].tolist() == [int(plain["hi"][0]), 300, int(plain["hi"][2])]
    assert int(res["reserved"]) == 77


def test_an_empty_clipped_box_does_nothing():
    mats, mine = sets.world()
    res, stamp, dirty = ref.detach(mats, mine, sets.EMPTY_BOX, ref.result0(1, 2, 3, 4))
    assert res.tobytes() == ref.result0(1, 2, 3, 4).tobytes() and stamp is None and dirty == []


def test_the_parameter_table_and_the_extent_rows():
    table, expected, names = sets.params_table()
    for row, ok, name in zip(table, expected, names):
        assert ref.valid(row, sets.R) == bool(ok), name
    assert not ref.valid(table[names.index("plain")], sets.R, stamp_out=False)
    assert ref.valid(table[names.index("a query")], sets.R, stamp_out=False)
    for row, ok in sets.EXTENT_ROWS:
        assert ref.valid(row, 512) == ok
