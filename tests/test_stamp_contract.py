"""The voxel-stamp contract (include/rt_abi.h: RtStampPlace, rt_stamp_capture, rt_edit_stamps) on the CPU: tests/stamp_edits.py, the
restatement the GPU tests compare with, held against the header's per-voxel orientation rule, against tests/voxel_edits.apply_edits fed
with explicitly enumerated records — order, `where`, ABSENT, clipping, the touched chunks — and against the undo identity."""
import itertools

import numpy as np
import pytest

from tests import shape_edits as se
from tests import stamp_edits as st
from tests import voxel_edits as ve

E = (5, 3, 7)                                                          # (ex, ey, ez): three different odd extents


def _distinct(E=E):
    """A stamp whose every word is different, all SOLID."""
    ex, ey, ez = E
    return np.arange(1, ex * ey * ez + 1, dtype=np.uint32).reshape(ez, ey, ex), np.full((ez, ey, ex), st.SOLID, np.uint8)


def test_the_transpose_form_equals_the_per_voxel_rule_for_all_48():
    mats, _ = _distinct()
    for orient in range(48):
        got = st.oriented(mats, orient)
        Ep = st.placed_extent(E, orient)
        assert st.extent_of(got) == Ep == tuple(E[st.PERMS[orient >> 3][k]] for k in range(3))
        want = np.empty_like(got)
        for d in itertools.product(range(Ep[0]), range(Ep[1]), range(Ep[2])):
            s = st.source_voxel(E, orient, d)
            want[d[2], d[1], d[0]] = mats[s[2], s[1], s[0]]
        assert np.array_equal(got, want), orient


def test_48_distinct_orientations_24_rotations_and_every_inverse():
    mats, _ = _distinct()
    views = [st.oriented(mats, o) for o in range(48)]
    keys = {(v.shape, v.tobytes()) for v in views}
    assert len(keys) == 48
    assert sum(st.is_rotation(o) for o in range(48)) == 24
    # handedness by the sign of the determinant of the axis map, independently of is_rotation's parity count
    for o in range(48):
        perm, f = st.PERMS[o >> 3], o & 7
        M = np.zeros((3, 3))
        for k in range(3):
            M[perm[k], k] = -1.0 if (f >> perm[k]) & 1 else 1.0
        assert (np.linalg.det(M) > 0) == st.is_rotation(o), o
    # every orientation is undone by one of the set: turning the turned stamp gives the stamp back
    for o in range(48):
        back = [q for q in range(48) if st.oriented(views[o], q).shape == mats.shape and np.array_equal(st.oriented(views[o], q), mats)]
        assert len(back) == 1 and st.is_rotation(back[0]) == st.is_rotation(o), o


R = 256


@pytest.fixture(scope="module")
def synthetic_world():
    """Ground below a wavy surface, a few floating blobs; every chunk's minefield is pack_into's."""
    rng = np.random.default_rng(11)
    z, y, x = np.mgrid[0:R, 0:R, 0:R]
    occ = z < 100 + 20 * np.sin(x / 17.0) + 15 * np.cos(y / 23.0)
    occ |= rng.random((R, R, R)) < 0.002
    mine = np.empty((R, R, R), np.uint8)
    for c in itertools.product(range(4), repeat=3):
        sl = tuple(slice(64 * v, 64 * v + 64) for v in c)
        mine[sl] = ve.chunk_minefield(occ[sl])
    mats = rng.integers(0, 2 ** 32, size=(R, R, R), dtype=np.uint64).astype(np.uint32)
    return mats, mine


def _tree():
    """A trunk with a crown: the corners of its box are ABSENT, the crown's inside is AIR (a hollow)."""
    rng = np.random.default_rng(5)
    state = np.zeros((12, 9, 9), np.uint8)
    state[:7, 4, 4] = st.SOLID
    state[6:12, 1:8, 1:8] = st.SOLID
    state[8:10, 3:6, 3:6] = st.AIR
    mats = rng.integers(1, 2 ** 32, size=state.shape, dtype=np.uint64).astype(np.uint32)
    return mats, state


def _brute(mats, mine, stamps, places):
    """One voxel at a time through source_voxel, on whole-region occupancy; the chunk rebuild through voxel_edits."""
    occ = mine == 0
    touched = set()
    for p in places:
        sm, ss = stamps[int(p["stamp"])]
        Es = st.extent_of(ss)
        Ep = st.placed_extent(Es, int(p["orient"]))
        at = [int(v) for v in p["at"]]
        inside = [(max(at[k], 0), min(at[k] + Ep[k], R)) for k in range(3)]
        if any(a >= b for a, b in inside):
            continue
        touched |= {c for c in itertools.product(*(range(a >> 6, ((b - 1) >> 6) + 1) for a, b in inside))}
        for x, y, z in itertools.product(*(range(a, b) for a, b in inside)):
            s = st.source_voxel(Es, int(p["orient"]), (x - at[0], y - at[1], z - at[2]))
            state = ss[s[2], s[1], s[0]]
            if state == st.ABSENT or (p["where"] == st.WHERE_SOLID and not occ[z, y, x]) or (p["where"] == st.WHERE_AIR and occ[z, y, x]):
                continue
            occ[z, y, x] = state == st.SOLID
            mats[z, y, x] = sm[s[2], s[1], s[0]]
    for (cx, cy, cz) in touched:
        sl = (slice(64 * cz, 64 * cz + 64), slice(64 * cy, 64 * cy + 64), slice(64 * cx, 64 * cx + 64))
        mine[sl] = ve.chunk_minefield(occ[sl])
    return sorted(touched)


def test_clipping_where_absent_and_last_wins_against_the_per_voxel_model(synthetic_world):
    stamps = {7: _tree(), 9: _distinct(), 11: (np.full((3, 4, 70), 0xABC, np.uint32), np.full((3, 4, 70), st.AIR, np.uint8))}
    places = st.batch([
        st.place(7, (60, 60, 100), 0, st.WHERE_AIR),                   # a tree on the ground, across a chunk corner
        st.place(7, (62, 61, 101), 13, st.WHERE_ALL),                  # overlapping it, turned: the last wins
        st.place(9, (-2, 254, 90), 29, st.WHERE_SOLID),                # clipped at x = 0 and y = R, paint
        st.place(9, (252, 10, 253), 47),                               # clipped at x = R and z = R
        st.place(11, (30, 100, 95), 2 << 3 | 3),                           # an AIR bar of 70 along y, mirrored: a carve
        st.place(9, (256, 0, 0), 0), st.place(9, (-5, 0, 0), 0), st.place(7, (0, 0, -1024), 5),   # wholly outside
    ])
    m1, f1 = (a.copy() for a in synthetic_world)
    m2, f2 = (a.copy() for a in synthetic_world)
    t1 = st.apply_stamps(m1, f1, stamps, places)
    t2 = _brute(m2, f2, stamps, places)
    assert t1 == t2 and len(t1) == 4 + 1 + 1 + 1           # (the bar's two chunks: one is the trees')
    assert np.array_equal(f1, f2) and np.array_equal(m1, m2) and not np.array_equal(f1, synthetic_world[1])
    boxes = st.pending_boxes(stamps, places, R)
    assert len(boxes) == 5 and boxes[2][0].tolist() == [0, 254, 90] and boxes[2][1].tolist() == [0, 255, 94]        # E' of p = 3 is (ey, ez, ex) = (3, 7, 5)
    assert boxes[4][0].tolist() == [30, 100, 95] and boxes[4][1].tolist() == [33, 169, 97]       # E' of p = 2 is (ey, ex, ez) = (4, 70, 3)
    # ABSENT: the corner of the first tree's box kept the world's word and occupancy
    assert m1[100, 60, 60] == synthetic_world[0][100, 60, 60]


def test_a_placement_that_selects_nothing_still_rebuilds_its_chunk():
    rng = np.random.default_rng(3)
    mine = rng.integers(0, 31, size=(64, 64, 64), dtype=np.uint8)      # arbitrary values: not pack_into's
    mats = np.zeros((64, 64, 64), np.uint32)
    stamps = {1: (np.zeros((2, 2, 2), np.uint32), np.zeros((2, 2, 2), np.uint8))}              # all ABSENT
    f2, m2 = mine.copy(), mats.copy()
    assert st.apply_stamps(m2, f2, stamps, st.batch([st.place(1, (5, 5, 5))])) == [(0, 0, 0)]
    assert np.array_equal(f2, ve.chunk_minefield(mine == 0)) and not np.array_equal(f2, mine) and np.array_equal(m2, mats)


def test_stamps_equal_the_enumerated_voxel_edits(synthetic_world):
    stamps = {7: _tree(), 9: _distinct()}
    places = st.batch([st.place(7, (100, 100, 100), 21, st.WHERE_AIR), st.place(9, (126, 62, 190), 44), st.place(7, (103, 98, 99), 2, st.WHERE_SOLID),
                       st.place(9, (-1, -1, 60), 17)])
    xyz, words, solid, touched = st.enumerate_records(*synthetic_world, stamps, places)
    assert sorted(set(map(tuple, (xyz >> 6).tolist()))) == touched             # every touched chunk holds a selected voxel
    m1, f1 = (a.copy() for a in synthetic_world)
    m2, f2 = (a.copy() for a in synthetic_world)
    assert st.apply_stamps(m1, f1, stamps, places) == touched
    ve.apply_edits(m2, f2, xyz, words, solid)
    assert np.array_equal(f1, f2) and np.array_equal(m1, m2)


def test_undo_on_a_piece_of_the_generated_world(procedural_region):
    """Capture, change by shapes, voxel edits and stamps, paste back: the 128^3 piece is what it was, minefield included (the
    generated world is pack_into's own)."""
    gm, gf = procedural_region
    piece = None
    for z0, y0, x0 in itertools.product((64, 0, 128), repeat=3):
        f = gf[z0:z0 + 128, y0:y0 + 128, x0:x0 + 128]
        if 0.1 < np.count_nonzero(f == 0) / f.size < 0.9:
            piece = (slice(z0, z0 + 128), slice(y0, y0 + 128), slice(x0, x0 + 128))
            break
    assert piece is not None
    mats, mine = gm[piece].copy(), gf[piece].copy()
    before = mats.copy(), mine.copy()
    lo, ext = (20, 30, 40), (80, 70, 60)
    saved = st.capture(mats, mine, lo, ext)
    assert set(np.unique(saved[1]).tolist()) == {st.AIR, st.SOLID}
    skip = st.capture(mats, mine, lo, ext, st.SKIP_AIR)
    assert np.array_equal(skip[1] == st.SOLID, saved[1] == st.SOLID) and not (skip[1] == st.AIR).any() and not skip[0][skip[1] == st.ABSENT].any()
    se.apply_shapes(mats, mine, se.batch([se.sphere((120, 130, 140), 50 * 50, 0, 0), se.box((25, 35, 45), (60, 60, 60), 0x77, 1)]))
    xyz = np.stack(np.meshgrid(np.arange(20, 100, 3), np.arange(30, 100, 3), np.arange(40, 100, 3), indexing="ij"), axis=-1).reshape(-1, 3)
    ve.apply_edits(mats, mine, xyz, np.full(len(xyz), 0x99, np.uint32), (xyz.sum(axis=1) & 1) == 0)
    st.apply_stamps(mats, mine, {1: _tree()}, st.batch([st.place(1, (50, 50, 70), 9)]))
    inside = tuple(slice(lo[k], lo[k] + ext[k]) for k in (2, 1, 0))
    assert not np.array_equal(mats[inside], before[0][inside]) and not np.array_equal(mine == 0, before[1] == 0)
    st.apply_stamps(mats, mine, {2: saved}, st.batch([st.place(2, lo)]))
    assert np.array_equal(mats, before[0]) and np.array_equal(mine, before[1])


def test_validity_verdicts():
    ids = {5}
    good = st.place(5, (1, 2, 3), 47, st.WHERE_AIR)
    assert st.valid(good, R, ids)

    def spoil(**kw):
        p = good.copy()
        for k, v in kw.items():
            p[k] = v
        return p
    for bad in (spoil(stamp=6), spoil(stamp=0), spoil(orient=48), spoil(where=3), spoil(reserved0=(0, 1)), spoil(reserved=(0, 0, 1)),
                spoil(at=(4 * R + 1, 0, 0)), spoil(at=(0, -4 * R - 1, 0))):
        assert not st.valid(bad, R, ids)
    assert st.valid(spoil(at=(4 * R, -4 * R, 0)), R, ids)
    assert st.bounding_box(spoil(at=(4 * R, 0, 0)), E, R) is None and st.bounding_box(spoil(at=(-5, 0, 0), orient=0), E, R) is None
    lo, hi = st.bounding_box(spoil(at=(-4, 0, 0), orient=0), E, R)
    assert lo.tolist() == [0, 0, 0] and hi.tolist() == [0, 2, 6]
