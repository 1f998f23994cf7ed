"""The rt_edit_shapes contract (include/rt_abi.h) on the CPU: tests/shape_edits.py, the restatement the GPU tests compare with, held
against tests/voxel_edits.apply_edits fed with explicitly enumerated records — order, `where`, clipping, the bounding box and the
touched chunks — on a synthetic 256^3 world built with chunk_minefield."""
import numpy as np
import pytest

from tests import shape_edits as se
from tests import voxel_edits as ve

R = 256


@pytest.fixture(scope="module")
def synthetic_world():
    """Ground below a wavy surface, a few floating blobs; every chunk's minefield is pack_into's."""
    rng = np.random.default_rng(7)
    z, y, x = np.mgrid[0:R, 0:R, 0:R]
    occ = z < 100 + 20 * np.sin(x / 17.0) + 15 * np.cos(y / 23.0)
    occ |= rng.random((R, R, R)) < 0.002
    mine = np.empty((R, R, R), np.uint8)
    for cz in range(4):
        for cy in range(4):
            for cx in range(4):
                sl = (slice(64 * cz, 64 * cz + 64), slice(64 * cy, 64 * cy + 64), slice(64 * cx, 64 * cx + 64))
                mine[sl] = ve.chunk_minefield(occ[sl])
    mats = rng.integers(0, 2 ** 32, size=(R, R, R), dtype=np.uint64).astype(np.uint32)
    return mats, mine


def _brute(shape, occ):
    """Every row of the region, one formula at a time in Python integers; numpy only along x."""
    a, b = [int(v) for v in shape["a"]], [int(v) for v in shape["b"]]
    x = np.arange(R, dtype=np.int64)
    out = np.zeros((R, R, R), bool)
    for zz in range(R):
        for yy in range(R):
            if shape["kind"] == se.BOX:
                if not (a[1] <= yy <= b[1] and a[2] <= zz <= b[2]):
                    continue
                m = (a[0] <= x) & (x <= b[0])
            else:
                rest = b[0] - (2 * yy + 1 - a[1]) ** 2 - (2 * zz + 1 - a[2]) ** 2
                if rest < 0:
                    continue
                m = (2 * x + 1 - a[0]) ** 2 <= rest
            if shape["where"] == se.SOLID:
                m = m & occ[zz, yy]
            elif shape["where"] == se.AIR:
                m = m & ~occ[zz, yy]
            out[zz, yy] = m
    return out


SHAPES = [
    se.sphere((21, 21, 21), 49, 5),                                   # radius 3.5 round voxel (10, 10, 10)
    se.sphere((256, 256, 200), 31 * 31, 6, solid=0),                  # centred on a chunk corner, in the ground: a carve
    se.sphere((-9, 255, 190), 40 * 40, 7, where=se.AIR),              # centred outside, clipped at x = 0
    se.box((250, 250, 90), (300, 258, 130), 8, where=se.SOLID),       # reaches past x = 255
    se.box((-1024, -1024, -1024), (-1, 1024, 1024), 9),               # wholly outside
    se.sphere((41, 41, 41), 0, 10),                                   # one voxel
    se.sphere((40, 41, 41), 0, 11),                                   # none
]


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_selected_is_the_formula_voxel_by_voxel(synthetic_world, k):
    occ = synthetic_world[1] == 0
    assert np.array_equal(se.selected(SHAPES[k], R, occ), _brute(SHAPES[k], occ))


def test_the_examples_of_the_header():
    lo, hi = se.bounding_box(SHAPES[0], R)
    assert lo.tolist() == [7, 7, 7] and hi.tolist() == [13, 13, 13]
    occ = np.zeros((R, R, R), bool)
    sel = se.selected(SHAPES[0], R, occ)
    assert sel[10, 10, 13] and sel[10, 13, 10] and not sel[10, 12, 13] and sel.sum() == 179      # |d| <= 3.5 on the integer grid
    assert se.selected(SHAPES[5], R, occ).sum() == 1 and se.selected(SHAPES[5], R, occ)[20, 20, 20]
    assert se.bounding_box(SHAPES[6], R) is None and se.bounding_box(SHAPES[4], R) is None
    lo, hi = se.bounding_box(SHAPES[3], R)
    assert lo.tolist() == [250, 250, 90] and hi.tolist() == [255, 255, 130]
    lo, hi = se.bounding_box(SHAPES[2], R)
    assert lo.tolist() == [0, 107, 75] and hi.tolist() == [15, 147, 114]


def test_verdicts():
    good = [se.box((-4 * R, 0, 0), (4 * R, 0, 0)), se.sphere((4 * R, -4 * R, 0), 2 ** 26), se.sphere((0, 0, 0), 0)]
    bad = [se.box((-4 * R - 1, 0, 0), (0, 0, 0)), se.box((0, 0, 0), (0, 4 * R + 1, 0)), se.box((0, 0, 5), (0, 0, 4)),
           se.sphere((0, 0, 4 * R + 1), 4), se.sphere((0, 0, 0), -1), se.sphere((0, 0, 0), 2 ** 26 + 1), se.sphere((0, 0, 0), 4, reserved=1)]
    s = se.sphere((0, 0, 0), 4)
    s["b"] = (4, 0, 1)
    bad.append(s)
    s = se.box((0, 0, 0), (1, 1, 1))
    s["kind"] = 2
    bad.append(s)
    s = se.box((0, 0, 0), (1, 1, 1))
    s["where"] = 3
    bad.append(s)
    assert all(se.valid(g, R) for g in good) and not any(se.valid(b, R) for b in bad)


def _against_records(world, shapes):
    mats, mine = world
    m1, f1 = mats.copy(), mine.copy()
    touched = se.apply_shapes(m1, f1, shapes)
    xyz, words, solid, touched2 = se.enumerate_records(mats, mine, shapes)
    m2, f2 = mats.copy(), mine.copy()
    edited = ve.apply_edits(m2, f2, xyz, words, solid)
    assert touched == touched2 and set(edited) <= set(touched)
    # (the world is pack_into's own, so a touched chunk without a selected voxel is rebuilt into the bytes it had)
    assert np.array_equal(f1, f2) and np.array_equal(m1, m2)
    return (m1, f1), touched, edited


def test_order_where_and_clipping_equal_enumerated_records(synthetic_world):
    lo, hi = (100, 100, 80), (140, 130, 120)
    shapes = se.batch([se.box(lo, hi, 1, where=se.AIR), se.box(lo, hi, 2, where=se.SOLID), se.box((110, 110, 90), (130, 120, 110), 0, solid=0),
                       se.box((110, 110, 90), (130, 120, 110), 3, solid=0, where=se.SOLID),   # nothing is solid there any more
                       SHAPES[1], SHAPES[2], SHAPES[3], SHAPES[4], SHAPES[6]])
    (m, f), touched, edited = _against_records(synthetic_world, shapes)
    assert (m[81:120, 100:131, 100:110] == 2).all() and (f[81:120, 100:131, 100:110] == 0).all()   # filled, then painted
    assert (f[90:111, 110:121, 110:112] != 0).all() and (m[90:111, 110:121, 110:112] == 0).all()   # carved; the fourth shape found nothing
    assert (1, 1, 1) in touched and len(touched) == 8 and len(edited) >= 6
    assert not np.array_equal(f, synthetic_world[1])


def test_the_last_shape_wins(synthetic_world):
    shapes = se.batch([se.box((60, 60, 60), (70, 70, 70), 1), se.box((65, 65, 65), (75, 75, 75), 2, solid=0), se.sphere((131, 131, 131), 36, 3)])
    (m, f), touched, _ = _against_records(synthetic_world, shapes)
    assert m[62, 62, 62] == 1 and m[70, 70, 70] == 2 and f[70, 70, 70] != 0 and m[65, 65, 65] == 3 and f[65, 65, 65] == 0
    assert len(touched) == 8


def test_a_touched_chunk_without_a_selected_voxel_is_rebuilt():
    """On arbitrary minefield values the rebuild shows: the chunk round an even-centred empty sphere becomes pack_into's, the
    others keep their bytes; a shape outside the region touches nothing."""
    rng = np.random.default_rng(3)
    mine = rng.integers(0, 31, size=(R, R, R), dtype=np.uint8)
    mats = rng.integers(0, 2 ** 32, size=(R, R, R), dtype=np.uint64).astype(np.uint32)
    m1, f1 = mats.copy(), mine.copy()
    assert se.apply_shapes(m1, f1, se.batch([se.sphere((300, 300, 300), 1, 9), SHAPES[4], SHAPES[6]])) == [(2, 2, 2)]
    assert se.selected(se.sphere((300, 300, 300), 1, 9), R, mine == 0).sum() == 0      # an even centre: the 8 nearest are at 3 > 1
    sl = (slice(128, 192),) * 3
    assert np.array_equal(f1[sl], ve.chunk_minefield(mine[sl] == 0)) and not np.array_equal(f1[sl], mine[sl])
    f1[sl] = mine[sl]
    assert np.array_equal(f1, mine) and np.array_equal(m1, mats)


def test_a_sub_box_of_a_larger_region():
    """apply_shapes on the chunk row x = 64..384 of a region of 1024: the shapes' coordinates are the region's."""
    rng = np.random.default_rng(5)
    occ = rng.random((64, 64, 320)) < 0.3
    mine = np.concatenate([ve.chunk_minefield(occ[:, :, 64 * i:64 * i + 64]) for i in range(5)], axis=2)
    mats = np.zeros(mine.shape, np.uint32)
    shapes = se.batch([se.box((150, 300, 440), (230, 340, 520), 4), se.sphere((2 * 192, 2 * 352, 2 * 480), 50 * 50, 5, solid=0)])
    touched = se.apply_shapes(mats, mine, shapes, origin=(64, 320, 448), region=1024)
    assert touched == [(2, 5, 7), (3, 5, 7)]
    assert (mats[0:64, 0:21, 86:103] == 4).all() and mats[32, 32, 128] == 5 and mine[32, 32, 128] != 0
    assert (mats[:, :, :64] == 0).all() and (mats[:, :, 192:] == 0).all()


def test_pending_boxes_are_the_bounding_boxes_in_shape_order():
    got = se.pending_boxes(se.batch(SHAPES), R)
    want = [se.bounding_box(s, R) for s in SHAPES if se.bounding_box(s, R) is not None]
    assert len(got) == 5 and all(np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) for g, w in zip(got, want))
    assert got[1][0].tolist() == [112, 112, 84] and got[1][1].tolist() == [143, 143, 115]


def test_uniform_chunks_take_the_short_way_to_the_same_minefield():
    for occ in (np.ones((64, 64, 64), bool), np.zeros((64, 64, 64), bool)):
        assert np.array_equal(se._minefield(occ), ve.chunk_minefield(occ))


def test_the_binding_builds_the_restatement_s_rows():
    """render.box_shape / sphere_shape and abi.RtShapeEdit lay a shape out as the header does: 32 bytes, a at 0, material at 12, b at
    16, then kind, where, solid, reserved."""
    import ctypes as C
    from raytrace_amd import abi, render
    assert render.SHAPE_DTYPE == se.SHAPE_DTYPE and C.sizeof(abi.RtShapeEdit) == 32
    assert [getattr(abi.RtShapeEdit, f).offset for f in ("a", "material", "b", "kind", "where", "solid", "reserved")] == [0, 12, 16, 28, 29, 30, 31]
    assert (abi.RT_SHAPE_BOX, abi.RT_SHAPE_SPHERE, abi.RT_WHERE_ALL, abi.RT_WHERE_SOLID, abi.RT_WHERE_AIR) == (se.BOX, se.SPHERE, se.ALL, se.SOLID, se.AIR)
    assert render.box_shape((1, -2, 3), (4, 5, 6), 0xDEADBEEF, solid=False, where=abi.RT_WHERE_AIR).tobytes() == \
        se.box((1, -2, 3), (4, 5, 6), 0xDEADBEEF, 0, se.AIR).tobytes()
    assert render.sphere_shape((10.5, 10.5, 10.5), 3.5, 5).tobytes() == SHAPES[0].tobytes()
    assert render.sphere_shape((64, 0, -3), 0, 1, where=abi.RT_WHERE_SOLID).tobytes() == se.sphere((128, 0, -6), 0, 1, 1, se.SOLID).tobytes()
    with pytest.raises(ValueError):
        render.sphere_shape((10.25, 0, 0), 1)
