"""numpy restatement of rt_edit_shapes (include/rt_abi.h) for the shape-edit tests.  Test infrastructure.

Arrays are [z, y, x] in texel order, as everywhere else; a shape is one row of SHAPE_DTYPE (RtShapeEdit's 32 bytes).  Everything is
int64 arithmetic on whole grids: no square root, no division — a sphere's bounding box is found by testing every texel of an axis.
The rule: shapes apply in order; a selected voxel gets the shape's material and occupancy; every 64^3 chunk that meets a shape's
bounding box gets pack_into's minefield (voxel_edits.chunk_minefield) of its occupancy, where a voxel that no shape selected is
occupied iff its minefield value is 0; nothing else changes.
"""
import numpy as np

from tests import voxel_edits as ve

BOX, SPHERE = 0, 1
ALL, SOLID, AIR = 0, 1, 2
MAX_SHAPES = 4096
MAX_BOXES = 16

SHAPE_DTYPE = np.dtype([("a", "<i4", 3), ("material", "<u4"), ("b", "<i4", 3), ("kind", "u1"), ("where", "u1"), ("solid", "u1"),
                        ("reserved", "u1")])
assert SHAPE_DTYPE.itemsize == 32


def box(lo, hi, material=0, solid=1, where=ALL, reserved=0):
    s = np.zeros((), SHAPE_DTYPE)
    s["a"], s["b"], s["material"] = lo, hi, material
    s["kind"], s["where"], s["solid"], s["reserved"] = BOX, where, solid, reserved
    return s


def sphere(a, b0, material=0, solid=1, where=ALL, reserved=0):
    """`a` = twice the centre in half texels, b0 = (2 r)^2."""
    s = np.zeros((), SHAPE_DTYPE)
    s["a"], s["b"], s["material"] = a, (b0, 0, 0), material
    s["kind"], s["where"], s["solid"], s["reserved"] = SPHERE, where, solid, reserved
    return s


def batch(shapes):
    return np.array([np.asarray(s, dtype=SHAPE_DTYPE) for s in shapes], dtype=SHAPE_DTYPE).reshape(-1)


def valid(shape, R):
    """The host's verdict on one shape."""
    a, b = shape["a"].astype(np.int64), shape["b"].astype(np.int64)
    if shape["kind"] > SPHERE or shape["where"] > AIR or shape["reserved"] != 0:
        return False
    if (a < -4 * R).any() or (a > 4 * R).any():
        return False
    if shape["kind"] == BOX:
        return bool((b >= -4 * R).all() and (b <= 4 * R).all() and (a <= b).all())
    return bool(0 <= b[0] <= 2 ** 26 and b[1] == 0 and b[2] == 0)


def _axis_pass(shape, R, k):
    """bool[R]: the texels of axis k that pass that axis's own test."""
    x = np.arange(R, dtype=np.int64)
    a, b = int(shape["a"][k]), shape["b"].astype(np.int64)
    if shape["kind"] == BOX:
        return (x >= a) & (x <= b[k])
    return (2 * x + 1 - a) ** 2 <= b[0]


def bounding_box(shape, R):
    """(lo, hi) int64[3] in (x, y, z), inclusive, or None when an axis has no texel in [0, R) that passes its test."""
    lo, hi = np.zeros(3, np.int64), np.zeros(3, np.int64)
    for k in range(3):
        ok = np.flatnonzero(_axis_pass(shape, R, k))
        if ok.size == 0:
            return None
        assert ok[-1] - ok[0] + 1 == ok.size              # an interval
        lo[k], hi[k] = ok[0], ok[-1]
    return lo, hi


def _member(shape, lo, hi):
    """bool[z, y, x] over the texel box lo..hi: inside the shape."""
    z, y, x = np.meshgrid(*(np.arange(lo[k], hi[k] + 1, dtype=np.int64) for k in (2, 1, 0)), indexing="ij", sparse=True)
    a, b = shape["a"].astype(np.int64), shape["b"].astype(np.int64)
    if shape["kind"] == BOX:
        return ((x >= a[0]) & (x <= b[0])) & ((y >= a[1]) & (y <= b[1])) & ((z >= a[2]) & (z <= b[2]))
    return (2 * x + 1 - a[0]) ** 2 + (2 * y + 1 - a[1]) ** 2 + (2 * z + 1 - a[2]) ** 2 <= b[0]


def selected(shape, R, occ):
    """bool[R, R, R]: the voxels the shape selects in a region whose occupancy is `occ` (bool[R, R, R]) at that moment."""
    out = np.zeros((R, R, R), dtype=bool)
    bb = bounding_box(shape, R)
    if bb is None:
        return out
    lo, hi = bb
    sl = tuple(slice(int(lo[k]), int(hi[k]) + 1) for k in (2, 1, 0))
    m = _member(shape, lo, hi)
    if shape["where"] == SOLID:
        m = m & occ[sl]
    elif shape["where"] == AIR:
        m = m & ~occ[sl]
    out[sl] = m
    return out


def _minefield(occ):
    """voxel_edits.chunk_minefield, with the two uniform chunks answered at once (a full chunk is 0, an empty one 6)."""
    if occ.all():
        return np.zeros(occ.shape, np.uint8)
    if not occ.any():
        return np.full(occ.shape, 6, np.uint8)
    return ve.chunk_minefield(occ)


def apply_shapes(mats, mine, shapes, origin=(0, 0, 0), region=None):
    """Applies one rt_edit_shapes batch to (mats, mine) IN PLACE; returns the touched chunks as a sorted list of (cx, cy, cz).

    The arrays hold the texels from `origin` (x, y, z; multiples of 64) on of a region of edge `region` (default: the arrays are
    the region); chunks outside the arrays are not the caller's business and are left out of the result."""
    ez, ey, ex = mine.shape
    R = int(region) if region is not None else ex
    o = np.asarray(origin, dtype=np.int64)
    ext = np.array([ex, ey, ez], dtype=np.int64)
    assert (o % 64 == 0).all() and (ext % 64 == 0).all()
    occ = {}                                                          # chunk -> bool[64, 64, 64], made when a shape first meets it

    def chunk_slices(c):
        return tuple(slice(64 * c[k] - int(o[k]), 64 * c[k] - int(o[k]) + 64) for k in (2, 1, 0))

    for s in shapes:
        bb = bounding_box(s, R)
        if bb is None:
            continue
        for cz in range(int(bb[0][2]) >> 6, (int(bb[1][2]) >> 6) + 1):
            for cy in range(int(bb[0][1]) >> 6, (int(bb[1][1]) >> 6) + 1):
                for cx in range(int(bb[0][0]) >> 6, (int(bb[1][0]) >> 6) + 1):
                    c = (cx, cy, cz)
                    c0 = np.array(c, dtype=np.int64) * 64
                    if (c0 < o).any() or (c0 >= o + ext).any():
                        continue
                    if c not in occ:
                        occ[c] = mine[chunk_slices(c)] == 0
                    lo, hi = np.maximum(bb[0], c0), np.minimum(bb[1], c0 + 63)          # the box inside this chunk
                    sl = tuple(slice(int(lo[k] - c0[k]), int(hi[k] - c0[k]) + 1) for k in (2, 1, 0))
                    m = _member(s, lo, hi)
                    if s["where"] == SOLID:
                        m = m & occ[c][sl]
                    elif s["where"] == AIR:
                        m = m & ~occ[c][sl]
                    occ[c][sl][m] = s["solid"] != 0
                    mats[chunk_slices(c)][sl][m] = s["material"]
    for c in sorted(occ):
        mine[chunk_slices(c)] = _minefield(occ[c])
    return sorted(occ)


def pending_boxes(shapes, R):
    """The texel boxes (lo, hi) rt_edit_shapes records on a context with edit_radius > 0: one per shape with a bounding box."""
    out = []
    for s in shapes:
        bb = bounding_box(s, R)
        if bb is not None:
            out.append(bb)
    return out


def enumerate_records(mats, mine, shapes):
    """The batch as rt_edit_voxels rows (xyz, materials, solid) in shape order — one per selected voxel — and the chunks the shapes
    touch (sorted (cx, cy, cz)).  (mats, mine) is the whole region and is not changed."""
    R = mine.shape[0]
    occ = mine == 0
    xyz, words, solid, touched = [], [], [], set()
    for s in shapes:
        bb = bounding_box(s, R)
        if bb is None:
            continue
        lo, hi = bb
        touched |= {(cx, cy, cz) for cz in range(int(lo[2]) >> 6, (int(hi[2]) >> 6) + 1) for cy in range(int(lo[1]) >> 6, (int(hi[1]) >> 6) + 1)
                    for cx in range(int(lo[0]) >> 6, (int(hi[0]) >> 6) + 1)}
        sel = selected(s, R, occ)
        z, y, x = np.nonzero(sel)
        xyz.append(np.stack([x, y, z], axis=1))
        words.append(np.full(len(x), s["material"], np.uint32))
        solid.append(np.full(len(x), s["solid"] != 0, bool))
        occ[sel] = s["solid"] != 0
    if not xyz:
        return np.zeros((0, 3), np.int64), np.zeros(0, np.uint32), np.zeros(0, bool), sorted(touched)
    return np.concatenate(xyz), np.concatenate(words), np.concatenate(solid), sorted(touched)
