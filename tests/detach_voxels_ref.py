"""numpy restatement of rt_detach_voxels (include/rt_abi.h "Voxel detachment") for the detach tests.  Test infrastructure, written
from the rules and not from the kernels.

The box's validity and clipping are tests/shape_edits.py's (`valid`, `bounding_box`) and the world change goes through
tests/voxel_edits.py's `apply_edits`: no shape rule and no rebuild rule is restated here.  Arrays are [z, y, x] in texel order.

The rules.  A cell of the clipped box is OCCUPIED iff its minefield byte is 0.  An occupied cell is an ANCHOR iff it lies on a face of
the clipped box whose bit is set in anchor_faces (bit 2k the low face of axis k, bit 2k + 1 the high one), or — with ANCHOR_MATERIAL —
iff (material & anchor_mask) == anchor_value.  SUPPORTED is what steps between face-adjacent occupied cells of the box reach from an
anchor, DETACHED the other occupied cells.  With CARVE the detached cells become unoccupied with air_material, as rt_edit_voxels with
one solid = 0 record per detached voxel; with CAPTURE a stamp of the clipped box holds them (SOLID with their word; everything else
ABSENT with word 0).

The set is stated twice.  `supported_flood` is the plain flood fill: one step of 6-neighbour dilation masked by occupancy, repeated.
`supported_passes` is the chunk-pass process of the contract, which also yields `passes`: the box is cut by the 64^3 chunks, S_0 is the
anchors, and S_p within a chunk part is the closure inside that part of S_{p-1} and of the occupied cells that touch S_{p-1} across a
chunk face; the first p with S_p = S_{p-1} ends it.  Its closure works on one chunk part at a time and is made of whole-line sweeps (a
cell is reached along an axis iff a reached cell of its line lies before it with no unoccupied cell between), and shares nothing with
the dilation but the occupancy."""
import numpy as np

from tests import shape_edits as se
from tests import voxel_edits as ve

# numpy views of RtVoxelDetach and RtDetachResult, declared here a second time on purpose (the binding's own are
# raytrace_amd.abi.DETACH_DTYPE and DETACH_RESULT_DTYPE)
DETACH_DTYPE = np.dtype([("lo", "<i4", 3), ("flags", "<u4"), ("hi", "<i4", 3), ("air_material", "<u4"), ("anchor_mask", "<u4"), ("anchor_value", "<u4"),
                         ("max_passes", "<u4"), ("anchor_faces", "u1"), ("reserved0", "u1", 3)])
RESULT_DTYPE = np.dtype([("detached", "<u4"), ("supported", "<u4"), ("passes", "<u4"), ("unconverged", "<u4"), ("lo", "<i4", 3), ("chunks", "<u4"),
                         ("hi", "<i4", 3), ("reserved", "<u4")])
assert DETACH_DTYPE.itemsize == 48 and RESULT_DTYPE.itemsize == 48
CARVE, CAPTURE, ANCHOR_MATERIAL = 1, 2, 4
MAX_PASSES, MAX_EXTENT = 256, 256
ABSENT, SOLID = 0, 2                                        # a stamp voxel's state
FACE_LO_X, FACE_HI_X, FACE_LO_Y, FACE_HI_Y, FACE_LO_Z, FACE_HI_Z = 1, 2, 4, 8, 16, 32
INT32_MAX, INT32_MIN = 0x7FFFFFFF, -0x80000000


def params(lo, hi, flags=0, anchor_faces=0, air_material=0, anchor_mask=0, anchor_value=0, max_passes=MAX_PASSES, reserved0=(0, 0, 0)):
    p = np.zeros((), DETACH_DTYPE)
    p["lo"], p["hi"], p["flags"], p["air_material"], p["anchor_mask"], p["anchor_value"] = lo, hi, flags, air_material, anchor_mask, anchor_value
    p["max_passes"], p["anchor_faces"], p["reserved0"] = max_passes, anchor_faces, reserved0
    return p


def with_(p, **kw):
    """A copy of `p` with fields replaced."""
    q = np.array(p, dtype=DETACH_DTYPE)
    for k, v in kw.items():
        q[k] = v
    return q


def result0(detached=0, supported=0, passes=0, unconverged=0, lo=(INT32_MAX,) * 3, chunks=0, hi=(INT32_MIN,) * 3, reserved=0):
    """A result record: by default what a host starts from."""
    r = np.zeros((), RESULT_DTYPE)
    r["detached"], r["supported"], r["passes"], r["unconverged"], r["chunks"], r["reserved"] = detached, supported, passes, unconverged, chunks, reserved
    r["lo"], r["hi"] = lo, hi
    return r


def shape_of(p):
    """The detach box as a shape_edits box row."""
    return se.box(tuple(int(v) for v in p["lo"]), tuple(int(v) for v in p["hi"]))


def clipped_box(p, R):
    """(lo, hi) int64[3] in (x, y, z), inclusive, or None when the box misses [0, R)^3."""
    return se.bounding_box(shape_of(p), R)


def valid(p, R, stamp_out=True):
    """The host's verdict on the parameters (`stamp_out`: whether the call passes a non-NULL stamp_out)."""
    flags = int(p["flags"])
    if flags & ~(CARVE | CAPTURE | ANCHOR_MATERIAL) or (flags & CAPTURE and not stamp_out):
        return False
    if not 1 <= int(p["max_passes"]) <= MAX_PASSES or int(p["anchor_faces"]) > 63:
        return False
    if int(p["anchor_value"]) & ~int(p["anchor_mask"]) & 0xFFFFFFFF:
        return False
    if not flags & ANCHOR_MATERIAL and (int(p["anchor_mask"]) or int(p["anchor_value"])):
        return False
    if p["reserved0"].any() or not se.valid(shape_of(p), R):
        return False
    bb = clipped_box(p, R)
    return bb is None or all(int(bb[1][k] - bb[0][k]) + 1 <= MAX_EXTENT for k in range(3))


def box_chunks(bb):
    """The chunk ids' coordinates (cx, cy, cz) of the box, in ascending id order (z-major)."""
    if bb is None:
        return []
    return [(cx, cy, cz) for cz in range(int(bb[0][2]) >> 6, (int(bb[1][2]) >> 6) + 1) for cy in range(int(bb[0][1]) >> 6, (int(bb[1][1]) >> 6) + 1)
            for cx in range(int(bb[0][0]) >> 6, (int(bb[1][0]) >> 6) + 1)]


def box_slices(bb):
    return tuple(slice(int(bb[0][k]), int(bb[1][k]) + 1) for k in (2, 1, 0))


def occupancy_and_anchors(mats, mine, p, bb):
    """(occupied, anchor) as bool[ez, ey, ex] over the clipped box."""
    sl = box_slices(bb)
    occ = mine[sl] == 0
    anc = np.zeros(occ.shape, bool)
    faces = int(p["anchor_faces"])
    for k in range(3):                                       # axis k of (x, y, z) is array axis 2 - k
        ix = [slice(None)] * 3
        if faces & (1 << (2 * k)):
            ix[2 - k] = 0
            anc[tuple(ix)] = True
        if faces & (2 << (2 * k)):
            ix[2 - k] = -1
            anc[tuple(ix)] = True
    if int(p["flags"]) & ANCHOR_MATERIAL:
        anc |= (mats[sl] & np.uint32(p["anchor_mask"])) == np.uint32(p["anchor_value"])
    return occ, anc & occ


# ---- (a) the global flood fill ------------------------------------------------------------------------------------------------------
def supported_flood(occ, anc):
    """bool[ez, ey, ex]: what repeated 6-neighbour dilation masked by occupancy reaches from the anchors.  Each step dilates the
    cells reached by the step before, inside their bounding box grown by one cell (nothing else can be new)."""
    sup = anc.copy()
    front = anc
    while front.any():
        nz = [np.nonzero(front.any(axis=tuple(a for a in range(3) if a != k)))[0] for k in range(3)]
        lo = [max(int(n[0]) - 1, 0) for n in nz]
        hi = [min(int(n[-1]) + 2, occ.shape[k]) for k, n in enumerate(nz)]
        win = tuple(slice(a, b) for a, b in zip(lo, hi))
        f = front[win]
        grown = np.zeros(f.shape, bool)
        for k in range(3):
            a, b = [slice(None)] * 3, [slice(None)] * 3
            a[k], b[k] = slice(1, None), slice(None, -1)
            grown[tuple(a)] |= f[tuple(b)]
            grown[tuple(b)] |= f[tuple(a)]
        new = grown & occ[win] & ~sup[win]
        sup[win] |= new
        front = np.zeros(occ.shape, bool)
        front[win] = new
    return sup


# ---- (b) the chunk passes -------------------------------------------------------------------------------------------------------------
def _sweep(reach, occ, axis):
    """The cells of `occ` that a reached cell of the same line along `axis` lies before (at a lower index, itself included) with no
    unoccupied cell between."""
    shape = [1, 1, 1]
    shape[axis] = occ.shape[axis]
    idx = np.arange(occ.shape[axis], dtype=np.int16).reshape(shape)
    last_reached = np.maximum.accumulate(np.where(reach, idx, np.int16(-1)), axis=axis)
    last_free = np.maximum.accumulate(np.where(occ, np.int16(-1), idx), axis=axis)
    return occ & (last_reached > last_free)


def _close(reach, occ):
    """The closure of `reach` through `occ` (one chunk part): sweeps along the three axes in both directions until none adds."""
    while True:
        before = int(reach.sum())
        for k in range(3):
            reach = reach | _sweep(reach, occ, k)
            reach = reach | np.flip(_sweep(np.flip(reach, k), np.flip(occ, k), k), k)
        if int(reach.sum()) == before:
            return reach


def _parts(bb):
    """For each array axis (z, y, x): the index ranges [a, b) into which the 64-texel chunk grid cuts the box."""
    out = []
    for k in (2, 1, 0):
        lo, hi = int(bb[0][k]), int(bb[1][k])
        cuts = [0] + [c - lo for c in range((lo >> 6 << 6) + 64, hi + 1, 64)] + [hi - lo + 1]
        out.append(list(zip(cuts[:-1], cuts[1:])))
    return out


def supported_passes(occ, anc, bb, max_passes=MAX_PASSES):
    """(supported bool[ez, ey, ex] or None when no pass up to max_passes ends the process, the pass count p or max_passes)."""
    parts = _parts(bb)
    s = anc.copy()
    for p in range(1, int(max_passes) + 1):
        seeds = s.copy()
        for k in range(3):                                   # occupied cells that touch S_{p-1} across a chunk face
            first = np.array([a for a, _ in parts[k][1:]], dtype=np.int64)          # the indices at which a later part begins
            if len(first) == 0:
                continue
            a, b = [slice(None)] * 3, [slice(None)] * 3
            a[k], b[k] = first, first - 1
            a, b = tuple(a), tuple(b)
            seeds[a] |= s[b] & occ[a]
            seeds[b] |= s[a] & occ[b]
        nxt = seeds
        for rz in parts[0]:
            for ry in parts[1]:
                for rx in parts[2]:
                    part = (slice(*rz), slice(*ry), slice(*rx))
                    # (from pass 2 on S_{p-1} is closed inside every part: a part that got no seed keeps its set)
                    if p == 1 or not np.array_equal(seeds[part], s[part]):
                        nxt[part] = _close(seeds[part], occ[part])
        if np.array_equal(nxt, s):
            return nxt, p
        s = nxt
    return None, int(max_passes)


# ---- the call ------------------------------------------------------------------------------------------------------------------------
def detach(mats, mine, p, result=None, supported=supported_passes):
    """One valid call on (mats, mine) IN PLACE -> (the result record — `result` added to and merged, or from result0() —, the stamp as
    (materials u32[ez, ey, ex], state u8[ez, ey, ex]) or None without CAPTURE or for an empty clipped box, the dirty chunks as a sorted
    list of (cx, cy, cz)).  `supported`: supported_passes, or supported_flood wrapped by `by_flood` (which cannot tell the passes)."""
    R = mine.shape[0]
    res = np.array(result0() if result is None else result, dtype=RESULT_DTYPE)
    bb = clipped_box(p, R)
    if bb is None:
        return res, None, []
    flags = int(p["flags"])
    occ, anc = occupancy_and_anchors(mats, mine, p, bb)
    sup, passes = supported(occ, anc, bb, int(p["max_passes"]))
    res["passes"] = (int(res["passes"]) + passes) & 0xFFFFFFFF
    stamp = None
    if flags & CAPTURE:
        stamp = (np.zeros(occ.shape, np.uint32), np.full(occ.shape, ABSENT, np.uint8))
    if sup is None:
        res["unconverged"] = (int(res["unconverged"]) + 1) & 0xFFFFFFFF
        return res, stamp, []
    det = occ & ~sup
    z, y, x = np.nonzero(det)
    xyz = np.stack([x + int(bb[0][0]), y + int(bb[0][1]), z + int(bb[0][2])], axis=1).astype(np.int64)
    dirty = sorted(set(map(tuple, (xyz >> 6).tolist())))
    res["detached"] = (int(res["detached"]) + len(xyz)) & 0xFFFFFFFF
    res["supported"] = (int(res["supported"]) + int(sup.sum())) & 0xFFFFFFFF
    res["chunks"] = (int(res["chunks"]) + len(dirty)) & 0xFFFFFFFF
    if len(xyz):
        res["lo"] = np.minimum(res["lo"], xyz.min(axis=0))
        res["hi"] = np.maximum(res["hi"], xyz.max(axis=0))
    if stamp is not None:
        stamp[0][det] = mats[box_slices(bb)][det]
        stamp[1][det] = SOLID
    if flags & CARVE and len(xyz):
        touched = ve.apply_edits(mats, mine, xyz, np.full(len(xyz), int(p["air_material"]), np.uint32), np.zeros(len(xyz), bool))
        assert sorted(touched) == dirty
    return res, stamp, dirty


def by_flood(occ, anc, bb, max_passes):
    """supported_flood in supported_passes' place: the set, and the pass count of supported_passes (the flood has none)."""
    sup_b, passes = supported_passes(occ, anc, bb, max_passes)
    return (None if sup_b is None else supported_flood(occ, anc)), passes
