"""numpy restatement of the voxel stamps (include/rt_abi.h: rt_stamp_capture, rt_edit_stamps) for the stamp tests.  Test infrastructure.

Arrays are [z, y, x] in texel order, as everywhere else; a stamp is a pair (materials u32[ez, ey, ex], state u8[ez, ey, ex]) with state
0 absent, 1 air, 2 solid; a placement is one row of PLACE_DTYPE (RtStampPlace's 32 bytes).  The rule: placements apply in order; the
placed box shows the stamp turned by `orient` (oriented(), built from np.transpose and np.flip alone); a selected voxel — one whose
stamp voxel is not absent, narrowed by `where` — gets the stamp's material word and occupancy state == 2; every 64^3 chunk that meets a
placement's bounding box gets pack_into's minefield (voxel_edits.chunk_minefield) of its occupancy, where a voxel that no placement
selected is occupied iff its minefield value is 0; nothing else changes.
"""
import numpy as np

from tests import voxel_edits as ve
from tests.shape_edits import _minefield

ABSENT, AIR, SOLID = 0, 1, 2                       # a stamp voxel's state
WHERE_ALL, WHERE_SOLID, WHERE_AIR = 0, 1, 2
SKIP_AIR = 1
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
MAX_PLACES = 4096
MAX_STAMPS = 1024
MAX_BOXES = 16

PLACE_DTYPE = np.dtype([("at", "<i4", 3), ("stamp", "<u4"), ("orient", "u1"), ("where", "u1"), ("reserved0", "u1", 2),
                        ("reserved", "<u4", 3)])
assert PLACE_DTYPE.itemsize == 32


def place(stamp, at, orient=0, where=WHERE_ALL):
    s = np.zeros((), PLACE_DTYPE)
    s["at"], s["stamp"], s["orient"], s["where"] = at, stamp, orient, where
    return s


def batch(places):
    return np.array([np.asarray(s, dtype=PLACE_DTYPE) for s in places], dtype=PLACE_DTYPE).reshape(-1)


def extent_of(arr):
    """(ex, ey, ez) of a [z, y, x] array."""
    return tuple(int(v) for v in arr.shape[::-1])


def placed_extent(E, orient):
    """E'_k = E[perm[k]]."""
    perm = PERMS[orient >> 3]
    return tuple(int(E[perm[k]]) for k in range(3))


def oriented(arr, orient):
    """The placed box of a stamp array [z, y, x]: bit j of f flips stamp axis j (numpy axis 2 - j), then world axis k (numpy axis
    2 - k of the result) is stamp axis perm[k]."""
    perm, f = PERMS[orient >> 3], orient & 7
    for j in range(3):
        if (f >> j) & 1:
            arr = np.flip(arr, axis=2 - j)
    axes = [0, 0, 0]
    for k in range(3):
        axes[2 - k] = 2 - perm[k]
    return np.transpose(arr, axes)


def source_voxel(E, orient, d):
    """The header's rule voxel by voxel: the stamp voxel s (x, y, z) that placed-local cell d (x, y, z) shows."""
    perm, f = PERMS[orient >> 3], orient & 7
    s = [0, 0, 0]
    for k in range(3):
        a = perm[k]
        s[a] = E[a] - 1 - d[k] if (f >> a) & 1 else d[k]
    return tuple(s)


def is_rotation(orient):
    """Proper rotation iff the permutation's parity plus the number of flips is even."""
    perm, f = PERMS[orient >> 3], orient & 7
    inversions = sum(1 for i in range(3) for j in range(i + 1, 3) if perm[i] > perm[j])
    return (inversions + bin(f).count("1")) % 2 == 0


def valid(p, R, ids):
    """The host's verdict on one placement."""
    at = p["at"].astype(np.int64)
    if int(p["stamp"]) not in ids or p["orient"] >= 48 or p["where"] > WHERE_AIR:
        return False
    if p["reserved0"].any() or p["reserved"].any():
        return False
    return bool((at >= -4 * R).all() and (at <= 4 * R).all())


def bounding_box(p, E, R):
    """(lo, hi) int64[3] in (x, y, z), inclusive: [at, at + E') clipped to [0, R)^3, or None when it is empty."""
    at = p["at"].astype(np.int64)
    ext = np.array(placed_extent(E, int(p["orient"])), dtype=np.int64)
    lo, hi = np.maximum(at, 0), np.minimum(at + ext, R) - 1
    if (lo > hi).any():
        return None
    return lo, hi


def capture(mats, mine, lo, extent, flags=0):
    """rt_stamp_capture of the box [lo, lo + extent) (x, y, z) of the region (mats, mine): (materials, state) copies."""
    sl = tuple(slice(int(lo[k]), int(lo[k]) + int(extent[k])) for k in (2, 1, 0))
    solid = mine[sl] == 0
    state = np.where(solid, SOLID, ABSENT if flags & SKIP_AIR else AIR).astype(np.uint8)
    m = np.where(state != ABSENT, mats[sl], 0).astype(np.uint32)
    return m, state


def apply_stamps(mats, mine, stamps, places):
    """Applies one rt_edit_stamps batch to the whole region (mats, mine) IN PLACE; `stamps` maps an id to (materials, state).
    Returns the touched chunks as a sorted list of (cx, cy, cz)."""
    R = mine.shape[0]
    occ = {}                                                          # chunk -> bool[64, 64, 64], made when a placement first meets it

    def chunk_slices(c):
        return tuple(slice(64 * c[k], 64 * c[k] + 64) for k in (2, 1, 0))

    for p in places:
        sm, ss = stamps[int(p["stamp"])]
        bb = bounding_box(p, extent_of(ss), R)
        if bb is None:
            continue
        om, os_ = oriented(sm, int(p["orient"])), oriented(ss, int(p["orient"]))
        at = p["at"].astype(np.int64)
        for cz in range(int(bb[0][2]) >> 6, (int(bb[1][2]) >> 6) + 1):
            for cy in range(int(bb[0][1]) >> 6, (int(bb[1][1]) >> 6) + 1):
                for cx in range(int(bb[0][0]) >> 6, (int(bb[1][0]) >> 6) + 1):
                    c = (cx, cy, cz)
                    c0 = np.array(c, dtype=np.int64) * 64
                    if c not in occ:
                        occ[c] = mine[chunk_slices(c)] == 0
                    lo, hi = np.maximum(bb[0], c0), np.minimum(bb[1], c0 + 63)          # the box inside this chunk
                    sl = tuple(slice(int(lo[k] - c0[k]), int(hi[k] - c0[k]) + 1) for k in (2, 1, 0))
                    src = tuple(slice(int(lo[k] - at[k]), int(hi[k] - at[k]) + 1) for k in (2, 1, 0))
                    state = os_[src]
                    m = state != ABSENT
                    if p["where"] == WHERE_SOLID:
                        m = m & occ[c][sl]
                    elif p["where"] == WHERE_AIR:
                        m = m & ~occ[c][sl]
                    occ[c][sl][m] = state[m] == SOLID
                    mats[chunk_slices(c)][sl][m] = om[src][m]
    for c in sorted(occ):
        mine[chunk_slices(c)] = _minefield(occ[c])
    return sorted(occ)


def pending_boxes(stamps, places, R):
    """The texel boxes (lo, hi) rt_edit_stamps records on a context with edit_radius > 0: one per placement with a bounding box."""
    out = []
    for p in places:
        bb = bounding_box(p, extent_of(stamps[int(p["stamp"])][1]), R)
        if bb is not None:
            out.append(bb)
    return out


def enumerate_records(mats, mine, stamps, places):
    """The batch as rt_edit_voxels rows (xyz, materials, solid) in placement order — one per selected voxel — and the chunks the
    placements touch (sorted (cx, cy, cz)).  (mats, mine) is the whole region and is not changed."""
    R = mine.shape[0]
    occ = mine == 0
    xyz, words, solid, touched = [], [], [], set()
    for p in places:
        sm, ss = stamps[int(p["stamp"])]
        bb = bounding_box(p, extent_of(ss), R)
        if bb is None:
            continue
        lo, hi = bb
        touched |= {(cx, cy, cz) for cz in range(int(lo[2]) >> 6, (int(hi[2]) >> 6) + 1) for cy in range(int(lo[1]) >> 6, (int(hi[1]) >> 6) + 1)
                    for cx in range(int(lo[0]) >> 6, (int(hi[0]) >> 6) + 1)}
        at = p["at"].astype(np.int64)
        sl = tuple(slice(int(lo[k]), int(hi[k]) + 1) for k in (2, 1, 0))
        src = tuple(slice(int(lo[k] - at[k]), int(hi[k] - at[k]) + 1) for k in (2, 1, 0))
        state, om = oriented(ss, int(p["orient"]))[src], oriented(sm, int(p["orient"]))[src]
        m = state != ABSENT
        if p["where"] == WHERE_SOLID:
            m = m & occ[sl]
        elif p["where"] == WHERE_AIR:
            m = m & ~occ[sl]
        z, y, x = np.nonzero(m)
        xyz.append(np.stack([x + lo[0], y + lo[1], z + lo[2]], axis=1))
        words.append(om[m].astype(np.uint32))
        solid.append(state[m] == SOLID)
        occ[sl][m] = state[m] == SOLID
    if not xyz:
        return np.zeros((0, 3), np.int64), np.zeros(0, np.uint32), np.zeros(0, bool), sorted(touched)
    return np.concatenate(xyz), np.concatenate(words), np.concatenate(solid), sorted(touched)
