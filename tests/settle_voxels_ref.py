"""numpy restatement of rt_settle_voxels (include/rt_abi.h "Voxel settling") for the settle tests.  Test infrastructure, written from
the rules and not from the kernels.

The box's validity and clipping are tests/shape_edits.py's (`valid`, `bounding_box`) and the world change goes through
tests/voxel_edits.py's `apply_edits`: no shape rule and no rebuild rule is restated here.  Arrays are [z, y, x] in texel order.

The rules.  Fix the two coordinates across `axis` and number the clipped box's cells along it by height h (h = x - lo' for toward = 0,
hi' - x for toward = 1).  A cell is OCCUPIED iff its minefield byte is 0, an occupied cell LOOSE iff (material & loose_mask) ==
loose_value, else FIXED.  For a loose cell at h, f = 1 + the highest fixed h' < h (0 if none) and E(h) = the number of unoccupied h'
with f <= h' < h; the voxel moves to h - min(max_fall, E(h)) with its word.  A cell a voxel left and none arrived at becomes
unoccupied with air_material; a cell a falling voxel only passes keeps its word.  The chunks that hold a source or a target of a
voxel that moved are rebuilt as rt_edit_voxels rebuilds them: one solid = 0 record per source, then one solid = 1 record per target.
moved / falling / distance / chunks are added to, wrapping.

`settle` is the closed form; `settle_naive` says the same a second way — max_fall sweeps, each moving a loose voxel one cell down,
bottom-up, if the cell below is free — and shares nothing with it but the box and the column view."""
import numpy as np

from tests import shape_edits as se
from tests import voxel_edits as ve

# numpy views of RtVoxelSettle and RtSettleCount, declared here a second time on purpose (the binding's own are
# raytrace_amd.abi.SETTLE_DTYPE and SETTLE_COUNT_DTYPE)
SETTLE_DTYPE = np.dtype([("lo", "<i4", 3), ("max_fall", "<u4"), ("hi", "<i4", 3), ("air_material", "<u4"), ("loose_mask", "<u4"), ("loose_value", "<u4"),
                         ("axis", "u1"), ("toward", "u1"), ("reserved0", "u1", 2), ("reserved1", "<u4")])
COUNT_DTYPE = np.dtype([("moved", "<u4"), ("falling", "<u4"), ("distance", "<u4"), ("chunks", "<u4")])
assert SETTLE_DTYPE.itemsize == 48 and COUNT_DTYPE.itemsize == 16
UNLIMITED = 0xFFFFFFFF


def params(lo, hi, max_fall=UNLIMITED, air_material=0, loose_mask=0, loose_value=0, axis=2, toward=0, reserved0=(0, 0), reserved1=0):
    p = np.zeros((), SETTLE_DTYPE)
    p["lo"], p["hi"], p["max_fall"], p["air_material"], p["loose_mask"], p["loose_value"] = lo, hi, max_fall, air_material, loose_mask, loose_value
    p["axis"], p["toward"], p["reserved0"], p["reserved1"] = axis, toward, reserved0, reserved1
    return p


def with_(p, **kw):
    """A copy of `p` with fields replaced."""
    q = np.array(p, dtype=SETTLE_DTYPE)
    for k, v in kw.items():
        q[k] = v
    return q


def shape_of(p):
    """The settle box as a shape_edits box row."""
    return se.box(tuple(int(v) for v in p["lo"]), tuple(int(v) for v in p["hi"]))


def valid(p, R):
    """The host's verdict on the parameters."""
    if p["axis"] > 2 or p["toward"] > 1 or p["max_fall"] == 0 or int(p["loose_value"]) & ~int(p["loose_mask"]) & 0xFFFFFFFF:
        return False
    if p["reserved0"].any() or p["reserved1"] != 0:
        return False
    return bool(se.valid(shape_of(p), R))


def clipped_box(p, R):
    """(lo, hi) int64[3] in (x, y, z), inclusive, or None when the box misses [0, R)^3."""
    return se.bounding_box(shape_of(p), R)


def box_chunks(bb):
    """The chunk ids' coordinates (cx, cy, cz) of the box, in ascending id order (z-major)."""
    if bb is None:
        return []
    return [(cx, cy, cz) for cz in range(int(bb[0][2]) >> 6, (int(bb[1][2]) >> 6) + 1) for cy in range(int(bb[0][1]) >> 6, (int(bb[1][1]) >> 6) + 1)
            for cx in range(int(bb[0][0]) >> 6, (int(bb[1][0]) >> 6) + 1)]


def box_slices(bb):
    return tuple(slice(int(bb[0][k]), int(bb[1][k]) + 1) for k in (2, 1, 0))


def columns(a, axis, toward):
    """A view of the box array a[z, y, x] with the fall axis last and h ascending: [.., .., h]."""
    v = np.moveaxis(a, 2 - int(axis), -1)
    return v[..., ::-1] if toward else v


def _coords(bb, axis, toward):
    """int64[.., .., H, 3]: the texel (x, y, z) of every cell of the box in the layout of `columns`."""
    z, y, x = np.meshgrid(*(np.arange(int(bb[0][k]), int(bb[1][k]) + 1, dtype=np.int64) for k in (2, 1, 0)), indexing="ij")
    return np.stack([columns(c, axis, toward) for c in (x, y, z)], axis=-1)


def drops(occ, loose, max_fall):
    """The closed form on column views (bool[.., .., H]): (drop, E) as int64 arrays, 0 where the cell is not loose."""
    free = ~occ
    below = np.cumsum(free, axis=-1) - free                                  # unoccupied cells under h
    fixed = occ & ~loose
    # `below` at the last fixed cell under h (it never falls as h rises, so the running maximum is the last one's), 0 if none
    base = np.maximum.accumulate(np.where(fixed, below, 0), axis=-1)
    E = np.where(occ & loose, below - base, 0).astype(np.int64)
    return np.minimum(E, int(max_fall)), E


def moves(mats, mine, p):
    """What a call on (mats, mine) does, nothing changed: dict(src, dst: int64[N, 3] texels (x, y, z) of the voxels that move, words:
    u32[N], moved, falling, distance) — or None for an empty clipped box."""
    R = mine.shape[0]
    assert valid(p, R)
    bb = clipped_box(p, R)
    if bb is None:
        return None
    sl = box_slices(bb)
    occ = columns(mine[sl] == 0, p["axis"], p["toward"])
    word = columns(mats[sl], p["axis"], p["toward"])
    loose = occ & ((word & np.uint32(p["loose_mask"])) == np.uint32(p["loose_value"]))
    drop, E = drops(occ, loose, p["max_fall"])
    xyz = _coords(bb, p["axis"], p["toward"])
    sel = drop > 0
    src = xyz[sel]
    dst = src.copy()
    dst[:, int(p["axis"])] += np.where(p["toward"], 1, -1) * drop[sel]
    return dict(src=src, dst=dst, words=word[sel].copy(), moved=int(sel.sum()), falling=int((E > drop).sum()), distance=int(drop.sum()))


def settle(mats, mine, p, counts=None):
    """One call on (mats, mine), changed IN PLACE -> (counts, touched): a COUNT_DTYPE record added to (zeros for None) and the sorted
    (cx, cy, cz) of the chunks that were rebuilt.  An empty clipped box changes nothing."""
    cnt = np.zeros(1, COUNT_DTYPE)[0] if counts is None else np.array(counts, dtype=COUNT_DTYPE).reshape(1)[0].copy()
    m = moves(mats, mine, p)
    if m is None:
        return cnt, []
    n = len(m["src"])
    xyz = np.concatenate([m["src"], m["dst"]])                                # the sources first: a target's record is the later one
    words = np.concatenate([np.full(n, p["air_material"], np.uint32), m["words"]])
    touched = sorted(ve.apply_edits(mats, mine, xyz, words, np.concatenate([np.zeros(n, bool), np.ones(n, bool)])))
    for k, v in (("moved", m["moved"]), ("falling", m["falling"]), ("distance", m["distance"]), ("chunks", len(touched))):
        cnt[k] = (int(cnt[k]) + v) & 0xFFFFFFFF
    return cnt, touched


def settle_naive(mats, mine, p):
    """The second restatement, nothing changed: sweeps over the box -> (occ, words, counts, dirty): the box's occupancy (bool[z, y, x])
    and material words after the call, what the call adds to the counts as a dict, and the sorted chunks (cx, cy, cz) that hold the
    first or the last cell of a voxel that ended elsewhere.  None for an empty clipped box."""
    R = mine.shape[0]
    bb = clipped_box(p, R)
    if bb is None:
        return None
    sl = box_slices(bb)
    occ_box, word_box = mine[sl] == 0, mats[sl].copy()
    occ0, word0 = occ_box.copy(), word_box.copy()
    occ, word = columns(occ_box, p["axis"], p["toward"]), columns(word_box, p["axis"], p["toward"])
    H = occ.shape[-1]
    origin = np.where(occ, np.arange(H), -1) + np.zeros(occ.shape, np.int64)   # the height a cell's voxel started at
    mask, value, air = np.uint32(p["loose_mask"]), np.uint32(p["loose_value"]), np.uint32(p["air_material"])

    def sweep(occ, word, origin):
        n = 0
        for h in range(1, H):                                                 # bottom-up: a voxel may follow the one under it
            go = occ[..., h] & ((word[..., h] & mask) == value) & ~occ[..., h - 1]
            n += int(go.sum())
            occ[..., h - 1] |= go
            word[..., h - 1] = np.where(go, word[..., h], word[..., h - 1])
            origin[..., h - 1] = np.where(go, origin[..., h], origin[..., h - 1])
            occ[..., h] &= ~go
            word[..., h] = np.where(go, air, word[..., h])
            origin[..., h] = np.where(go, -1, origin[..., h])
        return n

    distance = 0
    for _ in range(min(int(p["max_fall"]), H)):
        n = sweep(occ, word, origin)
        distance += n
        if n == 0:
            break
    falling = sweep(occ.copy(), word.copy(), origin.copy())                  # who would move in one more sweep
    # a cell that ends unoccupied holds air_material if a voxel of the call's start left it, else its own word (a cell a voxel only
    # passed through included)
    word_box[~occ_box] = np.where(occ0, air, word0)[~occ_box]
    xyz = _coords(bb, p["axis"], p["toward"])
    went = (origin >= 0) & (origin != np.arange(H))
    ends = xyz[went]
    starts = ends.copy()
    starts[:, int(p["axis"])] += np.where(p["toward"], -1, 1) * (origin[went] - np.nonzero(went)[-1])
    dirty = sorted(set(map(tuple, (np.concatenate([starts, ends]) >> 6).tolist())))
    return occ_box, word_box, dict(moved=int(went.sum()), falling=falling, distance=distance, chunks=len(dirty)), dirty
