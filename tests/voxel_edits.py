"""numpy restatement of rt_edit_voxels (include/rt_abi.h) for the voxel-edit tests.  Test infrastructure.

Arrays are [z, y, x] in texel order, as everywhere else; edits are rows (x, y, z) with a material word and a solid flag.
The rule: the last edit of a voxel wins; every 64^3 chunk holding an edit gets pack_into's minefield (src/world/chunk.rs:125-184)
of its occupancy, where an edited voxel is occupied iff its edit is solid and any other voxel iff its minefield value is 0;
nothing else changes.
"""
import numpy as np

CHUNK = 64


def chunk_minefield(occ):
    """pack_into's minefield of one 64^3 occupancy array: 0 on occupied voxels, else the first L in 1..6 whose aligned 2^L cube
    holds an occupied voxel (6 in a chunk with nothing occupied)."""
    occ = np.asarray(occ, dtype=bool).reshape(CHUNK, CHUNK, CHUNK)
    out = np.full(occ.shape, 6, np.uint8)
    levels = [occ]
    for L in range(1, 7):
        n = CHUNK >> L
        levels.append(levels[-1].reshape(n, 2, n, 2, n, 2).any(axis=(1, 3, 5)))
    for L in range(6, 0, -1):
        s = 1 << L
        out[levels[L].repeat(s, 0).repeat(s, 1).repeat(s, 2)] = L
    out[occ] = 0
    return out


def last_wins(xyz, materials, solid):
    """The edits that take effect: one per voxel, the last of the batch, in no particular order."""
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    materials = np.asarray(materials, dtype=np.uint32).reshape(-1)
    solid = np.asarray(solid).reshape(-1) != 0
    if xyz.shape[0] == 0:
        return xyz, materials, solid
    key = (xyz[:, 2] << 32) | (xyz[:, 1] << 16) | xyz[:, 0]
    _, first_of_reversed = np.unique(key[::-1], return_index=True)
    keep = xyz.shape[0] - 1 - first_of_reversed
    return xyz[keep], materials[keep], solid[keep]


def apply_edits(mats, mine, xyz, materials, solid):
    """Applies one rt_edit_voxels batch to (mats, mine) IN PLACE; returns the touched chunks as a list of (cx, cy, cz)."""
    xyz, materials, solid = last_wins(xyz, materials, solid)
    if xyz.shape[0] == 0:
        return []
    cidx = xyz >> 6
    chunks = sorted(set(map(tuple, cidx.tolist())))
    for (cx, cy, cz) in chunks:
        sel = np.all(cidx == (cx, cy, cz), axis=1)
        x, y, z = (xyz[sel, a] - 64 * c for a, c in ((0, cx), (1, cy), (2, cz)))
        box = (slice(64 * cz, 64 * cz + 64), slice(64 * cy, 64 * cy + 64), slice(64 * cx, 64 * cx + 64))
        occ = mine[box] == 0
        occ[z, y, x] = solid[sel]
        mats[box][z, y, x] = materials[sel]
        mine[box] = chunk_minefield(occ)
    return chunks


def edit_records(xyz, materials, solid, reserved=None):
    """RtVoxelEdit rows as a numpy structured array (16 bytes each)."""
    xyz = np.asarray(xyz).reshape(-1, 3)
    recs = np.zeros(xyz.shape[0], dtype=[("x", "<u2"), ("y", "<u2"), ("z", "<u2"), ("solid", "<u2"), ("material", "<u4"),
                                         ("reserved", "<u4")])
    recs["x"], recs["y"], recs["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    recs["solid"] = np.asarray(solid).reshape(-1) != 0
    recs["material"] = np.asarray(materials, dtype=np.uint32).reshape(-1)
    if reserved is not None:
        recs["reserved"] = reserved
    return recs
