"""Worlds outside the shape every `pack_into` scene has (minefield values 0..6 that bound the distance per 64^3 chunk, material
words from a 7-entry palette), for the parity tests of tests/test_adversarial_worlds.py and tests/test_gpu_adversarial_worlds.py.
Test infrastructure.  Arrays are [z, y, x] in texel order (texel = world + R/2), as everywhere else.

* `pyramid_world`: the rule of pack_into (value = smallest L >= 1 whose aligned 2^L cube holds a solid voxel) over the whole
  region instead of per chunk: a legal distance bound whose sky holds values above 6 (7 at R = 256, up to 9 at 1024: the
  terrain reaches into every half of the region) in uniform coarse cubes.
* `arbitrary_world`: legal (every value 0..30, which rt_upload_world accepts) but no distance bound.  Each coarse cube of the
  kernels' nibble map (edge R/64) is uniform v for some v in 0..30, mixed (random per-voxel values 0..30) or "uniform 1 except
  one solid voxel"; material words are random over all 32 bits, some solid voxels carry the word 0.  Around the camera poses
  of POSES the cubes are biased towards small values, so that frames hit geometry instead of leaving the region at once.
"""
import numpy as np

from raytrace_amd import world

# Camera poses, in world units of the 256 region (scaled by R / 256 for the larger ones): origin, heading, pitch, sun, lr.
# The last two: a camera outside the region (raytrace.comp:311-315 moves the start onto the face) and a scrolled window.
POSES = [
    dict(origin=(-40.0, -40.0, 20.0), heading=0.6, pitch=-0.2, sun=0.3, lr=(0, 0, 0)),
    dict(origin=(30.0, 50.0, -30.0), heading=-2.4, pitch=0.15, sun=-0.6, lr=(0, 0, 0)),
    dict(origin=(10.0, -90.0, 60.0), heading=1.3, pitch=-0.5, sun=1.1, lr=(0, 0, 0)),
    dict(origin=(-30.0, -200.0, 40.0), heading=np.pi / 2, pitch=-0.1, sun=0.2, lr=(0, 0, 0)),
    dict(origin=(60.0, -20.0, 40.0), heading=2.2, pitch=-0.3, sun=0.5, lr=(16, -32, 16)),
]

# The same roles on the terrain of the pyramid world (its ground is solid below world z = 0, hills reach the region's top).
PYRAMID_POSES = [
    dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.1, sun=0.3, lr=(0, 0, 0)),
    dict(origin=(60.0, 40.0, 120.0), heading=-2.4, pitch=-0.35, sun=-0.6, lr=(0, 0, 0)),
    dict(origin=(10.0, -90.0, 110.0), heading=1.3, pitch=-0.6, sun=1.1, lr=(0, 0, 0)),
    dict(origin=(-30.0, -200.0, 100.0), heading=np.pi / 2, pitch=-0.1, sun=0.2, lr=(0, 0, 0)),
    dict(origin=(60.0, -20.0, 120.0), heading=2.2, pitch=-0.3, sun=0.5, lr=(16, -32, 16)),
]
KIND_UNIFORM, KIND_MIXED, KIND_ODD = 0, 1, 2
# Uniform values of the cubes away from the cameras: every value 0..30, the nibble map's boundaries (6/7: the palette's
# largest value, 14/15: the largest stored value and "mixed") and the ABI's largest (30) weighted up, small values most.
_FAR_WEIGHTS = np.ones(31)
_FAR_WEIGHTS[[6, 7, 14, 15, 16, 30]] = 4.0
_FAR_WEIGHTS[[1, 2, 3]] = 18.0
_FAR_WEIGHTS[0] = 6.0
_NEAR_WEIGHTS = np.zeros(31)
_NEAR_WEIGHTS[[0, 1, 2, 3]] = (1.0, 12.0, 5.0, 2.0)


def pose_origin(pose, R):
    return tuple(c * (R // 256) for c in pose["origin"])


def pose_lr(pose, R):
    return tuple(c * (R // 256) for c in pose["lr"])


def pose_uniforms(po, pose, R, seed=7):
    return po.camera_uniforms(pose_origin(pose, R), pose["heading"], pose["pitch"], pose["sun"], seed, pose_lr(pose, R))


def pyramid_minefield(solid):
    """value = 0 on solid voxels, else the smallest L >= 1 whose aligned 2^L cube holds a solid voxel (log2(R) if none does)."""
    R = solid.shape[0]
    logr = R.bit_length() - 1
    occ = [None, solid.reshape(R // 2, 2, R // 2, 2, R // 2, 2).any(axis=(1, 3, 5))]
    for L in range(2, logr + 1):
        n = R >> L
        occ.append(occ[-1].reshape(n, 2, n, 2, n, 2).any(axis=(1, 3, 5)))
    v = np.full((1, 1, 1), logr, dtype=np.uint8)
    for L in range(logr, 0, -1):
        n = R >> L
        v = np.where(occ[L], np.uint8(L), v).astype(np.uint8)
        if L > 1:      # up one level: every cube of level L splits into 8 of level L - 1
            v = np.broadcast_to(v[:, None, :, None, :, None], (n, 2, n, 2, n, 2)).reshape(2 * n, 2 * n, 2 * n)
    h = R // 2
    out = np.broadcast_to(v[:, None, :, None, :, None], (h, 2, h, 2, h, 2)).reshape(R, R, R).copy()
    out[solid] = 0
    return out


def pyramid_world(R=256, seed=world.DEFAULT_SEED):
    """The procedural terrain of `seed` with the region-wide pyramid minefield.  Returns (materials, minefield, pack_into's
    minefield of the same solids)."""
    mats, mine = world.generate_region(seed, region=R)
    solid = mine == 0
    return mats, pyramid_minefield(solid), mine


def _near_cameras(R, radius):
    """[64,64,64] bool: coarse cubes whose centre lies within `radius` texels of a pose's origin (on the torus, so that the
    scrolled window's wrap is covered), plus every cube along the first `radius` texels of each pose's view direction."""
    e = R // 64
    c = (np.arange(64) + 0.5) * e
    near = np.zeros((64, 64, 64), dtype=bool)
    for pose in POSES:
        o = np.array(pose_origin(pose, R)) + R / 2
        o = np.clip(o, 0, R - 1)        # a camera outside the region: its rays enter at the face
        d = [np.minimum(np.abs(c - o[a]), R - np.abs(c - o[a])) for a in range(3)]
        near |= (d[2][:, None, None] ** 2 + d[1][None, :, None] ** 2 + d[0][None, None, :] ** 2) < radius ** 2
    return near


def arbitrary_world(R=256, seed=1):
    """Returns (materials u32[R,R,R], minefield u8[R,R,R], kinds u8[64,64,64], cube values u8[64,64,64]) — `kinds` and the
    values are what each coarse cube was drawn as (for the coverage checks)."""
    rng = np.random.default_rng(seed)
    e = R // 64
    near = _near_cameras(R, 48 * (R // 256))
    # the kind of each coarse cube: uniform, mixed or odd-voxel — near the cameras no mixed cubes (their big values end rays)
    u = rng.random((64, 64, 64))
    kinds = np.where(u < 0.14, KIND_MIXED, np.where(u < 0.34, KIND_ODD, KIND_UNIFORM)).astype(np.uint8)
    kinds[near & (kinds == KIND_MIXED)] = KIND_ODD
    vals = np.where(near, rng.choice(31, size=(64, 64, 64), p=_NEAR_WEIGHTS / _NEAR_WEIGHTS.sum()),
                    rng.choice(31, size=(64, 64, 64), p=_FAR_WEIGHTS / _FAR_WEIGHTS.sum())).astype(np.uint8)
    vals[kinds == KIND_ODD] = 1
    for pose in POSES:                  # no camera inside a solid voxel
        t = (np.clip(np.array(pose_origin(pose, R)) + R / 2, 0, R - 1) // e).astype(int)
        kinds[t[2], t[1], t[0]] = KIND_UNIFORM
        vals[t[2], t[1], t[0]] = 1
    # the odd voxel of each odd cube: the 64 offsets inside a 4^3 brick and the (e/4)^3 bricks of the cube taken in turn
    odd = np.argwhere(kinds == KIND_ODD)
    k = np.arange(len(odd))
    nsub = (e // 4) ** 3
    o64, sb = k % 64, (k // 64) % nsub
    sub = e // 4
    off = np.stack([(sb // (sub * sub)) * 4 + (o64 >> 4), ((sb // sub) % sub) * 4 + ((o64 >> 2) & 3), (sb % sub) * 4 + (o64 & 3)], 1)
    odd_voxels = odd * e + off          # (z, y, x)
    mats = np.empty((R, R, R), dtype=np.uint32)
    mine = np.empty((R, R, R), dtype=np.uint8)
    for cz in range(64):                # one layer of coarse cubes at a time: bounded temporaries at R = 1024
        z0 = cz * e
        layer = np.broadcast_to(vals[cz][None, :, None, :, None], (e, 64, e, 64, e)).reshape(e, R, R).copy()
        mixed = np.broadcast_to((kinds[cz] == KIND_MIXED)[None, :, None, :, None], (e, 64, e, 64, e)).reshape(e, R, R)
        rnd = rng.integers(0, 31, size=(e, R, R), dtype=np.uint8)
        layer[mixed] = rnd[mixed]
        sel = odd_voxels[:, 0] // e == cz
        layer[odd_voxels[sel, 0] - z0, odd_voxels[sel, 1], odd_voxels[sel, 2]] = 0
        mine[z0:z0 + e] = layer
        m = rng.integers(0, 1 << 32, size=(e, R, R), dtype=np.uint32)
        m[rng.random((e, R, R), dtype=np.float32) < 0.03] = 0
        mats[z0:z0 + e] = m
    return mats, mine, kinds, vals


def uniform_bricks(minefield):
    """[64^3] u8: 1 where the 4^3 brick of a 256 region holds one value (what the oracle's fetch histogram splits on)."""
    b = np.asarray(minefield).reshape(64, 4, 64, 4, 64, 4)
    return np.ascontiguousarray((b.min(axis=(1, 3, 5)) == b.max(axis=(1, 3, 5))).astype(np.uint8).reshape(-1))
