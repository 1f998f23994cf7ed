"""Noise textures other than tests/golden/blue_noise_512.rgba, and a world on which a frame's fate depends on them (test
infrastructure, numpy only) — for tests/test_adversarial_noise.py (the conditions, on the CPU) and
tests/test_gpu_adversarial_noise.py (parity).

The noise byte pair (r, g) of a path indexes the kernels' direction tables (sphere_lut, dif_lut: 6 faces x 65 536, sun_lut), so a
frame exercises exactly the entries its texels hold.  The shader's addressing is simple (raytrace.comp:298-304, :324): pixel
(px, py) of the sample with seed s reads texel ((bx + 8 wg(px)) mod 512, (by + 8 wg(py)) mod 512), (bx, by) = the r, g bytes of
texel (s % 512, min(s / 512, 511)), wg(p) = (p / 128) * 16 + p % 16 — the same texel at every level of the path.  A 16 x 16 frame
therefore reads a 16 x 16 lattice of spacing 8, and 256 samples whose base texels run over {0..7, 128..135}^2 tile the block
[0, 256)^2 exactly once.  `lattice_noise` holds every (r, g) pair once in that block and those base texels in row 300.

Arrays of worlds are [z, y, x] in texel order (texel = world + 128), as everywhere else."""
import functools

import numpy as np

from tests import adversarial_worlds

NOISE_SIZE = 512
LATTICE_ROW = 300
LATTICE_SEED0 = LATTICE_ROW * NOISE_SIZE      # seeds seed0 .. seed0 + 255 take their base texels from row 300, x = 0..255
LATTICE_FRAME = (16, 16, 256)                 # width, height, samples of the frame that reads the block once


def _base_byte(i):
    """The i-th of the 16 base offsets {0..7, 128..135}: with the lattice's 16 points of spacing 8 they cover 0..255 once."""
    return i % 8 + 128 * (i // 8)


def lattice_noise(perm_seed=0):
    """u8[512, 512, 4].  T[y, x, 0:2] for x, y < 256: a seeded bijection onto all 65 536 (r, g) pairs; row 300, x = k < 256: the base
    texel (k % 16, k / 16) of sample k; every other byte (all b and a channels included) random."""
    rng = np.random.default_rng(perm_seed)
    T = rng.integers(0, 256, size=(NOISE_SIZE, NOISE_SIZE, 4), dtype=np.uint8)
    pairs = rng.permutation(65536).astype(np.uint32)
    T[:256, :256, 0] = (pairs & 255).reshape(256, 256)
    T[:256, :256, 1] = (pairs >> 8).reshape(256, 256)
    k = np.arange(256)
    T[LATTICE_ROW, :256, 0] = _base_byte(k % 16)
    T[LATTICE_ROW, :256, 1] = _base_byte(k // 16)
    return T


def workgroup_of(p):
    return (p // 128) * 16 + p % 16


def lattice_reads(width, height, seed0, spp, noise=None):
    """The numpy model of the addressing: int[512, 512] (row = y), how often a width x height frame of `spp` samples starting at
    seed `seed0` reads each texel as a path's noise_value (once per level).  `noise`: the texture the base texels are taken from
    (default: lattice_noise(), whose row 300 does not depend on perm_seed)."""
    T = (lattice_noise() if noise is None else np.asarray(noise)).reshape(NOISE_SIZE, NOISE_SIZE, 4)
    reads = np.zeros((NOISE_SIZE, NOISE_SIZE), dtype=np.int64)
    wx, wy = workgroup_of(np.arange(width)) * 8, workgroup_of(np.arange(height)) * 8
    for s in range(spp):
        seed = (seed0 + s) % (NOISE_SIZE * NOISE_SIZE * 4)
        bx, by = T[min(seed // NOISE_SIZE, NOISE_SIZE - 1), seed % NOISE_SIZE, :2].astype(np.int64)
        np.add.at(reads, (((by + wy) % NOISE_SIZE)[:, None], ((bx + wx) % NOISE_SIZE)[None, :]), 1)
    return reads


def constant_noise(r, g, seed=0):
    """Every texel (r, g, random, random): (0, 0) makes every diffuse ray off a face-5 surface NaN (the sphere point (0, 0, 1) plus
    the face's (0, 0, -1)), (255, 255) makes every one off face 4 run along the surface with 1 / |d.z| = inf."""
    T = np.random.default_rng(seed).integers(0, 256, size=(NOISE_SIZE, NOISE_SIZE, 4), dtype=np.uint8)
    T[..., 0], T[..., 1] = r, g
    return T


def extreme_noise(seed=0):
    """Every byte drawn from {0, 1, 127, 128, 254, 255}."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 1, 127, 128, 254, 255], dtype=np.uint8), size=(NOISE_SIZE, NOISE_SIZE, 4))


def random_noise(seed=0):
    """Independent uniform bytes."""
    return np.random.default_rng(seed).integers(0, 256, size=(NOISE_SIZE, NOISE_SIZE, 4), dtype=np.uint8)


CUBE_LO, CUBE_HI = 64, 192          # solid texels 64..191 on each axis: world -64 .. 64
SHELL_DISTANCE, SHELL_DENSITY = 24, 0.5


@functools.lru_cache(maxsize=None)
def cube_world(shell, seed=5):
    """(materials u32, minefield u8) [256, 256, 256], read-only and built once: a solid cube with the region-wide pyramid
    minefield and random non-zero 32-bit material words.  shell=True adds one-voxel "dust" at Chebyshev distance 24 from the cube,
    each voxel solid with probability 0.5: whether a ray leaves then depends on its direction to about 0.01 rad, and the paths'
    deeper levels stand on all six faces."""
    rng = np.random.default_rng(seed)
    solid = np.zeros((256, 256, 256), dtype=bool)
    solid[CUBE_LO:CUBE_HI, CUBE_LO:CUBE_HI, CUBE_LO:CUBE_HI] = True
    if shell:
        c = np.arange(256)
        d1 = np.maximum(np.maximum(CUBE_LO - c, c - (CUBE_HI - 1)), 0)
        cheb = np.maximum(np.maximum(d1[:, None, None], d1[None, :, None]), d1[None, None, :])
        solid |= (cheb == SHELL_DISTANCE) & (rng.random(solid.shape) < SHELL_DENSITY)
    mine = adversarial_worlds.pyramid_minefield(solid)
    words = rng.integers(1, 1 << 32, size=solid.shape, dtype=np.uint64).astype(np.uint32)
    mats = np.where(solid, words, np.uint32(0)).astype(np.uint32)
    mats.setflags(write=False)
    mine.setflags(write=False)
    return mats, mine


# Six poses about 6 voxels off each cube face, looking straight at it: (face id every pixel of a 16 x 16 frame shows, origin,
# heading, pitch).  Face ids: 0 = +x, 1 = -x, 2 = +y, 3 = -y, 4 = +z, 5 = -z.
FACE_VIEWS = [
    (4, (0.3, 0.2, 70.0), 0.3, -1.5),
    (5, (0.3, 0.2, -70.5), 0.3, 1.5),
    (1, (-70.0, 0.3, 0.2), 0.0, 0.0),
    (0, (70.0, 0.3, 0.2), np.pi, 0.0),
    (3, (0.3, -70.0, 0.2), np.pi / 2, 0.0),
    (2, (0.3, 70.0, 0.2), -np.pi / 2, 0.0),
]
# The sun angle under which a good share of each face's shadow rays reaches the sky through the dust (the sun ray's cone is 0.05
# wide, so the share jumps with the angle; tests/test_adversarial_noise.py measures it), and a face turned away from each sun.
FACE_SUN = {4: 0.6, 5: 3.2, 1: -2.8, 0: 3.2, 3: -2.8, 2: 0.2}
SUN_ANGLES = (0.6, -2.2, -2.8, 3.2, 0.2)
# A sun behind each face: every shadow ray ends in the cube at once, so the frame's depth-1 sky exits are its diffuse exits alone.
FACE_DARK_SUN = {4: -2.2, 5: 0.6, 1: 0.6, 0: -2.2, 3: 0.6, 2: -2.2}
FACE_NORMALS = {0: (1, 0, 0), 1: (-1, 0, 0), 2: (0, 1, 0), 3: (0, -1, 0), 4: (0, 0, 1), 5: (0, 0, -1)}


def view_uniforms(po, view, sun, seed=LATTICE_SEED0):
    _, origin, heading, pitch = view
    return po.camera_uniforms(origin, heading, pitch, sun, seed)
