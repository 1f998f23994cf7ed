"""The deterministic terrain of raytrace_amd/host/world.cpp restated in numpy: the hashes, the gradient noise, the height function,
the material roll and a whole packed chunk.  Written from world.cpp alone (not from csrc/rt_terrain.hip), FP64 throughout, every
operation in the host's order, vectorised over columns.  It is the second statement that the host generator and the device kernels
are both compared with (tests/test_terrain_ref.py, tests/test_gpu_terrain_far.py).

np.power is the C library's pow, the same function the host calls: the restatement is independent of the host in everything but
that call.  The tests therefore also bound how close the value before truncation comes to an integer (ulps_to_integer): with a
margin of 2^20 ULPs no two pow implementations, each a few ULPs from the true value, can truncate to different heights.

The module also holds the inputs the far-terrain tests share, so that the CPU test of the margin condition runs over exactly the
columns the GPU tests compare (gpu_columns)."""
import numpy as np

U64 = np.uint64
MASK = (1 << 64) - 1

# ---- hashes ------------------------------------------------------------------------------------------------------------------------
K_ADD, K_MUL1, K_MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
K_SALT, K_Y, K_Z = 0xA5A5A5A5DEADBEEF, 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F
K_MATERIAL, K_OCTAVE = 0x51ED270B7F4A7C15, 0x632BE59BD9B4E019


def _u64(a):
    """A two's-complement view of integers as uint64 ((uint64_t)a of a long)."""
    a = np.asarray(a)
    if a.dtype == np.uint64:
        return a
    return a.astype(np.int64).view(np.uint64)


def mix64(x):
    """splitmix64 finaliser on uint64 arrays, wrapping."""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=U64) + U64(K_ADD)
        x = (x ^ (x >> U64(30))) * U64(K_MUL1)
        x = (x ^ (x >> U64(27))) * U64(K_MUL2)
        return x ^ (x >> U64(31))


def hash3(seed, a, b, c):
    """hash3(seed, a, b, c) of world.cpp; seed a Python int, a, b, c integer arrays (broadcast)."""
    with np.errstate(over="ignore"):
        h = mix64(np.array((int(seed) & MASK) ^ K_SALT, dtype=U64))
        h = mix64(h ^ _u64(a))
        h = mix64(h ^ _u64(b) * U64(K_Y))
        return mix64(h ^ _u64(c) * U64(K_Z))


# ---- noise -------------------------------------------------------------------------------------------------------------------------
K_DIR = np.array([
    [1.0, 0.0], [0.9238795325, 0.3826834324], [0.7071067812, 0.7071067812], [0.3826834324, 0.9238795325],
    [0.0, 1.0], [-0.3826834324, 0.9238795325], [-0.7071067812, 0.7071067812], [-0.9238795325, 0.3826834324],
    [-1.0, 0.0], [-0.9238795325, -0.3826834324], [-0.7071067812, -0.7071067812], [-0.3826834324, -0.9238795325],
    [0.0, -1.0], [0.3826834324, -0.9238795325], [0.7071067812, -0.7071067812], [0.9238795325, -0.3826834324]], dtype=np.float64)


def gradient_noise(x, y, seed):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    fx, fy = np.floor(x), np.floor(y)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    tx, ty = x - fx, y - fy

    def corner(cx, cy, dx, dy):
        g = K_DIR[(hash3(seed, cx, cy, np.int64(0)) & U64(15)).astype(np.intp)]
        return g[..., 0] * dx + g[..., 1] * dy

    def fade(t):
        return t * t * t * (t * (t * 6.0 - 15.0) + 10.0)

    n00, n10 = corner(ix, iy, tx, ty), corner(ix + 1, iy, tx - 1.0, ty)
    n01, n11 = corner(ix, iy + 1, tx, ty - 1.0), corner(ix + 1, iy + 1, tx - 1.0, ty - 1.0)
    u, v = fade(tx), fade(ty)
    a, b = n00 + (n10 - n00) * u, n01 + (n11 - n01) * u
    return (a + (b - a) * v) * 1.4142135623730951


def basic_multi(x, y, seed):
    px, py = np.asarray(x, np.float64) * 2.0, np.asarray(y, np.float64) * 2.0
    amp, total = 1.0, 0.0
    for o in range(6):
        total = total + gradient_noise(px, py, (int(seed) + o * K_OCTAVE) & MASK) * amp
        px, py, amp = px * 2.0, py * 2.0, amp * 0.5
    return total * 0.5


def get_noise(x, y, seed):
    return basic_multi(x, y, seed) * 0.5 + 0.5


def mountain_noise2(x, y, seed):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    d = 0.2
    left, right = get_noise(x - d, y, seed), get_noise(x + d, y, seed)
    up, down = get_noise(x, y - d, seed), get_noise(x, y + d, seed)
    dx, dy = (right - left) / (d * 2.0), (down - up) / (d * 2.0)
    slope = np.sqrt(dx * dx + dy * dy)
    base = get_noise(x, y, seed)
    eroded = base + (1.0 - slope) * 0.7
    eroded = np.where(eroded < 0.0, 0.0, eroded)
    return np.power(eroded / 1.5, 2.6)


K_SCALE = 600.0


def terrain_height(x, y, seed):
    """(height int64, value before truncation float64) of the columns (x, y): integer arrays, broadcast together."""
    x, y = np.broadcast_arrays(np.asarray(x, np.int64), np.asarray(y, np.int64))
    m = mountain_noise2(x.astype(np.float64) / K_SCALE, y.astype(np.float64) / K_SCALE, seed)
    v = m * K_SCALE * 0.2 + 10.0
    return np.trunc(v).astype(np.int64), v


def ulps_to_integer(v):
    """The distance of each value to the nearest integer, in units of that value's ULP."""
    v = np.asarray(v, np.float64)
    return np.abs(v - np.rint(v)) / np.spacing(np.abs(v))


# ---- materials and chunks ----------------------------------------------------------------------------------------------------------
GRASS_ID, DIRT_ID, ROCK_ID = 2, 5, 6
_ALBEDO = {GRASS_ID: (39, 110, 61), DIRT_ID: (62, 27, 22), ROCK_ID: (110, 116, 115)}   # MATERIALS[] of world.cpp, all solid


def material_word(material_id):
    """Material::pack of a solid material: albedo << 14 | << 7 | solid << 15."""
    r, g, b = _ALBEDO[int(material_id)]
    return (r << 14 | g << 7 | b) | (1 << 15)


def material_for_height(seed, x, y, z):
    """Material id (2 grass, 5 dirt, 6 rock) of a solid voxel; integer arrays, broadcast together."""
    x, y, z = np.broadcast_arrays(np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(z, np.int64))
    roll = (hash3((int(seed) & MASK) ^ K_MATERIAL, x, y, z) >> U64(16)).astype(np.uint32).astype(np.int64)
    low = np.where(roll % 60 < z - 20, DIRT_ID, GRASS_ID)
    high = np.where(roll % 80 < z - 80, ROCK_ID, DIRT_ID)
    return np.where(z < 20, GRASS_ID, np.where(z < 80, low, np.where(z < 160, high, ROCK_ID))).astype(np.uint8)


def heightmap(cx, cy, seed):
    """Heights and values before truncation of chunk column (cx, cy), each [64 y, 64 x]."""
    return terrain_height(64 * int(cx) + np.arange(64)[None, :], 64 * int(cy) + np.arange(64)[:, None], seed)


def chunk(cx, cy, cz, seed, heights=None):
    """(materials u32[64 z, 64 y, 64 x], minefield u8[64, 64, 64]) of generate_chunk followed by pack_into.  heights: the chunk
    column's heightmap where the caller has it already."""
    from tests.test_terrain_gen_contract import minefield_from_heights
    h = heightmap(cx, cy, seed)[0] if heights is None else heights
    oz = 64 * int(cz)
    if oz + 64 < 12:   # a deep chunk is solid grass whatever the heightmap says
        return np.full((64, 64, 64), material_word(GRASS_ID), np.uint32), np.zeros((64, 64, 64), np.uint8)
    z = oz + np.arange(64)[:, None, None]
    solid = z < h[None]
    words = np.zeros(7, np.uint32)
    for i in _ALBEDO:
        words[i] = material_word(i)
    ids = material_for_height(seed, 64 * int(cx) + np.arange(64)[None, None, :], 64 * int(cy) + np.arange(64)[None, :, None], z)
    mats = np.where(solid, words[ids], 0).astype(np.uint32)
    return mats, minefield_from_heights(h, int(cz))


# ---- the inputs of the far-terrain tests --------------------------------------------------------------------------------------------
SEEDS = [0x5EED, 7, 0xC0FFEE0123456789, 0, 2 ** 64 - 1, 1 << 63, 12345]
WINDOWS = [(-128, -128), (2 ** 31 - 256, -2 ** 31), (-2 ** 31, 2 ** 31 - 256), (999999888, -1000000000), (1975296, -1580240),
           (-1073741872, 1073741840)]
MARGIN_ULPS = 2.0 ** 20

# whole regions at R = 256: every window and every seed at least once
REGION_CASES = [(WINDOWS[0], SEEDS[3]), (WINDOWS[1], SEEDS[0]), (WINDOWS[2], SEEDS[1]), (WINDOWS[3], SEEDS[2]),
                (WINDOWS[4], SEEDS[4]), (WINDOWS[5], SEEDS[5]), (WINDOWS[1], SEEDS[6]), (WINDOWS[5], SEEDS[6])]
TALL = ((75355856, -1484678736), 7)            # the window where columns reach into chunk layer cz = 2
# z at the ends of int32 and around the deep rule: (x, y) windows and seeds of REGION_CASES
Z_CASES = [(REGION_CASES[1], 2 ** 31 - 256), (REGION_CASES[2], -2 ** 31), (REGION_CASES[5], -64 - 16), (REGION_CASES[6], -16)]
SLAB_LO, SLAB_SEED = (2 ** 31 - 256 - 64, -2 ** 31 + 48, -144), SEEDS[4]
SLAB_X_STEPS, SLAB_Y_STEPS = 4, 3              # the fourth x slab is the one that ends exactly at 2^31


def box_windows(R):
    """The two windows of the R = 512 / 1024 box test with their seeds; the second is unaligned on all three axes."""
    return [((2 ** 31 - R, -2 ** 31, -R // 2), SEEDS[2]), ((-1073741872, 1073741840, -R // 2 + 16), SEEDS[5])]


def box_chunks(lo, R):
    """Eight whole world chunks of the window: the first and last whole ones, four cut by the surface, one deep, one all air."""
    g = [v // 64 for v in lo]
    n = R // 64
    return [(g[0] + 1, g[1] + 1, g[2] + 1), (g[0] + n - 1, g[1] + n - 1, g[2] + n - 1),
            (g[0] + 2, g[1] + n - 2, 0), (g[0] + n - 1, g[1] + 1, 1), (g[0] + 1, g[1] + n - 1, 0), (g[0] + n // 2, g[1] + n // 2, 1),
            (g[0] + n - 2, g[1] + 3, -1), (g[0] + 3, g[1] + 2, n // 2 - 1)]


def wrap_boxes(lo, R):
    """Two texel boxes (t0, size) of an unaligned window across the texel wrap (texel (lo + R/2) mod R holds the window's first
    voxel, the texel before it the last): one across it on all three axes, one across it in x and y at the surface."""
    size = (24, 64, 40)
    tw = [(lo[a] + R // 2) % R for a in range(3)]
    all_axes = tuple(max(0, tw[a] - size[a] // 2) for a in range(3))
    surface = (all_axes[0], all_axes[1], (0 - lo[2] + tw[2]) % R)     # world z 0..40
    return [(all_axes, size), (surface, size)]


def box_world_coords(lo, R, t0, size):
    """World coordinates, per axis, of the texels t0 .. t0 + size of the window at lo."""
    return [lo[a] + ((np.arange(t0[a], t0[a] + size[a]) - lo[a] - R // 2) % R) for a in range(3)]


def gpu_columns():
    """Every column a test of tests/test_gpu_terrain_far.py compares, as (what, seed, xs, ys): the columns xs x ys."""
    out = []
    for (x, y), seed in REGION_CASES + [TALL]:
        out.append(("region (%d, %d)" % (x, y), seed, x + np.arange(256), y + np.arange(256)))
    x, y, _ = SLAB_LO
    out.append(("x slabs", SLAB_SEED, x + np.arange(256 + 16 * SLAB_X_STEPS), y + np.arange(256)))
    out.append(("y slabs", SLAB_SEED, x + np.arange(256), y - 16 * SLAB_Y_STEPS + np.arange(256 + 16 * SLAB_Y_STEPS)))
    for R in (512, 1024):
        for i, (lo, seed) in enumerate(box_windows(R)):
            for cx, cy, _ in box_chunks(lo, R):
                out.append(("R %d chunk column (%d, %d)" % (R, cx, cy), seed, 64 * cx + np.arange(64), 64 * cy + np.arange(64)))
            if i == 1:
                for t0, size in wrap_boxes(lo, R):
                    v = box_world_coords(lo, R, t0, size)
                    out.append(("R %d box at texel %s" % (R, t0), seed, v[0], v[1]))
    # the edge-of-int32 box of test_rejections_change_nothing (tests/test_gpu_terrain_gen.py)
    out.append(("edge box", SEEDS[0], 2 ** 31 - 64 + np.arange(64), -2 ** 31 + np.arange(64)))
    return out
