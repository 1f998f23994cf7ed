"""The named cases and the parameter table of the flow tests (tests/test_flow_voxels_contract.py judges them with the two restatements,
tests/test_gpu_flow_voxels.py runs them on the device, tests/test_flow_voxels_host.py hands the tables to the host's checks).

The world is tests/emit_particles_sets.py's: solid below texel z = 128 with a different random word in every voxel, air above.  A case
places its voxels in that air (or in a room carved out of the ground) through tests/voxel_edits.py and names the box.  WATER voxels
carry 0x5A in the top byte of their word and their level in the low nibble, FIXED ones 0x11 in the top byte, and MASK selects by that
byte; bits 8..23 of a fluid word are a tag the call must keep."""
import numpy as np

from tests import emit_particles_sets as es
from tests import flow_voxels_ref as ref
from tests import shape_edits as se
from tests import voxel_edits as ve

R = 256
WATER, FIXED = 0x5A000000, 0x11000000
MASK = dict(fluid_mask=0xFF000000, fluid_value=WATER)
AIR = 0x00A1A1A0                                            # air_material of the cases: no voxel of the world holds it
SRC = WATER | 0xF                                           # a source's word at level_shift 0


def world():
    return es.world()


def place(mats, mine, voxels):
    """Occupies the texels [(x, y, z, word)] of (mats, mine) in place."""
    v = np.asarray(voxels, dtype=np.int64).reshape(-1, 4)
    ve.apply_edits(mats, mine, v[:, :3], v[:, 3].astype(np.uint32), np.ones(len(v), bool))


def _case(voxels, p, carve=None, **expect):
    return dict(voxels=voxels, carve=carve, p=p, expect=expect)


def case_world(case):
    """(mats, mine) of a case before the call: new arrays."""
    mats, mine = (a.copy() for a in world())
    if case["carve"] is not None:
        se.apply_shapes(mats, mine, se.batch([case["carve"]]))
    place(mats, mine, case["voxels"])
    return mats, mine


def _slab(x0, x1, y0, y1, z, word=FIXED):
    return [(x, y, z, word | ((x * 31 + y) & 0xFF) << 8) for y in range(y0, y1 + 1) for x in range(x0, x1 + 1)]


# ---- the ledge: 12 x 3 x 6 in one chunk.  A ledge four cells long at height 3, a spring on its first cell: a run 7 6 5 4 (the 4 hangs over
# the edge), a fall, and on the floor 7 under the fall, 6 5 4 3 2 1 away from the ledge and 6 5 4 3 back under it ------------------------------
LEDGE_LO, LEDGE_HI = (66, 66, 132), (77, 68, 137)
LEDGE_SOURCE = (66, 67, 136)
LEDGE_TICKS = 15                                            # the fixed point: 4 along the run, 4 down, 6 over the floor, 1 more in the rows beside the spring


def ledge_voxels(source=SRC, fixed=FIXED):
    return _slab(66, 69, 66, 68, 135, fixed) + [LEDGE_SOURCE + (source | 0x00C0DE00,)]


LEDGE_RUN = [14, 7, 6, 5, 4, 0, 0, 0, 0, 0, 0, 0]           # states along x at y = 67, z = 136
LEDGE_FLOOR = [3, 4, 5, 6, 7, 6, 5, 4, 3, 2, 1, 0]          # ... and at z = 132
DRY_TICKS = 24                                              # the ledge's fixed point without its source is dry within these


def ledge(ticks=LEDGE_TICKS, **kw):
    return _case(ledge_voxels(), ref.params(LEDGE_LO, LEDGE_HI, ticks=ticks, air_material=AIR, **dict(MASK, **kw)))


def ledge_dry(ticks=DRY_TICKS):
    """The ledge at its fixed point with the source taken away (the voxels are placed as the fixed point's states say)."""
    case = ledge()
    mats, mine = case_world(case)
    _, _, s = ref.flow(mats, mine, case["p"])
    z, y, x = np.nonzero((s >= 1) & (s < ref.SOURCE))
    wet = [(int(a) + LEDGE_LO[0], int(b) + LEDGE_LO[1], int(c) + LEDGE_LO[2], WATER | 0x00BEEF00 | int(s[c, b, a])) for a, b, c in zip(x, y, z)]
    return _case(_slab(66, 69, 66, 68, 135) + wet, ref.params(LEDGE_LO, LEDGE_HI, ticks=ticks, air_material=AIR, **MASK))


# ---- a room carved over the chunk corner at (64, 64, 64): a spring on a platform in the upper chunks, the floor in the lower ones ----------
CORNER_LO, CORNER_HI = (40, 50, 56), (87, 77, 71)           # extent 48 x 28 x 16
CORNER_CARVE = se.box(CORNER_LO, CORNER_HI, 0x0C0C0C0C, 0)


def corner(ticks=30):
    voxels = _slab(60, 68, 60, 68, 65) + [(64, 64, 66, SRC | 0x00123400), (50, 70, 60, SRC), (52, 70, 59, FIXED)]
    return _case(voxels, ref.params(CORNER_LO, CORNER_HI, ticks=ticks, air_material=AIR, **MASK), CORNER_CARVE)


# ---- the field elsewhere in the word, the shortest and the longest reach -------------------------------------------------------------------
def variant(max_level, level_shift):
    """The ledge with the level field at `level_shift` (the mask moves out of its way) and `max_level`."""
    mask, water, fixed = (0x00FF0000, 0x005A0000, 0x00110000) if level_shift >= 20 else (0xFF000000, WATER, FIXED)
    voxels = [(x, y, z, (w & 0xFFFF00) >> 8 | fixed) for x, y, z, w in _slab(66, 69, 66, 68, 135, 0)]
    voxels += [LEDGE_SOURCE + (water | (0xF << level_shift) & 0xFFFFFFFF,), (75, 67, 132, water | (14 << level_shift) & 0xFFFFFFFF)]
    return _case(voxels, ref.params(LEDGE_LO, LEDGE_HI, mask, water, ticks=20, air_material=AIR, level_shift=level_shift, max_level=max_level))


# ---- a box the region's edge clips ------------------------------------------------------------------------------------------------------------
def clipped(ticks=12):
    voxels = [(2, 253, 130, FIXED), (2, 253, 131, SRC), (0, 255, 128, WATER | 3), (5, 250, 129, WATER | 9)]
    return _case(voxels, ref.params((-5, 249, 128), (6, 262, 133), ticks=ticks, air_material=AIR, **MASK))


def random_small(seed=3, ext=(13, 11, 9), ticks=5):
    """A random box over the floor: fixed cells, sources, flowing cells of every raw level (above max_level and 14 included)."""
    rng = np.random.default_rng(seed)
    lo = (70, 80, 128)
    n = ext[0] * ext[1] * ext[2]
    kind = rng.choice(4, size=n, p=[0.6, 0.2, 0.17, 0.03])                     # empty, fixed, flowing, source
    x, y, z = (np.arange(n) % ext[0], np.arange(n) // ext[0] % ext[1], np.arange(n) // (ext[0] * ext[1]))
    word = np.where(kind == 1, FIXED | np.arange(n), np.where(kind == 2, WATER | rng.integers(0, 15, n) | np.arange(n) << 8, SRC))
    sel = kind != 0
    voxels = np.stack([x + lo[0], y + lo[1], z + lo[2], word], axis=1)[sel]
    return _case(voxels, ref.params(lo, tuple(lo[k] + ext[k] - 1 for k in range(3)), ticks=ticks, air_material=AIR, max_level=7, **MASK))


def cases():
    return {
        "ledge": ledge(),
        "ledge, one tick": ledge(1),
        "ledge, three ticks": ledge(3),
        "ledge, fourteen ticks": ledge(14),
        "ledge, forty ticks": ledge(40),
        "ledge without its source": ledge_dry(),
        "chunk corner": corner(),
        "max_level 1": variant(1, 0),
        "max_level 13": variant(13, 0),
        "level_shift 28": variant(7, 28),
        "clipped by the region": clipped(),
        "random 13 x 11 x 9": random_small(),
    }


# ---- more than two tiles on every axis, on arbitrary minefield values --------------------------------------------------------------------
TILES_LO, TILES_EXT = (30, 100, 40), (70, 36, 35)           # 3 x 3 x 3 tiles of 32 x 16 x 16; chunks x 0..1, y 1..2, z 0..1


def tiles_world(mats, mine, ticks, seed=9):
    """(mats, mine, p): copies of an arbitrary world (tests/adversarial_worlds.py) whose box holds random fixed cells, sources and
    flowing cells of every raw level; the unoccupied cells keep the arbitrary non-zero bytes they have (a 0 becomes 3)."""
    rng = np.random.default_rng(seed)
    mats, mine = mats.copy(), mine.copy()
    sl = tuple(slice(TILES_LO[k], TILES_LO[k] + TILES_EXT[k]) for k in (2, 1, 0))
    shape = mine[sl].shape
    kind = rng.choice(4, size=shape, p=[0.72, 0.16, 0.1, 0.02])                  # empty, fixed, flowing, source
    fixed_word = rng.integers(0, 1 << 32, size=shape, dtype=np.uint32)
    fixed_word = np.where(fixed_word >> 24 == 0x5A, fixed_word ^ 0x01000000, fixed_word)
    flowing = (WATER | rng.integers(0, 15, size=shape) | rng.integers(0, 1 << 16, size=shape) << 8).astype(np.uint32)
    mats[sl] = np.where(kind == 1, fixed_word, np.where(kind == 2, flowing, np.where(kind == 3, np.uint32(SRC), mats[sl])))
    mine[sl] = np.where(kind != 0, 0, np.where(mine[sl] == 0, 3, mine[sl]))
    hi = tuple(TILES_LO[k] + TILES_EXT[k] - 1 for k in range(3))
    return mats, mine, ref.params(TILES_LO, hi, ticks=ticks, air_material=AIR, max_level=7, **MASK)


def params_table():
    """(FLOW_DTYPE[N], bool[N] expected verdicts at R = 256, names)."""
    rows = []

    def add(name, ok, **kw):
        rows.append((name, ok, ref.params(**dict(dict(lo=(10, 20, 30), hi=(40, 55, 70), **MASK), **kw))))

    add("plain", True)
    add("one texel", True, lo=(7, 7, 7), hi=(7, 7, 7))
    add("the whole region", True, lo=(0, 0, 0), hi=(255, 255, 255))
    add("eight chunks", True, lo=(40, 40, 40), hi=(90, 90, 90))
    add("at the range's ends", True, lo=(-1024, -1024, -1024), hi=(1024, 1024, 1024))
    add("box beyond the region", True, lo=(300, 10, 10), hi=(310, 20, 20))
    add("box below the region", True, lo=(10, -9, 10), hi=(20, -1, 20))
    add("clipped at both faces", True, lo=(-5, 250, 100), hi=(3, 260, 101))
    add("256 x 16 x 8", True, lo=(0, 3, 5), hi=(255, 18, 12))
    add("lo beyond the range", False, lo=(-1025, 0, 0))
    add("hi beyond the range", False, hi=(40, 55, 1025))
    add("lo above hi", False, lo=(10, 56, 30))
    add("ticks 0", False, ticks=0)
    add("ticks 1", True, ticks=1)
    add("ticks 256", True, ticks=256)
    add("ticks 257", False, ticks=257)
    add("level_shift 28", True, level_shift=28, fluid_mask=0x00FF0000, fluid_value=0x005A0000)
    add("level_shift 29", False, level_shift=29, fluid_mask=0x00FF0000, fluid_value=0x005A0000)
    add("level_shift 255", False, level_shift=255, fluid_mask=0x00FF0000, fluid_value=0x005A0000)
    add("max_level 0", False, max_level=0)
    add("max_level 1", True, max_level=1)
    add("max_level 13", True, max_level=13)
    add("max_level 14", False, max_level=14)
    add("no mask", False, fluid_mask=0, fluid_value=0)
    add("mask in the field", False, fluid_mask=0xFF000001)
    add("mask in the shifted field", False, fluid_mask=0xFF000100, level_shift=8)
    add("mask beside the shifted field", True, fluid_mask=0xFF000001, level_shift=8)
    add("value outside the mask", False, fluid_value=WATER | 0x10)
    add("word in the field", False, fluid_word=WATER | 1)
    add("word fails the test", False, fluid_word=0x5B000000)
    add("word with other bits", True, fluid_word=WATER | 0x00777700)
    add("full mask but the field", True, fluid_mask=0xFFFFFFF0, fluid_value=0x12345670)
    add("air material", True, air_material=0xFFFFFFFF)
    add("reserved0", False, reserved0=1)
    add("reserved1[0]", False, reserved1=(1, 0))
    add("reserved1[1]", False, reserved1=(0, 0x80))
    add("reserved2[0]", False, reserved2=(1, 0, 0))
    add("reserved2[2]", False, reserved2=(0, 0, 1 << 31))
    table = np.array([r[2] for r in rows], dtype=ref.FLOW_DTYPE)
    return table, np.array([r[1] for r in rows]), [r[0] for r in rows]


def extent_table():
    """Rows (lo, hi, logr, ok): the clipped extent's limit needs a region above 256."""
    return [((0, 0, 0), (255, 255, 255), 9, True), ((0, 0, 0), (256, 15, 7), 9, False), ((100, 5, 5), (355, 20, 12), 9, True), ((100, 5, 5), (356, 20, 12), 9, False),
            ((5, 5, 600), (20, 12, 1100), 10, False), ((5, 5, 800), (20, 12, 1100), 10, True), ((-300, 0, 0), (255, 15, 7), 9, True), ((-300, 0, 0), (256, 15, 7), 9, False)]


GROUPS = (1, 2, 4, 8)
