"""The named cases and the parameter table of the settle tests (tests/test_settle_voxels_contract.py judges them with the restatement,
tests/test_gpu_settle_voxels.py runs them on the device, tests/test_settle_voxels_host.py hands the table to the host's checks).

The world is tests/emit_particles_sets.py's: solid below texel z = 128 with a different random word in every voxel, air above.  A case
places its voxels in that air through tests/voxel_edits.py and names the box; LOOSE voxels carry 0x5A in the top byte of their word,
FIXED ones 0x11, and MASK selects by that byte."""
import numpy as np

from tests import emit_particles_sets as es
from tests import settle_voxels_ref as ref
from tests import shape_edits as se
from tests import voxel_edits as ve

R = 256
LOOSE, FIXED = 0x5A000000, 0x11000000
MASK = dict(loose_mask=0xFF000000, loose_value=LOOSE)
AIR = 0x00A1A1A1                                            # air_material of the cases: no voxel of the world holds it


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


def _col(x, y, zs, kind=LOOSE, first=0):
    return [(x, y, z, kind | (first + i)) for i, z in enumerate(zs)]


STACK = _col(70, 70, (134, 135, 138, 141, 142))            # over the box floor z = 132: gaps of 2, 0, 2, 2, 0 cells
STACK_BOX = ((68, 68, 132), (72, 72, 145))
SPLIT = _col(70, 70, (133, 139, 140), first=0) + _col(70, 70, (136,), FIXED, first=8) + _col(70, 70, (137,), first=9)
BOUNDARY = (_col(101, 101, (66, 67)) + _col(102, 101, (70,), first=2) + _col(102, 101, (66,), FIXED, first=3) + _col(103, 101, (62,), first=4))
BOUNDARY_CARVE = se.box((100, 100, 56), (104, 104, 75), 0x0C0C0C0C, 0)
FIXTURE = (_col(70, 70, (134, 137)) + _col(71, 70, (133,), first=2) + _col(73, 72, (139,), FIXED, first=3) + _col(74, 72, (139,), first=4) +
           _col(70, 73, (136,), first=5) + _col(76, 66, (141,), first=6) + _col(72, 72, (135, 136), first=7) + _col(72, 71, (135,), FIXED, first=9))
FIXTURE_BOX = ((66, 66, 132), (77, 75, 141))               # 12 x 10 x 10: no two extents alike


def random_case(seed=5):
    """64 x 64 columns, 32 cells high, over two chunks in x: a column is empty, sparse or dense, a voxel loose or (one in eight) fixed,
    so that a wave holds lanes that move many voxels, lanes that move few and lanes that move none."""
    rng = np.random.default_rng(seed)
    lo, hi = (96, 64, 130), (159, 127, 161)
    density = rng.choice([0.0, 0.0, 0.1, 0.5, 0.9], size=(64, 64))
    fill = rng.random((32, 64, 64)) < density[None]
    z, y, x = np.nonzero(fill)
    kind = np.where(rng.random(len(z)) < 0.125, FIXED, LOOSE)
    voxels = np.stack([x + lo[0], y + lo[1], z + lo[2], kind | np.arange(len(z))], axis=1)
    return _case(voxels, ref.params(lo, hi, 5, AIR, **MASK))


def cases():
    return {
        "onto the box floor": _case(_col(70, 70, (140,)), ref.params(*STACK_BOX, air_material=AIR), moved=1, falling=0, distance=8, chunks=1),
        "onto a fixed voxel": _case(_col(70, 70, (140,)) + _col(70, 70, (134,), FIXED, 1), ref.params(*STACK_BOX, air_material=AIR, **MASK),
                                    moved=1, falling=0, distance=5, chunks=1),
        "onto texel 0": _case(_col(5, 70, (140,)), ref.params((-3, 68, 138), (9, 72, 142), air_material=AIR, axis=0), moved=1, falling=0, distance=5, chunks=1),
        "at rest": _case(_col(70, 70, (132,)), ref.params(*STACK_BOX, air_material=AIR), moved=0, falling=0, distance=0, chunks=0),
        "stack fall 1": _case(STACK, ref.params(*STACK_BOX, 1, AIR), moved=5, falling=5, distance=5, chunks=1),
        "stack fall 3": _case(STACK, ref.params(*STACK_BOX, 3, AIR), moved=5, falling=3, distance=13, chunks=1),
        "stack unlimited": _case(STACK, ref.params(*STACK_BOX, air_material=AIR), moved=5, falling=0, distance=20, chunks=1),
        "split by a fixed voxel": _case(SPLIT, ref.params(*STACK_BOX, air_material=AIR, **MASK), moved=3, falling=0, distance=3, chunks=1),
        "split, every voxel loose": _case(SPLIT, ref.params(*STACK_BOX, air_material=AIR), moved=5, falling=0, distance=15, chunks=1),
        "stack falls by less than its height": _case(_col(70, 70, (134, 135, 136, 137)), ref.params(*STACK_BOX, 2, AIR), moved=4, falling=0, distance=8, chunks=1),
        "chunk boundary": _case(BOUNDARY, ref.params((100, 100, 60), (104, 104, 70), air_material=AIR, **MASK), BOUNDARY_CARVE,
                                moved=4, falling=0, distance=6 + 6 + 3 + 2, chunks=2),
        "one column": _case(_col(70, 70, (140,)) + _col(71, 70, (140,), first=1) + _col(72, 70, (140,), first=2) + _col(71, 71, (140,), first=3),
                            ref.params((71, 70, 132), (71, 70, 145), air_material=AIR), moved=1, falling=0, distance=8, chunks=1),
        "outside the region": _case(_col(3, 66, (250, 252)) + _col(0, 68, (249,), first=2), ref.params((-20, 64, 248), (10, 70, 300), 4, AIR, toward=1),
                                    moved=3, falling=1, distance=4 + 3 + 4, chunks=1),
        "random 64 x 64": random_case(),
    }


AXES = [(axis, toward) for axis in range(3) for toward in range(2)]


def fixture_case(axis, toward):
    return _case(FIXTURE, ref.params(*FIXTURE_BOX, air_material=AIR, axis=axis, toward=toward, **MASK))


EIGHT_WORD = 0xD1CE0001
EIGHT_BOX = ((40, 40, 40), (90, 90, 90))


def eight_chunks_world(mats, mine):
    """(mats, p): a copy of `mats` in which a few occupied voxels of two of the box's eight chunks — (0, 0, 0) and (1, 1, 1) — that have
    a free cell under them carry EIGHT_WORD, and the parameters that make exactly those loose (any world; only material words differ, so
    the minefield keeps whatever values it has)."""
    mats = mats.copy()
    assert not (mats == EIGHT_WORD).any()
    for lo in (40, 64):
        occ = mine[lo:lo + 20, lo:lo + 20, lo:lo + 20] == 0
        z, y, x = np.nonzero(occ[1:] & ~occ[:-1])                              # occupied over a free cell
        assert len(z) >= 8
        pick = np.arange(0, len(z), len(z) // 8)[:8]
        mats[z[pick] + 1 + lo, y[pick] + lo, x[pick] + lo] = EIGHT_WORD
    return mats, ref.params(*EIGHT_BOX, air_material=AIR, loose_mask=0xFFFFFFFF, loose_value=EIGHT_WORD)


def params_table():
    """(SETTLE_DTYPE[N], bool[N] expected verdicts at R = 256, names)."""
    rows = []

    def add(name, ok, **kw):
        rows.append((name, ok, ref.params(**dict(dict(lo=(10, 20, 30), hi=(40, 55, 70)), **kw))))

    add("plain", True)
    add("one texel", True, lo=(7, 7, 7), hi=(7, 7, 7))
    add("the whole region", True, lo=(0, 0, 0), hi=(255, 255, 255))
    add("eight chunks", True, lo=(40, 40, 40), hi=(90, 90, 90))
    add("at the range's ends", True, lo=(-1024, -1024, -1024), hi=(1024, 1024, 1024))
    add("box beyond the region", True, lo=(300, 10, 10), hi=(310, 20, 20))
    add("box below the region", True, lo=(10, -9, 10), hi=(20, -1, 20))
    add("clipped at both faces", True, lo=(-5, 250, 100), hi=(3, 260, 101), axis=1, toward=1)
    add("lo beyond the range", False, lo=(-1025, 0, 0))
    add("hi beyond the range", False, hi=(40, 50, 1025))
    add("lo above hi", False, lo=(10, 56, 30))
    for axis in range(3):
        for toward in range(2):
            add("axis %d toward %d" % (axis, toward), True, axis=axis, toward=toward)
    add("axis 3", False, axis=3)
    add("axis 255", False, axis=255)
    add("toward 2", False, toward=2)
    add("max_fall 0", False, max_fall=0)
    add("max_fall 1", True, max_fall=1)
    add("max_fall 2^32 - 2", True, max_fall=0xFFFFFFFE)
    add("mask and value", True, loose_mask=0xFF000000, loose_value=0x5A000000)
    add("full mask", True, loose_mask=0xFFFFFFFF, loose_value=0x12345678)
    add("mask with value 0", True, loose_mask=0x80000000)
    add("value outside the mask", False, loose_mask=0xFF000000, loose_value=0x5A000001)
    add("value without a mask", False, loose_value=1)
    add("air material", True, air_material=0xFFFFFFFF)
    add("reserved0[0]", False, reserved0=(1, 0))
    add("reserved0[1]", False, reserved0=(0, 0x80))
    add("reserved1", False, reserved1=1)
    table = np.array([r[2] for r in rows], dtype=ref.SETTLE_DTYPE)
    return table, np.array([r[1] for r in rows]), [r[0] for r in rows]
