"""The named cases and the parameter table of the detach tests (tests/test_detach_voxels_contract.py judges them with the two
restatements, tests/test_gpu_detach_voxels.py runs them on the device, tests/test_detach_voxels_host.py hands the table to the host's
checks).

The world is tests/emit_particles_sets.py's: solid below texel z = 128 with a different random word in every voxel, air above.  A case
places its voxels in that air through tests/voxel_edits.py and names the box; voxels meant to anchor by material carry 0xA7 in the top
byte of their word, all others 0x5A, and MASK selects by that byte.  The chunk faces a case can straddle in the air are x = 64, y = 64
and z = 192."""
import numpy as np

from tests import detach_voxels_ref as ref
from tests import emit_particles_sets as es
from tests import voxel_edits as ve

R = 256
BODY, ANCHOR = 0x5A000000, 0xA7000000
MASK = dict(anchor_mask=0xFF000000, anchor_value=ANCHOR)
AIR = 0x00A1A1A1                                            # air_material of the cases: no voxel of the world holds it
LO_X, HI_X, LO_Y, HI_Y, LO_Z, HI_Z = ref.FACE_LO_X, ref.FACE_HI_X, ref.FACE_LO_Y, ref.FACE_HI_Y, ref.FACE_LO_Z, ref.FACE_HI_Z
BOTH = ref.CARVE | ref.CAPTURE


def world():
    return es.world()


def place(mats, mine, voxels):
    """Occupies the texels [(x, y, z, word)] of (mats, mine) in place."""
    v = np.asarray(voxels, dtype=np.int64).reshape(-1, 4)
    if len(v):
        ve.apply_edits(mats, mine, v[:, :3], v[:, 3].astype(np.uint32), np.ones(len(v), bool))


def _case(voxels, p, **expect):
    return dict(voxels=voxels, p=p, expect=expect)


def case_world(case):
    """(mats, mine) of a case before the call: new arrays."""
    mats, mine = (a.copy() for a in world())
    place(mats, mine, case["voxels"])
    return mats, mine


def cells(xs, ys, zs, kind=BODY, first=0):
    """The voxels of the box xs x ys x zs (each an int or an iterable), numbered from `first` in the low bits of the word."""
    xs, ys, zs = ([v] if isinstance(v, int) else list(v) for v in (xs, ys, zs))
    out = []
    for z in zs:
        for y in ys:
            for x in xs:
                out.append((x, y, z, kind | (first + len(out))))
    return out


def path(points, kind=BODY, first=0):
    """The voxels of an axis-parallel polyline through `points` (x, y, z), each once."""
    seen, out = set(), []
    for a, b in zip(points[:-1], points[1:]):
        n = max(abs(b[k] - a[k]) for k in range(3))
        for i in range(n + 1):
            c = tuple(a[k] + (b[k] - a[k]) * i // max(n, 1) for k in range(3))
            if c not in seen:
                seen.add(c)
                out.append(c + (kind | (first + len(out)),))
    return out


def serpentine(x0, x1, y0, y1, z, kind=BODY, first=0):
    """A corridor one cell wide that runs along x, steps two cells in y and runs back, from (x0, y0) until y1 is passed."""
    pts, y, left = [], y0, True
    while y <= y1:
        pts += [(x0, y, z), (x1, y, z)] if left else [(x1, y, z), (x0, y, z)]
        left, y = not left, y + 2
    return path(pts, kind, first)


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------------
ONE = (70, 70, 140)
WORD_BOX = ((5, 70, 132), (37, 90, 150))                   # inside one chunk, x not aligned to 64: a pillar on the floor, a floating bar
WORD = cells(20, 80, range(132, 145)) + cells(range(6, 37), 75, 148, first=100) + cells(5, 90, 150, first=200) + cells(37, 70, 132, first=300)
STUBS_BOX = ((70, 70, 134), (90, 92, 160))                 # 21 x 23 x 27: one stub against each face, none touching another
STUBS = {LO_X: cells((70, 71), 80, 140), HI_X: cells((89, 90), 82, 150, first=10), LO_Y: cells(80, (70, 71), 145, first=20),
         HI_Y: cells(78, (91, 92), 155, first=30), LO_Z: cells(84, 86, (134, 135), first=40), HI_Z: cells(76, 76, (159, 160), first=50)}
EDGE = cells(range(70, 74), range(70, 74), 140, ANCHOR) + cells(range(74, 78), range(74, 78), 141, first=100)         # touch at a corner
EDGE2 = cells(range(70, 74), range(70, 74), 140, ANCHOR) + cells(range(74, 78), range(70, 74), 141, first=100)        # ... along an edge
SNAKE = serpentine(66, 126, 66, 126, 133)
SNAKE[0] = SNAKE[0][:3] + (ANCHOR,)                          # its first cell anchors; a short bar beside it does not
SNAKE_BOX = ((65, 65, 132), (127, 127, 135))
# leaves the chunk x < 64 and re-enters it twice: segments in chunk 0, 1, 0, 1, 0 of x
REENTER = path([(50, 70, 140), (66, 70, 140), (66, 74, 140), (60, 74, 140), (60, 78, 140), (67, 78, 140), (67, 82, 140), (58, 82, 140), (58, 86, 140)])
REENTER[0] = REENTER[0][:3] + (ANCHOR,)
REENTER_BOX = ((48, 68, 138), (70, 88, 142))


def bar(axis, lo, hi, at, kind=BODY, first=0):
    """A bar from lo to hi along `axis` through the point `at` (its coordinate on `axis` is ignored)."""
    r = [at[0], at[1], at[2]]
    r[axis] = range(lo, hi + 1)
    return cells(r[0], r[1], r[2], kind, first)


def straddle(axis):
    """A box 60..70 (188..198 in z) across the chunk face of `axis`: a bar across the face that starts on the low face of the axis
    (anchored there) and one across it that touches no face."""
    lo, hi = [70, 70, 132], [80, 80, 142]
    lo[axis], hi[axis] = (188, 198) if axis == 2 else (60, 70)
    at = [74, 74, 136]
    free = [77, 77, 139]
    v = bar(axis, lo[axis], hi[axis] - 2, at) + bar(axis, lo[axis] + 2, hi[axis] - 1, free, first=100)
    return _case(v, ref.params(lo, hi, BOTH, 1 << (2 * axis), AIR), detached=hi[axis] - lo[axis] - 2, supported=hi[axis] - lo[axis] - 1)


RANDOM_LO = (40, 40, 168)


def random_case(seed=9):
    """A 40 % fill of 48^3 texels across 2 x 2 x 2 chunks (x and y from 40, z from 168), anchored at the low z face."""
    rng = np.random.default_rng(seed)
    lo = RANDOM_LO
    fill = rng.random((48, 48, 48)) < 0.4
    z, y, x = np.nonzero(fill)
    voxels = np.stack([x + lo[0], y + lo[1], z + lo[2], BODY | np.arange(len(z))], axis=1)
    return _case(voxels, ref.params(lo, tuple(v + 47 for v in lo), BOTH, LO_Z, AIR))


def cases():
    out = {
        "one cell, occupied, anchored": _case(cells(*ONE), ref.params(ONE, ONE, BOTH, LO_Z, AIR), detached=0, supported=1, passes=1),
        "one cell, occupied, free": _case(cells(*ONE), ref.params(ONE, ONE, BOTH, 0, AIR), detached=1, supported=0, passes=1, chunks=1),
        "one cell, empty, anchored": _case([], ref.params(ONE, ONE, BOTH, 63, AIR), detached=0, supported=0, passes=1),
        "one cell, empty, free": _case([], ref.params(ONE, ONE, BOTH, 0, AIR), detached=0, supported=0, passes=1),
        "inside one chunk off the word grid": _case(WORD, ref.params(*WORD_BOX, BOTH, LO_Z, AIR), detached=32, supported=14, passes=2, chunks=1),
        "straddles x = 64": straddle(0),
        "straddles y = 64": straddle(1),
        "straddles z = 192": straddle(2),
        "straddles three faces": _case(path([(60, 60, 188), (60, 60, 195), (68, 60, 195), (68, 69, 195), (68, 69, 198)]) +
                                       path([(62, 62, 190), (66, 62, 190), (66, 66, 190), (66, 66, 193)], first=100),
                                       ref.params((60, 60, 188), (70, 70, 198), BOTH, LO_Z, AIR), detached=5 + 4 + 3, supported=8 + 8 + 9 + 3),
        "touch at a corner": _case(EDGE, ref.params((68, 68, 138), (80, 80, 143), BOTH | ref.ANCHOR_MATERIAL, 0, AIR, **MASK),
                                   detached=16, supported=16, passes=1, chunks=1),
        "touch along an edge": _case(EDGE2, ref.params((68, 68, 138), (80, 80, 143), BOTH | ref.ANCHOR_MATERIAL, 0, AIR, **MASK),
                                     detached=16, supported=16, passes=1, chunks=1),
        "serpentine": _case(SNAKE + cells(range(70, 80), 100, 135, first=5000), ref.params(*SNAKE_BOX, BOTH | ref.ANCHOR_MATERIAL, 0, AIR, **MASK),
                            detached=10, supported=len(SNAKE), passes=2, chunks=1),
        "re-enters a chunk twice": _case(REENTER + cells(69, 88, 142, first=900), ref.params(*REENTER_BOX, BOTH | ref.ANCHOR_MATERIAL, 0, AIR, **MASK),
                                         detached=1, supported=len(REENTER), passes=6, chunks=1),
        "no anchors": _case(sum(STUBS.values(), []), ref.params(*STUBS_BOX, BOTH, 0, AIR), detached=12, supported=0, passes=1, chunks=1),
        "the material anchor alone": _case(WORD + cells(20, 75, 148, ANCHOR, 700), ref.params(*WORD_BOX, BOTH | ref.ANCHOR_MATERIAL, 0, AIR, **MASK),
                                           detached=13 + 2, supported=31, passes=2, chunks=1),
        "against a face that does not anchor": _case(sum(STUBS.values(), []), ref.params(*STUBS_BOX, BOTH, LO_Z, AIR), detached=10, supported=2, passes=2),
        "outside the region": _case(cells(range(0, 6), 100, 140) + cells(range(2, 8), 104, 140, first=10),
                                    ref.params((-10, 98, 138), (9, 106, 142), BOTH, LO_X, AIR), detached=6, supported=6, passes=2, chunks=1),
        "random 40 % over eight chunks": random_case(),
    }
    for face, name in ((LO_X, "low x"), (HI_X, "high x"), (LO_Y, "low y"), (HI_Y, "high y"), (LO_Z, "low z"), (HI_Z, "high z")):
        out["anchor face " + name] = _case(sum(STUBS.values(), []), ref.params(*STUBS_BOX, BOTH, face, AIR), detached=10, supported=2, passes=2, chunks=1)
    return out


EMPTY_BOX = ref.params((300, 10, 10), (310, 20, 20), BOTH, LO_Z, AIR)


def slab_case(mats, mine):
    """The whole 256^3 region of a world (any) after a slab and four trenches were carved out of it: (mats, mine) carved — new arrays —
    and the parameters.  The slab z = 96..99 under x, y = 64..191 and the trenches round that block up to the sky cut what stands
    on it loose: one body over 2 x 2 chunks and more than one chunk layer; the low z face anchors."""
    from tests import shape_edits as se
    mats, mine = mats.copy(), mine.copy()
    cuts = [se.box((64, 64, 96), (191, 191, 99), AIR, 0), se.box((64, 64, 96), (65, 191, 255), AIR, 0), se.box((190, 64, 96), (191, 191, 255), AIR, 0),
            se.box((64, 64, 96), (191, 65, 255), AIR, 0), se.box((64, 190, 96), (191, 191, 255), AIR, 0)]
    se.apply_shapes(mats, mine, se.batch(cuts))
    return mats, mine, ref.params((0, 0, 0), (255, 255, 255), BOTH, LO_Z, AIR, max_passes=32)


def params_table():
    """(DETACH_DTYPE[N], bool[N] expected verdicts at R = 256 with a stamp_out given, names)."""
    rows = []

    def add(name, ok, **kw):
        rows.append((name, ok, ref.params(**dict(dict(lo=(10, 20, 30), hi=(40, 55, 70), flags=BOTH, anchor_faces=LO_Z), **kw))))

    add("plain", True)
    add("a query", True, flags=0)
    add("carve alone", True, flags=ref.CARVE)
    add("capture alone", True, flags=ref.CAPTURE)
    add("one texel", True, lo=(7, 7, 7), hi=(7, 7, 7))
    add("the whole region", True, lo=(0, 0, 0), hi=(255, 255, 255))
    add("at the range's ends", True, lo=(-1024, -1024, -1024), hi=(1024, 1024, 1024))
    add("box beyond the region", True, lo=(300, 10, 10), hi=(310, 20, 20))
    add("box below the region", True, lo=(10, -9, 10), hi=(20, -1, 20))
    add("clipped at both faces", True, lo=(-5, 250, 100), hi=(3, 260, 101))
    add("lo beyond the range", False, lo=(-1025, 0, 0))
    add("hi beyond the range", False, hi=(40, 50, 1025))
    add("lo above hi", False, lo=(10, 56, 30))
    add("flag bit 3", False, flags=BOTH | 8)
    add("flag bit 31", False, flags=0x80000000)
    add("max_passes 0", False, max_passes=0)
    add("max_passes 1", True, max_passes=1)
    add("max_passes 256", True, max_passes=256)
    add("max_passes 257", False, max_passes=257)
    for f in (0, 1, 2, 4, 8, 16, 32, 63):
        add("anchor_faces %d" % f, True, anchor_faces=f)
    add("anchor_faces 64", False, anchor_faces=64)
    add("anchor_faces 255", False, anchor_faces=255)
    add("mask and value", True, flags=BOTH | ref.ANCHOR_MATERIAL, **MASK)
    add("full mask", True, flags=ref.ANCHOR_MATERIAL, anchor_mask=0xFFFFFFFF, anchor_value=0x12345678)
    add("the material flag with mask 0", True, flags=ref.ANCHOR_MATERIAL)
    add("value outside the mask", False, flags=ref.ANCHOR_MATERIAL, anchor_mask=0xFF000000, anchor_value=0x5A000001)
    add("mask without the flag", False, anchor_mask=0xFF000000)
    add("value without the flag", False, anchor_value=1)
    add("air material", True, air_material=0xFFFFFFFF)
    add("reserved0[0]", False, reserved0=(1, 0, 0))
    add("reserved0[1]", False, reserved0=(0, 0x80, 0))
    add("reserved0[2]", False, reserved0=(0, 0, 1))
    table = np.array([r[2] for r in rows], dtype=ref.DETACH_DTYPE)
    return table, np.array([r[1] for r in rows]), [r[0] for r in rows]


# extents that need R = 512 to be judged: a clipped extent of 257 is refused, 256 accepted
EXTENT_ROWS = [(ref.params((100, 0, 0), (355, 10, 10), BOTH, LO_Z), True), (ref.params((100, 0, 0), (356, 10, 10), BOTH, LO_Z), False),
               (ref.params((-50, 0, 0), (255, 10, 600), BOTH, LO_Z), False), (ref.params((-50, 0, 300), (255, 10, 600), BOTH, LO_Z), True)]
