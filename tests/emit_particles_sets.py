"""The worlds, named cases and emitter table of the rt_emit_particles tests.  Test infrastructure.

A case is a dict: emitters (EMIT_DTYPE rows), lr, capacity, next (the cursor's input), max_emit, and `empty` — whether the rules
give N = 0 for it on `world()`.  tests/test_emit_particles_contract.py asserts from the restatement that every other case emits at
least one particle, so that a change of the world cannot hollow out the GPU tests."""
import numpy as np

from raytrace_amd import world as rw
from tests import emit_particles_ref as ref
from tests import scenes
from tests import shape_edits as se

R = 256
LR_SEAM = (40, -24, 8)        # the window's seam lies at texels x = 40, y = 232, z = 8
_WORLD = {}


def world():
    """(mats, mine) of a region that is solid below texel z = 128 except for a few shafts, with blocks floating above; every
    voxel's material word is different, so that a particle shows which voxel it came from.  Built once."""
    if "w" not in _WORLD:
        ids = scenes.floor_ids()
        ids[100:128, 16:24, 8:12] = 0                     # a shaft through the box cases' neighbourhood
        ids[120:128, 60:63, 0:3] = 0                      # ... and one that takes a bite out of the sphere
        ids[128:131, 64:70, 2:6] = 3                      # a block above the floor, inside the sphere's reach
        ids[126:131, 230:236, 250:256] = 5                # solid across z = 128 near the far corner (the seam case)
        mats, mine = rw.region_from_ids(ids)
        mats = mats.reshape(R, R, R) ^ np.random.default_rng(11).integers(0, 2 ** 32, size=(R, R, R), dtype=np.uint32)
        _WORLD["w"] = (np.ascontiguousarray(mats), np.ascontiguousarray(mine.reshape(R, R, R)))
    return _WORLD["w"]


def _e(shape, origin=None, **kw):
    if origin is None:                                     # the shape's centre in world units under lr = 0
        a, b = shape["a"].astype(np.float64), shape["b"].astype(np.float64)
        origin = (a + b + 1) / 2 - R / 2 if shape["kind"] == se.BOX else a / 2 - R / 2
    kw = dict(dict(seed=7, speed=6.0, spread=1.5, drift=(0.0, 0.0, 2.0), half=0.125, life_min=0.5, life_span=2.0, response=3, light=3,
                   emission=0xFF102030), **kw)
    return ref.emitter(shape, origin, **kw)


SPHERE = se.sphere((3, 129, 253), 49)                      # radius 3.5 round voxel (1, 64, 126): a brick edge, a chunk edge, the face x = 0
BOX543 = se.box((9, 18, 101), (13, 21, 103))               # 5 x 4 x 3, aligned to no brick; the shaft takes some of it
SOLID543 = se.box((41, 50, 101), (45, 53, 103))            # the same extent where all 60 voxels are solid
BIG = se.box((70, 70, 110), (81, 81, 117))                 # 1152 solid voxels


def _case(emitters, lr=(0, 0, 0), capacity=4096, next=5, max_emit=None, empty=False):
    return dict(emitters=ref.batch(emitters), lr=tuple(lr), capacity=capacity, next=next, max_emit=capacity if max_emit is None else max_emit,
                empty=empty)


def _tiny():
    """256 one-voxel emitters: a diagonal walk through the floor, every fifth on the voxel before it (emitted twice), a few in air."""
    out = []
    for i in range(256):
        j = i - 1 if i % 5 == 4 else i
        p = (20 + j % 37, 90 + (3 * j) % 41, 127 - (j % 9) + (4 if i % 50 == 0 else 0))
        out.append(_e(se.box(p, p), seed=100 + i, density=256))
    return out


def cases():
    return {
        "sphere": _case([_e(SPHERE)]),
        "one voxel": _case([_e(se.box((10, 10, 100), (10, 10, 100)))]),
        "box 5x4x3": _case([_e(BOX543)]),
        "empty sphere": _case([_e(se.sphere((20, 20, 200), 0))], empty=True),
        "outside": _case([_e(se.box((300, 10, 10), (310, 20, 20)))], empty=True),
        "air": _case([_e(se.box((100, 100, 200), (103, 103, 203)))], empty=True),
        "seam": _case([_e(se.sphere((509, 465, 253), 49), origin=(166.5, 80.0, 7.0)),
                       _e(se.sphere((509 - 2 * R, 465, 253), 49), origin=(166.5, 80.0, 7.0))], lr=LR_SEAM),
        "overlap": _case([_e(SOLID543), _e(se.box((44, 52, 102), (48, 56, 105)), seed=8)]),
        "density 37": _case([_e(BIG, density=37)]),
        "density 256": _case([_e(BIG, density=256)]),
        "256 tiny": _case(_tiny()),
        "wrap": _case([_e(SOLID543)], capacity=64, next=60),
        "cut": _case([_e(SOLID543)], capacity=64, next=3, max_emit=25),
        "next beyond": _case([_e(BOX543)], capacity=64, next=64 + 7),
    }


# ---- the emitter table: valid and invalid records with the verdict the rules give ----------------------------------------------------
def emitter_table():
    """(EMIT_DTYPE[N], bool[N] expected verdicts at R = 256, names)."""
    rows = []

    def add(name, ok, shape=BOX543, **kw):
        e = _e(shape)
        for k, v in kw.items():
            e[k] = v
        rows.append((name, ok, e))

    add("box", True)
    add("sphere", True, SPHERE)
    add("sphere of budget 0", True, se.sphere((20, 20, 200), 0))
    add("box beyond the region", True, se.box((300, 10, 10), (310, 20, 20)))
    add("box at 4R", True, se.box((4 * R, 0, 0), (4 * R, 0, 0)))
    add("box beyond 4R", False, se.box((4 * R + 1, 0, 0), (4 * R + 1, 0, 0)))
    add("box with a > b", False, se.box((5, 5, 5), (4, 5, 5)))
    add("sphere with b1", False, SPHERE, b=(49, 1, 0))
    add("sphere budget above 2^26", False, SPHERE, b=(2 ** 26 + 1, 0, 0))
    add("kind 2", False, kind=2)
    add("response 3", True, response=3)
    add("response 4", False, response=4)
    add("reserved byte", False, reserved0=(0, 1))
    add("reserved word", False, reserved=(0, 1))
    add("density 0", False, density=0)
    add("density 1", True, density=1)
    add("density 256", True, density=256)
    add("density 257", False, density=257)
    add("half 2^-8", True, half=2.0 ** -8)
    add("half below 2^-8", False, half=np.nextafter(np.float32(2.0 ** -8), np.float32(0)))
    add("half 0.5", True, half=0.5)
    add("half above 0.5", False, half=np.nextafter(np.float32(0.5), np.float32(1)))
    add("half nan", False, half=np.nan)
    add("speed 0", True, speed=0.0)
    add("speed 4096", True, speed=4096.0)
    add("speed negative", False, speed=-1.0)
    add("speed above", False, speed=4097.0)
    add("speed inf", False, speed=np.inf)
    add("spread 4096", True, spread=4096.0)
    add("spread negative", False, spread=-0.5)
    add("spread nan", False, spread=np.nan)
    add("drift -4096", True, drift=(0, -4096.0, 0))
    add("drift beyond", False, drift=(0, 0, 4097.0))
    add("drift nan", False, drift=(np.nan, 0, 0))
    add("origin 2^22", True, origin=(2.0 ** 22, -2.0 ** 22, 0))
    add("origin beyond", False, origin=(0, 2.0 ** 22 + 1, 0))
    add("origin inf", False, origin=(0, 0, -np.inf))
    add("life_min inf", True, life_min=np.inf)
    add("life_min 0", False, life_min=0.0)
    add("life_min negative", False, life_min=-1.0)
    add("life_min nan", False, life_min=np.nan)
    add("life_min -inf", False, life_min=-np.inf)
    add("life_span 0", True, life_span=0.0)
    add("life_span 4096", True, life_span=4096.0)
    add("life_span negative", False, life_span=-1.0)
    add("life_span inf", False, life_span=np.inf)
    add("any seed, light, emission", True, seed=0xFFFFFFFF, light=0xFFFFFFFF, emission=0)
    return ref.batch([e for _, _, e in rows]), np.array([ok for _, ok, _ in rows]), [n for n, _, _ in rows]


# windows: (lr, the verdict at R = 256)
WINDOWS = [((0, 0, 0), True), ((2 ** 22 - R, -(2 ** 22 - R), 0), True), ((2 ** 22 - R + 1, 0, 0), False), ((0, 0, -(2 ** 22 - R) - 1), False),
           ((0, -2 ** 31, 0), False)]

# the plans the host test prints: batches by the names of their emitters in the table
PLAN_BATCHES = [["box"], ["sphere"], ["sphere of budget 0"], ["box", "box beyond the region", "sphere", "box at 4R", "density 1"]]
