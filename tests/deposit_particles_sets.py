"""The named cases and the parameter table of the rt_deposit_particles tests.  Test infrastructure.

A case is a dict: p (a DEPOSIT_DTYPE row), states (STATE_DTYPE[N]) and `expect` — the four counts its name promises on
emit_particles_sets.world(), worked out here from how the records were laid out and not from the restatement;
tests/test_deposit_particles_contract.py holds the restatement against them, so that a change of the world cannot hollow out the
GPU tests.  The world is solid below texel z = 128 (world z < 0 under lr = 0) and air above, with every material word different."""
import numpy as np

from tests import deposit_particles_ref as ref
from tests import emit_particles_ref as eref
from tests import emit_particles_sets as es
from tests import particle_step_ref as psr
from tests import shape_edits as se
from tests import sweep_ref as sr
from tests import voxel_edits as ve

R = 256
f32 = np.float32
LR_SEAM = es.LR_SEAM          # the window's seam lies at texels x = 40, y = 232, z = 8
STICK_AT_REST = psr.STICK | 0x40000      # a STICK particle stopped by the floor: contact on z


def world():
    return es.world()


def resting(voxels, flags=STICK_AT_REST, half=0.125, material0=0xA000):
    """STATE_DTYPE[N]: one particle at rest per world voxel (x, y, z) of `voxels` — a cube of half edge `half` that stands on the
    voxel's floor, centred in x and y — with material word material0 + i and a byte pattern in the fields no rule reads."""
    v = np.asarray(voxels, dtype=np.int64).reshape(-1, 3)
    n = len(v)
    s = ((np.arange(n * 64, dtype=np.uint32) * 29 + 5) % 249).astype(np.uint8).view(ref.STATE_DTYPE).copy()
    c = v.astype(f32) + f32(0.5)
    c[:, 2] = v[:, 2].astype(f32) + f32(half)
    s["lo"], s["hi"] = c - f32(half), c + f32(half)
    s["velocity"] = 0
    s["flags"] = flags
    s["material"] = material0 + np.arange(n)
    s["half"], s["reserved"] = half, 0
    return s


def draw_of(states):
    """DRAW_DTYPE[N] as a step would have left them for these states (half kept from the state)."""
    d = np.zeros(states.size, ref.DRAW_DTYPE)
    with np.errstate(all="ignore"):
        d["center"] = (states["lo"] + states["hi"]) * f32(0.5)
    d["half"], d["material"], d["emission"], d["light"] = states["half"], states["material"], states["emission"], states["light"]
    d["reserved"] = 0x5A5A5A5A                                 # (no rule reads or writes it)
    return d


def _case(p, states, **expect):
    return dict(p=p, states=states, expect=dict(dict(deposited=0, voxels=0, occupied=0, outside=0), **expect))


COUNTS = (1, 63, 64, 65, 257, 1025)
COUNT_BOX = ((20, 30, 120), (100, 70, 135))                     # eight chunks: x 0..1, y 0..1, z 1..2


def count_case(n):
    """n records on distinct voxels of the floor's surface; every fifth is DEAD, every seventh of the others sits one voxel down, inside
    the floor."""
    i = np.arange(n)
    v = np.stack([-100 + i % 61, -90 + i // 61, np.zeros(n, np.int64)], axis=1)
    dead, sunk = i % 5 == 4, (i % 5 != 4) & (i % 7 == 6)
    v[sunk, 2] = -1
    s = resting(v)
    s["flags"][dead] |= psr.DEAD
    live = int((~dead & ~sunk).sum())
    return _case(ref.params(*COUNT_BOX), s, deposited=live, voxels=live, occupied=int(sunk.sum()))


def clipped_case():
    """A box clipped by the region's face x = 0: four records on texels x = 0..3, one beyond the window's edge (world x = -129), one
    inside the window but beside the box (texel x = 21)."""
    v = [(-128, -90, 0), (-127, -90, 0), (-126, -90, 0), (-125, -90, 0), (-129, -90, 0), (-107, -90, 0)]
    return _case(ref.params((-10, 30, 120), (20, 50, 140)), resting(v), deposited=4, voxels=4, outside=2)


def seam_case():
    """lr != 0: the window's seam in x lies between texels 39 (world x = 167) and 40 (world x = -88); one record on each side, one
    beyond the window (world x = 168, which would alias texel 40) and one below it in z."""
    v = [(167, 0, 8), (-88, 0, 8), (168, 0, 8), (-88, 1, -121)]
    return _case(ref.params((30, 120, 120), (50, 135, 140), lr=LR_SEAM), resting(v), deposited=2, voxels=2, outside=2)


SHARED_TEXELS = [(-60, -60, 0), (-59, -60, 0), (-60, -59, 0), (-59, -59, 0), (-58, -58, 0)]


def shared_case():
    """300 records into 5 texels with distinct materials.  Texel 0 gets its first record at index 260, in the last wave of the launch;
    texel 1 gets index 0, in the first."""
    i = np.arange(300)
    which = i % 5
    which[(which == 0) & (i < 260)] = 1
    return _case(ref.params((60, 60, 120), (75, 75, 135)), resting(np.asarray(SHARED_TEXELS)[which]), deposited=300, voxels=5)


SHARED_WINNERS = {0: 260, 1: 0, 2: 2, 3: 3, 4: 4}                # texel -> the index whose material it takes


def nothing_case():
    """Candidates that are occupied or outside, and records that are no candidates: nothing deposits."""
    s = resting([(-60, -60, -1), (-60, -60, -5), (100, 100, 0), (-60, -59, 0), (-60, -58, 0), (-60, -57, 0), (-60, -56, 0)])
    s["flags"][3] = psr.STICK                                  # no contact
    s["flags"][4] |= psr.INVALID
    s["velocity"][5] = (0.0, 0.5, 0.0)                         # still moving
    s["lo"][6, 0] = np.nan
    return _case(ref.params((60, 60, 120), (75, 75, 135)), s, occupied=2, outside=1)


def eight_chunks_case(mine):
    """A box that meets the eight chunks round texel (64, 64, 64), with deposits in two of them only — (0, 0, 0) and (1, 1, 1) — on the
    first texels there whose minefield byte is not 0 in `mine` (any world; lr = 0).  Two records share the first texel."""
    lo, hi = (40, 40, 40), (90, 90, 90)
    picks = []
    for a, b in ((40, 63), (64, 90)):
        z, y, x = np.nonzero(mine[a:b + 1, a:b + 1, a:b + 1] != 0)
        assert len(z) >= 3
        picks += [(int(x[k]) + a, int(y[k]) + a, int(z[k]) + a) for k in range(3)]
    picks.append(picks[0])
    v = np.asarray(picks, dtype=np.int64) - R // 2
    return _case(ref.params(lo, hi), resting(v), deposited=7, voxels=6)


def cases():
    out = {"count %d" % n: count_case(n) for n in COUNTS}
    out["count 0"] = _case(ref.params(*COUNT_BOX), resting(np.zeros((0, 3))))
    out["clipped"] = clipped_case()
    out["seam"] = seam_case()
    out["shared"] = shared_case()
    out["nothing"] = nothing_case()
    return out


# ---- the debris chain: emit, carve, STICK ticks, deposit, one more step -------------------------------------------------------------
CHAIN_LR = (0, 0, 0)
CHAIN_BLAST = se.sphere((125, 125, 267), 64, material=0, solid=0)          # radius 4 round voxel (62, 62, 133)
CHAIN_STEP = dict(dt=0.1, accel=(0.0, 0.0, -32.0), damping=1.0, restitution=0.5, friction=1.0, rest_speed=0.0, sweeps=3)
CHAIN_TICKS = 3
CHAIN_CAPACITY = 160
CHAIN_DEPOSIT = ref.params((60, 58, 126), (62, 66, 132), max_speed=0.0, lr=CHAIN_LR)    # three of the block's five columns in x
_CHAIN = {}


def chain_world():
    """world() with a 5^3 block of 125 different material words three voxels above the floor (texels 60..64, 60..64, 131..135)."""
    mats, mine = (a.copy() for a in world())
    mats[131:136, 60:65, 60:65] = 0xC0000000 + np.arange(125, dtype=np.uint32).reshape(5, 5, 5)
    ve.apply_edits(mats, mine, np.argwhere(np.ones((5, 5, 5), bool))[:, ::-1] + (60, 60, 131), mats[131:136, 60:65, 60:65].reshape(-1),
                   np.ones(125, bool))
    return mats, mine


def chain_emitters():
    """One emitter: the whole block falls straight down (no radial speed, no jitter), STICK, and lives through the chain."""
    return eref.batch([eref.emitter(CHAIN_BLAST, (0.0, 0.0, 0.0), seed=3, speed=0.0, spread=0.0, drift=(0.0, 0.0, -10.0), half=0.125, life_min=100.0,
                                   life_span=0.0, density=256, response=psr.STICK, light=1, emission=0xFF112233)])


def chain_reference():
    """The chain in the restatements alone, computed once: a dict with the world before the chain, the ring and cursor after the emit,
    the states after CHAIN_TICKS ticks on the carved world, the states, draw records and counts after the deposit, the world after it
    with its touched chunks, and the states and draw records of one more step on that world."""
    if "c" in _CHAIN:
        return _CHAIN["c"]
    mats, mine = chain_world()
    out = dict(world=(mats.copy(), mine.copy()))
    ring = np.zeros(CHAIN_CAPACITY, dtype=ref.STATE_DTYPE)
    ring["flags"], ring["material"] = psr.DEAD, np.arange(CHAIN_CAPACITY)
    cur = np.zeros(1, eref.CURSOR_DTYPE)
    cur[0]["next"] = 150                                          # the emit wraps
    out["ring0"], out["cursor0"] = ring.copy(), cur.copy()
    N, ring, cur = eref.emit(mats, mine, chain_emitters(), CHAIN_LR, ring, CHAIN_CAPACITY, cur[0])
    out["N"], out["emitted"], out["cursor"] = N, ring.copy(), cur
    se.apply_shapes(mats, mine, se.batch([CHAIN_BLAST]))
    p = psr.Params(**CHAIN_STEP)
    history = psr.run(sr.Occupancy(mats, mine, CHAIN_LR, R), p, ring, CHAIN_TICKS)
    out["stepped"], out["stepped_draw"] = history[-1][0], history[-1][1]
    states, draw, counts, touched = ref.deposit(mats, mine, CHAIN_DEPOSIT, history[-1][0], history[-1][1])
    out["deposited"], out["deposited_draw"], out["counts"], out["touched"] = states, draw, counts, touched
    out["world_after"] = (mats.copy(), mine.copy())
    out["last"], out["last_draw"], _ = psr.step(sr.Occupancy(mats, mine, CHAIN_LR, R), p, states)
    _CHAIN["c"] = out
    return out


# ---- the parameter table: valid and invalid records with the verdict the rules give at R = 256 -------------------------------------
def params_table():
    """(DEPOSIT_DTYPE[N], bool[N] expected verdicts at R = 256, names)."""
    rows = []

    def add(name, ok, lo=(20, 30, 120), hi=(100, 70, 135), **kw):
        rows.append((name, ok, ref.params(lo, hi, **kw)))

    add("box", True)
    add("one texel", True, (5, 5, 5), (5, 5, 5))
    add("whole region", True, (0, 0, 0), (255, 255, 255))
    add("box beyond the region", True, (300, 10, 10), (310, 20, 20))
    add("box across a face", True, (-10, 30, 120), (20, 50, 140))
    add("box at 4R", True, (-4 * R, 0, 0), (4 * R, 0, 0))
    add("box beyond 4R", False, (0, 0, 0), (4 * R + 1, 0, 0))
    add("box below -4R", False, (0, -4 * R - 1, 0), (0, 0, 0))
    add("lo above hi", False, (5, 5, 6), (5, 5, 5))
    add("max_speed 0.25", True, max_speed=0.25)
    add("max_speed huge", True, max_speed=3.0e38)
    add("max_speed negative", False, max_speed=-0.5)
    add("max_speed inf", False, max_speed=np.inf)
    add("max_speed nan", False, max_speed=np.nan)
    add("reserved0", False, reserved0=1)
    add("reserved1", False, reserved1=0x80000000)
    add("window at the bound", True, lr=(2 ** 22 - R, -(2 ** 22 - R), 0))
    add("window beyond", False, lr=(2 ** 22 - R + 1, 0, 0))
    add("window far below", False, lr=(0, 0, -2 ** 31))
    return np.array([p for _, _, p in rows], dtype=ref.DEPOSIT_DTYPE), np.array([ok for _, ok, _ in rows]), [n for n, _, _ in rows]


# (logr, lo, hi): boxes whose clipped texel count the host test prints — 2^24 exactly, and 2^24 + 1 = 97 x 257 x 673
LIMIT_BOXES = [(8, (0, 0, 0), (255, 255, 255)), (10, (3, 5, 7), (3 + 96, 5 + 256, 7 + 672)), (9, (0, 0, 0), (255, 255, 256))]
