"""numpy restatement of rt_deposit_particles (include/rt_abi.h "Particle deposits") for the deposit tests.  Test infrastructure,
written from the rules and not from the kernels.

The box's validity and clipping are tests/shape_edits.py's (`valid`, `bounding_box`) and the world change goes through
tests/voxel_edits.py's `apply_edits`: no shape rule and no rebuild rule is restated here.  Arrays are [z, y, x] in texel order; a
particle is one row of particle_step_ref.STATE_DTYPE, a draw record one of DRAW_DTYPE.

The rules.  Record i is a CANDIDATE iff DEAD and INVALID are clear, a CONTACT bit is set, |velocity_k| <= max_speed on every axis and
every lo_k, hi_k is finite with |.| <= 2^22 (a comparison with a NaN is false).  Its TARGET is the world voxel v_k =
floor((lo_k + hi_k) * 0.5f), fp32 with one rounding per operation; the texel is x_k = (v_k + R/2) mod R and exists only if lr_k - R/2
<= v_k < lr_k + R/2.  A candidate whose target lies outside the window or outside the clipped box counts as `outside`; one whose
texel is occupied (minefield byte 0) before the call as `occupied`; every other one DEPOSITS: DEAD is ORed into its flags, its draw
record's half becomes +0.0, its texel becomes occupied with the material of the depositing record of the LOWEST index, and the
chunks that hold such texels are rebuilt as rt_edit_voxels rebuilds them.  The four counts are added to, wrapping."""
import numpy as np

from tests import particle_step_ref
from tests import shape_edits as se
from tests import voxel_edits as ve

f32 = np.float32
STATE_DTYPE = particle_step_ref.STATE_DTYPE
DRAW_DTYPE = particle_step_ref.DRAW_DTYPE
DEAD, INVALID, CONTACT = particle_step_ref.DEAD, particle_step_ref.INVALID, particle_step_ref.CONTACT

# numpy views of RtParticleDeposit and RtDepositCount, declared here a second time on purpose (the binding's own are
# raytrace_amd.abi.DEPOSIT_DTYPE and DEPOSIT_COUNT_DTYPE)
DEPOSIT_DTYPE = np.dtype([("lo", "<i4", 3), ("max_speed", "<f4"), ("hi", "<i4", 3), ("reserved0", "<u4"), ("lr", "<i4", 3), ("reserved1", "<u4")])
COUNT_DTYPE = np.dtype([("deposited", "<u4"), ("voxels", "<u4"), ("occupied", "<u4"), ("outside", "<u4")])
assert DEPOSIT_DTYPE.itemsize == 48 and COUNT_DTYPE.itemsize == 16

MAX_PARTICLES, MAX_TEXELS, MAX_COORD = 1 << 20, 1 << 24, f32(4194304.0)


def params(lo, hi, max_speed=0.0, lr=(0, 0, 0), reserved0=0, reserved1=0):
    p = np.zeros((), DEPOSIT_DTYPE)
    p["lo"], p["hi"], p["lr"], p["max_speed"], p["reserved0"], p["reserved1"] = lo, hi, lr, max_speed, reserved0, reserved1
    return p


def shape_of(p):
    """The deposit box as a shape_edits box row."""
    return se.box(tuple(int(v) for v in p["lo"]), tuple(int(v) for v in p["hi"]))


def window_valid(lr, R):
    return all(abs(int(v)) <= 2 ** 22 - R for v in lr)


def valid(p, R):
    """The host's verdict on the parameters (the 2^24 limit apart: `clipped_box` and MAX_TEXELS)."""
    if not (p["max_speed"] >= 0 and np.isfinite(p["max_speed"])) or p["reserved0"] != 0 or p["reserved1"] != 0:
        return False
    return bool(se.valid(shape_of(p), R) and window_valid(p["lr"], R))


def clipped_box(p, R):
    """(lo, hi) int64[3] in (x, y, z), inclusive, or None when the box misses [0, R)^3."""
    return se.bounding_box(shape_of(p), R)


def box_texels(bb):
    return 0 if bb is None else int(np.prod(bb[1] - bb[0] + 1))


def box_chunks(bb):
    """The chunk ids' coordinates (cx, cy, cz) of the box, in ascending id order (z-major)."""
    if bb is None:
        return []
    return [(cx, cy, cz) for cz in range(int(bb[0][2]) >> 6, (int(bb[1][2]) >> 6) + 1) for cy in range(int(bb[0][1]) >> 6, (int(bb[1][1]) >> 6) + 1)
            for cx in range(int(bb[0][0]) >> 6, (int(bb[1][0]) >> 6) + 1)]


def candidate(rec, max_speed):
    flags = int(rec["flags"])
    if flags & (DEAD | INVALID) or not flags & CONTACT:
        return False
    with np.errstate(all="ignore"):
        for k in range(3):
            if not np.abs(f32(rec["velocity"][k])) <= f32(max_speed):
                return False
            if not (np.abs(f32(rec["lo"][k])) <= MAX_COORD and np.abs(f32(rec["hi"][k])) <= MAX_COORD):
                return False
    return True


def target(rec):
    """The world voxel (x, y, z) of a candidate's centre."""
    return tuple(int(np.floor(f32(f32(f32(rec["lo"][k]) + f32(rec["hi"][k])) * f32(0.5)))) for k in range(3))


def texel_of(v, lr, R):
    """The texel of world voxel v under window centre lr, or None outside the window."""
    h = R // 2
    if not all(int(lr[k]) - h <= v[k] < int(lr[k]) + h for k in range(3)):
        return None
    return tuple((v[k] + h) % R for k in range(3))


def outcomes(mine, p, states):
    """Per record: None (no candidate), "outside", "occupied" or the target texel (x, y, z) of a depositing record."""
    R = mine.shape[0]
    bb = clipped_box(p, R)
    out = []
    for rec in states:
        if not candidate(rec, p["max_speed"]):
            out.append(None)
            continue
        t = texel_of(target(rec), p["lr"], R)
        if t is None or bb is None or any(t[k] < bb[0][k] or t[k] > bb[1][k] for k in range(3)):
            out.append("outside")
        elif mine[t[2], t[1], t[0]] == 0:
            out.append("occupied")
        else:
            out.append(t)
    return out


def deposit(mats, mine, p, states, draw=None, counts=None):
    """One call on (mats, mine), changed IN PLACE -> (states, draw, counts, touched): new arrays, `draw` None when none was given,
    `counts` a COUNT_DTYPE record added to (zeros for None), `touched` the sorted (cx, cy, cz) of the chunks that were rebuilt.  A call
    with no record or an empty clipped box changes nothing."""
    R = mine.shape[0]
    states = np.array(states, dtype=STATE_DTYPE).reshape(-1)
    draw = None if draw is None else np.array(draw, dtype=DRAW_DTYPE).reshape(-1)
    cnt = np.zeros(1, COUNT_DTYPE)[0] if counts is None else np.array(counts, dtype=COUNT_DTYPE).reshape(1)[0].copy()
    assert valid(p, R) and states.size <= MAX_PARTICLES and box_texels(clipped_box(p, R)) <= MAX_TEXELS
    if states.size == 0 or clipped_box(p, R) is None:
        return states, draw, cnt, []
    what = outcomes(mine, p, states)
    winners = {}
    add = dict(deposited=0, voxels=0, occupied=0, outside=0)
    for i, w in enumerate(what):
        if w is None:
            continue
        if isinstance(w, str):
            add[w] += 1
            continue
        add["deposited"] += 1
        states[i]["flags"] = np.uint32(int(states[i]["flags"]) | DEAD)
        if draw is not None:
            draw[i]["half"] = f32(0.0)
        winners.setdefault(w, i)                               # ascending i: the first is the lowest index
    add["voxels"] = len(winners)
    for k, v in add.items():
        cnt[k] = (int(cnt[k]) + v) & 0xFFFFFFFF
    xyz = np.array(sorted(winners), dtype=np.int64).reshape(-1, 3)
    words = np.array([states[winners[tuple(t)]]["material"] for t in xyz.tolist()], dtype=np.uint32)
    touched = ve.apply_edits(mats, mine, xyz, words, np.ones(len(xyz), bool))
    return states, draw, cnt, sorted(touched)
