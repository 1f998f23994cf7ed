"""Inputs of the entity-sweep tests (tests/test_sweep_entities_contract.py, tests/test_gpu_sweep_entities.py): one small arena
world, stamps, and hand-built and seeded cases — sweeps with the boxes and models they are swept against.  Test infrastructure;
nothing here restates a rule.

The arena (`arena_ids`): solid below world z = 0, seeded pillars up to three voxels high on |x|, |y| < 24, bare floor elsewhere.
The hand-built cases stand on the bare floor at x >= 30, where only the floor is in their way.

A case is a dict: sweeps SWEEP_DTYPE[N], boxes BOX_DTYPE[B] or None, models MODEL_DTYPE[M] or None, and `aim`, the class the case
was built to produce (the census of the contract test counts classes from the restatement, not from this word)."""
import numpy as np

from tests import scenes
from tests import stamp_edits as se
from tests.entity_query_sets import BOX_DTYPE, MODEL_DTYPE, stamp_arrays
from tests.sweep_entities_ref import SWEEP_DTYPE, make_sweeps

f32 = np.float32
PLAYER = np.array([0.6, 0.6, 1.8])
SCALES = [1.0 / 16.0, 1.0, 3.0]
# (extent (x, y, z), seed, share of solid voxels): up to 16^3; the last two are the merged-plane models' (solid)
SPECS = [((16, 16, 16), 1, 0.3), ((9, 5, 12), 2, 0.5), ((3, 11, 4), 3, 1.0), ((8, 8, 8), 4, 0.15), ((8, 8, 8), 5, 1.0), ((16, 16, 16), 6, 1.0)]
MERGED_8, MERGED_16 = 4, 5          # indices into SPECS


def arena_ids(seed=11):
    ids = scenes.floor_ids(0)
    rng = np.random.default_rng(seed)
    for _ in range(160):
        x, y = rng.integers(-24, 24, 2)
        ids[128:128 + int(rng.integers(1, 4)), 128 + y, 128 + x] = 3
    return ids


def stamps_by_id(ids=None):
    ids = list(range(1, len(SPECS) + 1)) if ids is None else list(ids)
    return {int(i): stamp_arrays(*spec) for i, spec in zip(ids, SPECS)}


def boxes_of(lo, hi, seed=0):
    lo = np.asarray(lo, dtype=np.float64).reshape(-1, 3)
    b = np.zeros(lo.shape[0], dtype=BOX_DTYPE)
    b["lo"], b["hi"] = lo.astype(f32), np.asarray(hi, dtype=np.float64).reshape(-1, 3).astype(f32)
    rng = np.random.default_rng(seed)
    b["material"], b["emission"] = rng.integers(1, 1 << 21, b.size), 0xFF000000
    return b


def models_of(stamp, origin, scale, orient=0):
    origin = np.asarray(origin, dtype=np.float64).reshape(-1, 3)
    m = np.zeros(origin.shape[0], dtype=MODEL_DTYPE)
    m["origin"], m["scale"], m["stamp"], m["orient"], m["emission"] = origin.astype(f32), scale, stamp, orient, 0xFF000000
    return m


def case(aim, lo, hi, motion, boxes=None, models=None, skip_box=None, skip_model=None):
    return {"aim": aim, "sweeps": make_sweeps(lo, hi, motion, skip_box, skip_model), "boxes": boxes, "models": models}


# ---- seeded cases ------------------------------------------------------------------------------------------------------------------
def entities(seed, nboxes, nmodels, ids, stamps, scales=SCALES, centre=(0.0, 0.0, 0.0), spread=20.0):
    """Boxes and models standing, hovering or sunk a little in the arena's pillar field (or round `centre`); a third on the quarter
    grid."""
    rng = np.random.default_rng(seed)
    centre = np.asarray(centre, dtype=np.float64)
    lo = centre + np.concatenate([rng.uniform(-spread, spread, (nboxes, 2)), rng.uniform(-0.5, 5.0, (nboxes, 1))], 1)
    size = rng.uniform(0.3, 3.0, (nboxes, 3))
    snap = rng.random(nboxes) < 0.35
    lo[snap], size[snap] = np.round(lo[snap] * 4) / 4, np.maximum(np.round(size[snap] * 4) / 4, 0.25)
    boxes = boxes_of(lo, lo + size, seed)
    usable = np.array(list(ids)[:MERGED_8], dtype=np.uint32)
    origin = centre + np.concatenate([rng.uniform(-spread, spread, (nmodels, 2)), rng.uniform(-0.5, 4.0, (nmodels, 1))], 1)
    snap = rng.random(nmodels) < 0.4
    origin[snap] = np.round(origin[snap])
    models = models_of(usable[rng.integers(0, usable.size, nmodels)], origin, np.array(scales, dtype=f32)[rng.integers(0, len(scales), nmodels)],
                       rng.integers(0, 48, nmodels))
    return (boxes if nboxes else None), (models if nmodels else None)


def bounds(boxes, models, stamps):
    """float64[B + M, 2, 3]: the bounding boxes of the entities (a model's in real arithmetic)."""
    out = []
    for b in ([] if boxes is None else boxes):
        out.append([b["lo"].astype(np.float64), b["hi"].astype(np.float64)])
    for m in ([] if models is None else models):
        ext = np.array(se.placed_extent(se.extent_of(stamps[int(m["stamp"])][1]), int(m["orient"])), dtype=np.float64)
        out.append([m["origin"].astype(np.float64), m["origin"].astype(np.float64) + ext * float(m["scale"])])
    return np.array(out, dtype=np.float64).reshape(-1, 2, 3)


def sweeps_at(seed, n, boxes, models, stamps, centre=(0.0, 0.0, 0.0), spread=20.0):
    """n sweeps aimed at the entities: most start beside one and move at a point of it, a fifth come along one axis on the quarter
    grid (faces that touch, corners met exactly), the rest fall to the floor or move anywhere in the arena."""
    rng = np.random.default_rng(seed)
    centre = np.asarray(centre, dtype=np.float64)
    bb = bounds(boxes, models, stamps)
    lo, size, m = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        size[i] = PLAYER if rng.random() < 0.5 else rng.uniform(0.3, 2.5, 3)
        mode = rng.random()
        tl, th = bb[rng.integers(0, len(bb))] if len(bb) else (centre + rng.uniform(-spread, spread, 3), centre + rng.uniform(-spread, spread, 3))
        aim = tl + rng.random(3) * (th - tl)
        if mode < 0.5:
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            dist = rng.uniform(0.5, 5.0) + 0.5 * np.linalg.norm(th - tl)
            lo[i] = aim - d * dist - 0.5 * size[i]
            m[i] = d * dist * rng.uniform(0.5, 1.6)
        elif mode < 0.7:
            size[i] = np.maximum(np.round(size[i] * 4) / 4, 0.25)
            k, sign = rng.integers(0, 3), rng.choice([-1.0, 1.0])
            lo[i] = np.round((aim - 0.5 * size[i]) * 4) / 4
            gap = np.round(rng.uniform(0.0, 3.0) * 4) / 4
            lo[i, k] = (np.round(tl[k] * 4) / 4 - size[i, k] - gap) if sign > 0 else (np.round(th[k] * 4) / 4 + gap)
            m[i, k] = sign * np.round(rng.uniform(0.25, 5.0) * 4) / 4
            if rng.random() < 0.5:                       # a diagonal on the quarter grid
                j = (k + 1 + rng.integers(0, 2)) % 3
                m[i, j] = rng.choice([-1.0, 1.0]) * abs(m[i, k])
        elif mode < 0.85:
            lo[i] = np.array([aim[0], aim[1], centre[2] + rng.uniform(0.0, 4.0)]) - np.array([0.3, 0.3, 0.0])
            m[i] = [rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), -rng.uniform(0.5, 6.0)]
        else:
            lo[i] = centre + np.concatenate([rng.uniform(-spread - 2.0, spread + 2.0, 2), rng.uniform(0.0, 6.0, 1)])
            m[i] = rng.uniform(-6.0, 6.0, 3) * (rng.random(3) < 0.8)
    return make_sweeps(lo, lo + size, np.clip(m, -60.0, 60.0))


def seeded(seed, n, nboxes, nmodels, ids, stamps, scales=SCALES, centre=(0.0, 0.0, 0.0), spread=20.0):
    boxes, models = entities(seed, nboxes, nmodels, ids, stamps, scales, centre, spread)
    return {"aim": "seeded", "sweeps": sweeps_at(seed + 1000, n, boxes, models, stamps, centre, spread), "boxes": boxes, "models": models}


# ---- hand-built cases, on the bare floor at x >= 30 ----------------------------------------------------------------------------------
def hand_built(ids, stamps, seed=3):
    """The classes of the census that chance does not reliably give, a dozen sweeps each."""
    rng = np.random.default_rng(seed)
    ids = list(ids)
    out = []
    n = 12
    x0 = 32.0 + 3.0 * np.arange(n)
    frac = rng.uniform(0.0, 1.0, (n, 3))
    # exact tie: a box lying in the floor with its top at z = 0, the world's own plane: both block at (0 - lo_z) / m_z
    lo = np.stack([x0 + frac[:, 0], 5.0 + frac[:, 1], 0.25 + frac[:, 2]], 1)
    obst = boxes_of(np.stack([x0 - 1.0, np.full(n, 4.0), np.full(n, -0.75)], 1), np.stack([x0 + 3.0, np.full(n, 8.0), np.zeros(n)], 1))
    out.append(case("tie", lo, lo + PLAYER, np.stack([frac[:, 1] - 0.5, frac[:, 0] - 0.5, -2.0 - frac[:, 2]], 1), obst))
    # world earlier: the same sweeps over boxes buried a little deeper
    deep = boxes_of(np.stack([x0 - 1.0, np.full(n, 4.0), np.full(n, -1.5)], 1), np.stack([x0 + 3.0, np.full(n, 8.0), np.full(n, -0.125)], 1))
    out.append(case("world earlier", lo, lo + PLAYER, np.stack([frac[:, 1] - 0.5, frac[:, 0] - 0.5, -2.0 - frac[:, 2]], 1), deep))
    # touching start: the leading face lies on the obstacle's near face, bit for bit, and moves into it: blocked at t = 0
    wall_lo = np.stack([x0 + 1.0 + frac[:, 0], np.full(n, 10.0), np.full(n, 0.0)], 1)
    wall = boxes_of(wall_lo, wall_lo + np.array([0.5, 2.0, 3.0]))
    hi = np.stack([wall["lo"][:, 0].astype(np.float64), 10.5 + frac[:, 1], 0.5 + PLAYER[2] + frac[:, 2]], 1)
    out.append(case("touching", hi - PLAYER.astype(f32).astype(np.float64), hi, np.stack([0.5 + frac[:, 2], frac[:, 1] - 0.5, np.zeros(n)], 1), wall))
    # ... and moves along it or away from it: a face that is only touched does not catch
    out.append(case("none", hi - PLAYER.astype(f32).astype(np.float64), hi, np.stack([-frac[:, 2], frac[:, 1] + 0.25, np.zeros(n)], 1), wall))
    # exact corner: quarter-grid boxes on a diagonal that meets the obstacle's edge at the same t on two axes
    q = np.round(frac * 4) / 4
    c_lo = np.stack([x0, np.full(n, 16.0), 0.5 + q[:, 2]], 1)
    corner = boxes_of(c_lo, c_lo + 1.0)
    gap = 0.25 + q[:, 0]
    s_hi = np.stack([c_lo[:, 0] - gap, c_lo[:, 1] - gap, c_lo[:, 2] + 0.75], 1)
    mv = gap + 0.5
    out.append(case("corner", s_hi - 0.5, s_hi, np.stack([mv, mv, np.zeros(n)], 1), corner))
    out.append(case("corner", np.stack([c_lo[:, 0] + 1.0 + gap, c_lo[:, 1] - gap - 0.5, c_lo[:, 2]], 1),
                    np.stack([c_lo[:, 0] + 1.5 + gap, c_lo[:, 1] - gap, c_lo[:, 2] + 0.5], 1), np.stack([-mv, mv, np.zeros(n)], 1), corner))
    # embedded in an entity: in a box; in a model cell
    out.append(case("embedded", c_lo + 0.5 * frac, c_lo + 0.5 * frac + 0.75, frac - 0.5, corner))
    solid = models_of(ids[2], np.stack([x0, np.full(n, 22.0), frac[:, 2]], 1), 1.0 / 16.0, np.arange(n) * 4)
    m_lo = solid["origin"].astype(np.float64) + 0.05
    out.append(case("embedded", m_lo, m_lo + 0.3, frac - 0.5, None, solid))
    # mobs: every sweep is the box of entity i itself and ignores it; half walk into their neighbour
    mob_lo = np.stack([32.0 + 1.0 * np.arange(n), np.full(n, 28.0), np.zeros(n)], 1)
    mobs = boxes_of(mob_lo, mob_lo + np.array([0.75, 0.75, 1.5]))
    out.append(case("self", mobs["lo"], mobs["hi"], np.stack([np.where(np.arange(n) % 2, 0.75, 0.125), frac[:, 1] - 0.5, np.zeros(n)], 1), mobs, None, np.arange(n)))
    doors = models_of(ids[2], np.stack([x0, np.full(n, 34.0), np.zeros(n)], 1), 1.0, 0)
    ext = np.array(se.extent_of(stamps[ids[2]][1]), dtype=np.float64)
    d_lo = doors["origin"].astype(np.float64)
    out.append(case("self", d_lo, d_lo + np.minimum(ext, 8.0), frac - 0.5, None, doors, None, np.arange(n)))
    # merged planes: at scale 2^-8 the 8^3 model's nine planes all round to its origin near 2^21 and it has no cell at all; the 16^3
    # model near 2^18 keeps a few cells 1/32 wide between runs of merged planes
    for spec, at, aim in ((MERGED_8, 2097152.0, "merged"), (MERGED_16, 262144.0, "merged")):
        model = models_of(ids[spec], [[at, at, -at]], 1.0 / 256.0, 5)
        s_lo = np.stack([at - 1.0 - frac[:, 0], at - 0.25 + 0.0 * frac[:, 1], -at - 0.25 + 0.0 * frac[:, 2]], 1)
        out.append(case(aim, s_lo, s_lo + 0.5, np.stack([2.0 + frac[:, 1], 0.125 * (frac[:, 0] - 0.5), 0.125 * (frac[:, 2] - 0.5)], 1), None, model))
    # nothing at all: high above everything
    far_lo = np.stack([x0, np.full(n, 40.0), 20.0 + frac[:, 2]], 1)
    out.append(case("none", far_lo, far_lo + PLAYER, frac - 0.5, corner, solid))
    return out


def invalid(sweeps, seed=9):
    """A copy of `sweeps` with one record in five outside the validated domain, and which."""
    rng = np.random.default_rng(seed)
    bad = sweeps.copy()
    which = np.sort(rng.choice(bad.size, max(8, bad.size // 5), replace=False))
    for j, i in enumerate(which):
        k = int(rng.integers(0, 3))
        what = j % 6
        if what == 0: bad["lo"][i, k] = np.nan
        elif what == 1: bad["motion"][i, k] = np.inf
        elif what == 2: bad["hi"][i, k] = bad["lo"][i, k]
        elif what == 3: bad["hi"][i, k] = bad["lo"][i, k] + f32(9.0)
        elif what == 4: bad["motion"][i, k] = -65.0
        else: bad["lo"][i, k], bad["hi"][i, k] = 2.0 ** 23, 2.0 ** 23 + 1
    return bad, which
