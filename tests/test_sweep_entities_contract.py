"""The entity-sweep rules on their restatement alone (tests/sweep_entities_ref.py; no GPU): the obstacle rule against the world's
event order on voxel sets, a grid-aligned model against the same voxels stamped into the world, the horizon loop against
tests/sweep_ref.py, and the census of the input sets the GPU test uses (tests/test_gpu_sweep_entities.py imports `cases` and
`census` from here, so that what is asserted about them here is what runs there)."""
import numpy as np
import pytest

from raytrace_amd import world
from tests import sweep_entities_ref as ref
from tests import sweep_entities_sets as sets
from tests import sweep_ref as sr

f32 = np.float32
CLASSES = ("box", "model", "world earlier", "tie", "touching", "corner", "embedded", "self", "merged", "invalid", "none")


class VoxelSet:
    """An occupancy that is a set of world voxels (what sweep_ref.sweep needs: first_occupied); the material is a function of v."""

    def __init__(self, voxels):
        self.v = set(tuple(int(c) for c in v) for v in voxels)

    def first_occupied(self, cx, cy, cz):
        for z in range(cz[0], cz[1] + 1):
            for y in range(cy[0], cy[1] + 1):
                for x in range(cx[0], cx[1] + 1):
                    if (x, y, z) in self.v:
                        return (x, y, z), 7
        return None


def random_sweep(rng):
    """Random, quarter-grid and exact-diagonal sweeps round the origin."""
    mode = rng.integers(0, 3)
    if mode == 0:
        lo, size, m = rng.uniform(-4, 4, 3), rng.uniform(0.1, 2.5, 3), rng.uniform(-6, 6, 3)
    elif mode == 1:
        lo, size, m = rng.integers(-16, 16, 3) / 4, rng.integers(1, 8, 3) / 4, rng.integers(-16, 17, 3) / 4
    else:
        lo, size = rng.integers(-8, 8, 3) / 2, rng.integers(1, 4, 3) / 2
        m = rng.choice([-1, 0, 1], 3) * (rng.integers(1, 6) / 2)
    lo = lo.astype(f32)
    return lo, (lo + size.astype(f32)).astype(f32), np.asarray(m, dtype=f32)


def test_the_obstacle_rule_is_the_worlds_event_order_on_voxel_sets():
    """Every occupied voxel v as the box [v, v + 1]; the winner the smallest (t, axis), then ascending (z, y, x): kind, t, axis and
    voxel are sweep_ref's, on 4000 sweeps over random voxel sets."""
    rng = np.random.default_rng(5)
    seen = {}
    for _ in range(4000):
        vox = rng.integers(-3, 4, size=(int(rng.integers(1, 40)), 3))
        vox = np.array(sorted(set(map(tuple, vox)), key=lambda v: (v[2], v[1], v[0])))
        lo, hi, m = random_sweep(rng)
        w = sr.sweep(VoxelSet(vox), lo, hi, m)
        emb, blk, t, a = ref.obstacle(vox.astype(f32), (vox + 1).astype(f32), lo, hi, m)
        if emb.any():
            got = (sr.EMBEDDED, f32(0.0), 3, tuple(vox[int(np.argmax(emb))]))
        elif blk.any():
            j = min(np.nonzero(blk)[0], key=lambda j: (t[j], a[j], j))
            got = (sr.BLOCKED, t[j], int(a[j]), tuple(vox[j]))
        else:
            got = (sr.FREE, f32(1.0), 3, sr.NO_TEXEL)
        assert got == (w["kind"], w["t"], w["axis"], tuple(w["texel"])), (lo, hi, m, got, w)
        seen[w["kind"]] = seen.get(w["kind"], 0) + 1
    assert min(seen.get(k, 0) for k in (sr.FREE, sr.BLOCKED, sr.EMBEDDED)) > 300, seen


def test_a_grid_aligned_model_is_the_same_voxels_in_the_world():
    """A model with scale 1 and an integer origin in an empty world gives the t, axis and returned box that the same voxels give as
    world voxels: the model's planes are the integer planes, the horizon's clamps the world's own."""
    rng = np.random.default_rng(8)
    stamps = sets.stamps_by_id()
    empty = VoxelSet([])
    kinds = {}
    for it in range(600):
        sid = int(rng.integers(1, 5))
        model = sets.models_of(sid, [rng.integers(-6, 3, 3)], 1.0, int(rng.integers(0, 48)))
        (planes, state, vox, mats), = ref.place(model, stamps)
        z, y, x = np.nonzero(state == 2)
        origin = model["origin"][0].astype(np.int64)
        voxels = np.stack([x, y, z], 1) + origin
        lo, hi, m = random_sweep(rng)
        centre = origin + np.array(state.shape[::-1]) // 2
        lo, hi = (lo + centre.astype(f32)).astype(f32), (hi + centre.astype(f32)).astype(f32)
        s = ref.make_sweeps([lo], [hi], [m])
        w = sr.sweep(VoxelSet(voxels), lo, hi, m)
        _, e = ref.sweep_entities(empty, s, None, model, stamps)
        e = e[0]
        kinds[w["kind"]] = kinds.get(w["kind"], 0) + 1
        if w["kind"] == sr.FREE:
            assert e["entity"] == ref.NONE and e["kind"] == ref.FREE
        else:
            assert e["entity"] == ref.MODEL and e["kind"] == w["kind"] and e["t"] == w["t"] and e["axis"] == w["axis"], (lo, hi, m, w, e)
            assert tuple(e["cell"] + origin) == tuple(w["texel"])          # (VoxelSet reports the world voxel as the texel)
        assert e["lo"].tobytes() == np.array(w["lo"], dtype=f32).tobytes() and e["hi"].tobytes() == np.array(w["hi"], dtype=f32).tobytes(), (w, e)
    assert min(kinds.get(k, 0) for k in (sr.FREE, sr.BLOCKED, sr.EMBEDDED)) > 40, kinds


@pytest.fixture(scope="module")
def arena(native_built):
    mats, mine = world.region_from_ids(sets.arena_ids())
    return sr.Occupancy(mats, mine, (0, 0, 0), 256)


def cases(ids=None):
    """The cases of the census and of the GPU test, for stamps created under `ids` (default 1, 2, ...): (stamps, list of cases)."""
    stamps = sets.stamps_by_id(ids)
    ids = sorted(stamps) if ids is None else list(ids)
    out = sets.hand_built(ids, stamps)
    out.append(sets.seeded(21, 257, 130, 1, ids, stamps))
    out.append(sets.seeded(22, 65, 65, 65, ids, stamps))
    out.append(sets.seeded(23, 64, 64, 0, ids, stamps))
    out.append(sets.seeded(24, 63, 63, 3, ids, stamps))
    out.append(sets.seeded(25, 1, 1, 1, ids, stamps))
    out.append(sets.seeded(26, 40, 0, 0, ids, stamps))
    bad = dict(out[-4])
    bad["sweeps"], bad["which"] = sets.invalid(out[-4]["sweeps"])
    bad["aim"] = "invalid"
    out.append(bad)
    return stamps, out


def census(occ, c, stamps):
    """The outcome classes of one case by the restatement alone: (world_hits, entity_hits, {class: count})."""
    W, E, cls = ref.sweep_entities(occ, c["sweeps"], c["boxes"], c["models"], stamps, classes=True)
    count = {k: 0 for k in CLASSES}
    placed = ref.place(c["models"], stamps) if c["models"] is not None else []
    for i, s in enumerate(c["sweeps"]):
        if cls[i] in count:
            count[cls[i]] += 1
        e = E[i]
        lo, hi, m = s["lo"], s["hi"], s["motion"]
        if e["kind"] == ref.BLOCKED and e["t"] == 0:
            count["touching"] += 1
        if e["kind"] == ref.BLOCKED and e["entity"] == ref.BOX:
            b = c["boxes"][e["index"]]
            te = [ref.axis_terms(b["lo"][k], b["hi"][k], lo[k], hi[k], m[k])[1] for k in range(3)]
            te = [float(t) for t in te if t is not None]
            count["corner"] += len(te) > len(set(te))
        if s["reserved0"] or s["reserved1"]:
            plain = s.copy()
            plain["reserved0"] = plain["reserved1"] = 0
            _, e0 = ref.sweep_entities(occ, np.array([plain]), c["boxes"], c["models"], stamps)
            mine = (ref.BOX, s["reserved0"] - 1) if s["reserved0"] else (ref.MODEL, s["reserved1"] - 1)
            count["self"] += e0[0]["kind"] == ref.EMBEDDED and (e0[0]["entity"], e0[0]["index"]) == mine and e.tobytes() != e0[0].tobytes()
        for planes, *_ in placed:
            merged = any((p[:-1] == p[1:]).any() for p in planes)
            with np.errstate(all="ignore"):
                reach = all(min(lo[k], lo[k] + m[k]) <= planes[k][-1] and max(hi[k], hi[k] + m[k]) >= planes[k][0] for k in range(3))
            if merged and reach and cls[i] != "invalid":
                count["merged"] += 1
                break
    return W, E, count


def test_horizon_loop_at_horizon_1_is_sweep_ref(arena):
    stamps, cs = cases()
    kinds = {}
    for c in cs:
        for s in c["sweeps"] if c["aim"] == "invalid" else c["sweeps"][:40]:   # (the case with records outside the domain whole)
            a, b = ref.horizon_sweep(arena, s["lo"], s["hi"], s["motion"]), sr.sweep(arena, s["lo"], s["hi"], s["motion"])
            assert sr.pack([a]).tobytes() == sr.pack([b]).tobytes(), (s, a, b)
            kinds[b["kind"]] = kinds.get(b["kind"], 0) + 1
    assert min(kinds.get(k, 0) for k in (sr.FREE, sr.BLOCKED, sr.EMBEDDED, sr.INVALID)) >= 8, kinds


def test_census_of_the_sets(arena):
    """Each outcome class holds at least 8 sweeps, by the restatement alone."""
    stamps, cs = cases()
    total = {k: 0 for k in CLASSES}
    for c in cs:
        _, E, count = census(arena, c, stamps)
        for k in CLASSES:
            total[k] += count[k]
        assert (E["reserved0"] == 0).all() and (E["reserved1"] == 0).all() and (E["reserved2"] == 0).all()
    assert min(total.values()) >= 8, total
