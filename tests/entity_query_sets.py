"""Inputs of the entity-query tests (tests/test_entity_query_contract.py, tests/test_gpu_entity_queries.py): stamps, and boxes and models
placed along the rays that will be asked about, so that a known share of any ray set — coherent or not — meets an entity.  Test
infrastructure; nothing here restates a rule."""
import numpy as np

from tests import stamp_edits as se

f32 = np.float32
BOX_DTYPE = np.dtype([("lo", "<f4", 3), ("material", "<u4"), ("hi", "<f4", 3), ("emission", "<u4")])
MODEL_DTYPE = np.dtype([("origin", "<f4", 3), ("scale", "<f4"), ("stamp", "<u4"), ("orient", "u1"), ("reserved0", "u1", 3),
                        ("emission", "<u4"), ("reserved", "<u4")])
HIT_DTYPE = np.dtype([("position", "<f4", 3), ("distance", "<f4"), ("texel", "<i4", 3), ("material", "<u4"), ("normal", "<u4"),
                      ("kind", "<u4"), ("iterations", "<u4"), ("border_fetches", "<u4")])
SCALES = [1.0 / 16.0, 0.37, 1.0, 2.5]
# (extent (x, y, z), seed, share of solid voxels): tests/test_gpu_draw_stamps.py's FOUR, the longest stamp a walk can meet and the smallest
SPECS = [((9, 9, 12), 1, 0.3), ((12, 5, 7), 2, 1.0), ((3, 11, 4), 3, 0.15), ((6, 6, 6), 4, 0.6), ((1, 1, 256), 5, 0.05), ((1, 1, 1), 6, 1.0)]


def stamp_arrays(ext, seed, fill):
    """(materials u32[ez, ey, ex], state u8[ez, ey, ex]): fill = 1 is solid, otherwise that share solid and the rest air and absent."""
    rng = np.random.default_rng(seed)
    ex, ey, ez = ext
    rest = (1.0 - fill) / 2.0
    state = rng.choice(np.array([se.ABSENT, se.AIR, se.SOLID], dtype=np.uint8), size=(ez, ey, ex), p=[rest, rest, fill])
    mats = rng.integers(1, 1 << 21, size=(ez, ey, ex)).astype(np.uint32)
    mats[state == se.ABSENT] = 0
    return mats, state


def stamps_by_id(ids=None, specs=SPECS):
    """{id: (materials, state)}; ids default to 1, 2, ..."""
    ids = list(range(1, len(specs) + 1)) if ids is None else list(ids)
    return {int(i): stamp_arrays(*spec) for i, spec in zip(ids, specs)}


def sky(n):
    """World hits of n rays that all left the region."""
    return np.zeros(n, dtype=HIT_DTYPE)


def _anchors(o, d, n, rng, near, far):
    """n points on randomly chosen finite rays with a direction, at log-uniform distances."""
    o, d = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        norm = np.linalg.norm(d, axis=1)
        usable = np.nonzero(np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (norm > 1e-6) & (norm < 1e6) & (np.abs(o).max(axis=1) < 1e5))[0]
    pick = usable[rng.integers(0, usable.size, n)]
    t = np.exp(rng.uniform(np.log(near), np.log(far), n))
    return o[pick] + d[pick] / norm[pick][:, None] * t[:, None]


def boxes_along(o, d, n, seed, near=4.0, far=300.0):
    """n valid entity-sized boxes round points of the rays (o, d)."""
    rng = np.random.default_rng(seed)
    c = _anchors(o, d, n, rng, near, far)
    half = rng.uniform(0.15, 1.2, (n, 3))
    b = np.zeros(n, dtype=BOX_DTYPE)
    b["lo"], b["hi"] = (c - half).astype(f32), (c + half).astype(f32)
    b["material"] = rng.integers(1, 1 << 21, n)
    b["emission"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    assert (b["lo"] < b["hi"]).all()
    return b


def models_along(o, d, n, seed, stamps, near=4.0, far=300.0, scales=SCALES):
    """n valid models of random stamps, scales and orientations whose bounding boxes hold points of the rays (o, d)."""
    rng = np.random.default_rng(seed)
    c = _anchors(o, d, n, rng, near, far)
    ids = np.array(sorted(stamps), dtype=np.uint32)
    m = np.zeros(n, dtype=MODEL_DTYPE)
    m["stamp"] = ids[rng.integers(0, ids.size, n)]
    m["orient"] = rng.integers(0, 48, n)
    m["scale"] = np.array(scales, dtype=f32)[rng.integers(0, len(scales), n)]
    m["emission"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    for i in range(n):
        ext = np.array(se.placed_extent(se.extent_of(stamps[int(m["stamp"][i])][1]), int(m["orient"][i])), dtype=np.float64)
        m["origin"][i] = (c[i] - rng.uniform(0.2, 0.8, 3) * ext * float(m["scale"][i])).astype(f32)
    return m
