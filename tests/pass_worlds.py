"""The worlds, camera poses and scattered records of tests/test_pass_inputs.py (CPU: the inputs are what they claim) and
tests/test_gpu_pass_worlds.py (GPU: the frame passes, the entity queries and the probes on them).  Test infrastructure.

Worlds: the arbitrary and the pyramid world of tests/adversarial_worlds.py at regions 256 and 512, and the "limit" window of
tests/test_gpu_ray_queries.py — the procedural terrain scrolled to lr = (2048, 0, 0), where a ray that has to cross an x plane at
x >= 2048 stalls (the shader's 0.0001 is below half an ulp there) and ends at RT_TRACE_LIMIT.  Two poses per world, the second one
scrolled (in the limit window both are).

The scattered lights and the occluders put between a light and a surface are the recipes tests/test_gpu_light_shadows.py always
used; they live here so that a test without a GPU can import them."""
import numpy as np

from raytrace_amd import render, world
from tests import adversarial_worlds as aw
from tests import entity_shadow_ref as shadow_ref
from tests import point_light_ref as pl
from tests import stamp_edits as se
from tests.draw_stamps_ref import batch as model_batch, model as one_model

f32 = np.float32
STAMP_EXTENT = (3, 4, 5)                 # entity_shadow_ref.small_stamp's
LIMIT_LR = (2048, 0, 0)
LIMIT_POSES = [
    dict(origin=(2018.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.2, sun=0.3, lr=LIMIT_LR),
    dict(origin=(2070.0, -120.0, 110.0), heading=np.pi / 2 + 0.4, pitch=-0.35, sun=-0.6, lr=LIMIT_LR),
]
# a third pose of the arbitrary world at 256, found by a seeded search over the oracle's frames: it looks into mixed cubes, where a ray
# often lands deep inside solid voxels — a quarter of its surface points P' lie on a 0 texel
ON_ZERO_POSE = dict(origin=(51.5, -59.5, -12.5), heading=0.69, pitch=-0.18, sun=0.4, lr=(0, 0, 0))
PLAIN, SCROLLED, ON_ZERO = 0, 1, 2       # the poses of a world; ON_ZERO exists for ("arbitrary", 256) only
WORLDS = [("arbitrary", 256), ("arbitrary", 512), ("pyramid", 256), ("pyramid", 512), ("limit", 256)]
SHAPES = [(52, 36), (100, 60)]           # partial 8x8 tiles on both axes

_HELD = {}


def world_of(name, R):
    """(materials, minefield) [z, y, x], built once; one region above 256 is held at a time."""
    if (name, R) not in _HELD:
        for k in [k for k in _HELD if k[1] > 256]:
            del _HELD[k]
        if name == "arbitrary":
            w = aw.arbitrary_world(R)
        elif name == "pyramid":
            w = aw.pyramid_world(R)
        else:
            assert (name, R) == ("limit", 256)
            w = world.toroidal_region(LIMIT_LR)
        _HELD[(name, R)] = (w[0], w[1])
    return _HELD[(name, R)]


def poses(name, R=256):
    """[the plain pose, the scrolled pose, (the on-zero pose)] of a world."""
    if name == "limit":
        return LIMIT_POSES
    if name == "pyramid":
        return [aw.PYRAMID_POSES[0], aw.PYRAMID_POSES[4]]
    return [aw.POSES[0], aw.POSES[4]] + ([ON_ZERO_POSE] if R == 256 else [])


def uniforms(po, name, R, pose, seed=7):
    """The uniforms of pose PLAIN, SCROLLED or ON_ZERO (False and True read as the first two)."""
    return aw.pose_uniforms(po, poses(name, R)[int(pose)], R, seed=seed)


def fetch_under(minefield, R, P):
    """The minefield value under each point of P[n, 3] (the sampler of the restatements)."""
    return pl._fetch(np.ascontiguousarray(minefield, dtype=np.uint8).reshape(-1), int(R), np.asarray(P, dtype=f32).reshape(-1, 3))


def light_pairs(planes, u, lights, minefield, W, H, R):
    """How the shadow rays of the (pixel, light) pairs that pass the pair test end, from tests/point_light_ref alone: dict of
    `visible`, `blocked` and `limit` (a part of blocked) counts."""
    lights = np.asarray(lights).reshape(-1)
    surface, P, axis, even = pl.surface_points(planes, u, W, H)
    Pf = P.reshape(-1, 3)
    passes, v, dist2, _, _ = pl.pair_terms(Pf, axis.reshape(-1), even.reshape(-1), lights["position"].astype(f32), lights["radius"].astype(f32))
    passes &= surface.reshape(-1)[None, :] & pl.valid(lights)[:, None]
    li, pi = np.nonzero(passes)
    vis, end = pl.trace_visible(minefield, R, tuple(int(x) for x in u.lr[:]), Pf[pi], v[li, pi], dist2[li, pi], ends=True)
    assert np.array_equal(vis, (end == pl.END_REACHED) | (end == pl.END_AIR))
    return dict(visible=int(vis.sum()), blocked=int((~vis).sum()), limit=int((end == pl.END_LIMIT).sum()))


def sun_kinds(planes, u, minefield, W, H, R):
    """(surface bool[H, W], kind int[H, W]): how the sun ray of every surface pixel ends (entity_shadow_ref.AIR, SOLID, LIMIT; -1
    off the surfaces)."""
    surface, P, _, _ = pl.surface_points(planes, u, W, H)
    kind = np.full((H, W), -1, dtype=np.int64)
    kind[surface] = shadow_ref.trace_kind(minefield, R, tuple(int(x) for x in u.lr[:]), P[surface], shadow_ref.sun_of(u)[0])
    return surface, kind


# ---- scattered records ------------------------------------------------------------------------------------------------------------------
def scatter_lights(before, u, W, H, n, seed, rmin=2.0, rmax=12.0):
    """test_gpu_point_lights.scatter's recipe: n lights just off the frame's surfaces — a random surface pixel's P', moved 0.2 to 5
    units along its face's normal (one in ten the other way: into the ground) and up to 1.5 units sideways; radii rmin..rmax, colours
    up to 40 with some zeros."""
    rng = np.random.default_rng(seed)
    surface, P, axis, even = pl.surface_points(before, u, W, H)
    pts, ax, ev = P[surface].astype(np.float64), axis[surface], even[surface]
    assert len(pts) > 100
    j = rng.integers(0, len(pts), n)
    pos = pts[j] + rng.uniform(-1.5, 1.5, (n, 3))
    off = rng.uniform(0.2, 5.0, n) * np.where(ev[j], 1.0, -1.0) * np.where(rng.random(n) < 0.1, -1.0, 1.0)
    pos[np.arange(n), ax[j]] += off
    color = rng.random((n, 3)) * 40.0
    color[rng.random(n) < 0.05] = 0.0
    return render.make_point_lights(pos, rng.uniform(rmin, rmax, n), color)


def midpoints(before, u, W, H, lights, n, rng):
    """n points halfway between a light and a surface point that passes its pair test (float64[n, 3])."""
    surface, P, axis, even = pl.surface_points(before, u, W, H)
    Pf = P[surface]
    passes = pl.pair_terms(Pf, axis[surface], even[surface], lights["position"].astype(f32), lights["radius"].astype(f32))[0] & pl.valid(lights)[:, None]
    li, pi = np.nonzero(passes)
    assert li.size > 0, "no light reaches a surface"
    j = rng.integers(0, li.size, n)
    return 0.5 * (lights["position"][li[j]].astype(np.float64) + Pf[pi[j]].astype(np.float64))


def boxes_at(centres, rng, half=(0.05, 0.5)):
    h = rng.uniform(half[0], half[1], (len(centres), 3))
    b = np.zeros(len(centres), dtype=render.DRAW_BOX_DTYPE)
    b["lo"], b["hi"] = (centres - h).astype(f32), (centres + h).astype(f32)
    b["material"], b["emission"] = 0x1FFFFF, 0xFF000000
    return b


def models_at(centres, sid, seed, extent=STAMP_EXTENT, scales=(0.25, 0.125, 0.5)):
    out = []
    for i, c in enumerate(centres):
        orient, scale = (7 * i + seed) % 48, scales[i % len(scales)]
        e = np.array(se.placed_extent(tuple(extent), orient), dtype=np.float64)
        out.append(one_model(sid, (c - 0.5 * e * scale).astype(f32), scale, orient))
    return model_batch(out)


def occluders(before, u, W, H, lights, nboxes, nmodels, seed, sid):
    """Occluders put on purpose between a light and a surface it reaches (two in three; a single one always), and random ones
    scattered over the surfaces as for the sun's shadows."""
    rng = np.random.default_rng(1000 + seed)
    boxes = models = None
    if nboxes:
        k = max(1, (2 * nboxes) // 3)
        boxes = boxes_at(midpoints(before, u, W, H, lights, k, rng), rng)
        if nboxes > k:
            boxes = np.concatenate([boxes, shadow_ref.scatter_boxes(before, u, W, H, nboxes - k, seed, lift=(0.2, 3.0))])
    if nmodels:
        k = max(1, (2 * nmodels) // 3)
        models = models_at(midpoints(before, u, W, H, lights, k, rng), sid, seed)
        if nmodels > k:
            models = np.concatenate([models, shadow_ref.scatter_models(before, u, W, H, nmodels - k, seed, sid, STAMP_EXTENT, scales=(0.5, 0.125),
                                                                        lift=(0.2, 3.0))])
    return boxes, models


def sun_boxes(before, u, W, H, n, seed):
    """n boxes for the sun's shadows: n - 1 scattered above the surfaces (entity_shadow_ref.scatter_boxes) and one canopy, a box
    that holds the three quarters of the surface points with the lowest x — those pixels are shaded whatever their sun ray meets,
    so that the world's sun ray decides for many pixels and not only for the few under a small box."""
    boxes = shadow_ref.scatter_boxes(before, u, W, H, n - 1, seed)
    surface, P, _, _ = pl.surface_points(before, u, W, H)
    pts = P[surface].astype(np.float64)
    lo, hi = pts.min(axis=0) - 1.0, pts.max(axis=0) + 1.0
    hi[0] = np.percentile(pts[:, 0], 75.0)
    canopy = np.zeros(1, dtype=render.DRAW_BOX_DTYPE)
    canopy["lo"], canopy["hi"] = lo.astype(f32), hi.astype(f32)
    canopy["material"], canopy["emission"] = 0x1FFFFF, 0xFF000000
    return np.concatenate([boxes, canopy])


def face_lights(n, seed=9):
    """6 n RtProbeLight records: what rt_draw_boxes / rt_draw_stamps light the faces of n entities with."""
    rng = np.random.default_rng(seed)
    out = np.zeros(6 * n, dtype=render.PROBE_LIGHT_DTYPE)
    out["light"] = rng.random((6 * n, 3), dtype=np.float32) * f32(20.0)
    return out


def limit_lights(before, u, W, H, n, seed, radius=1024.0):
    """n lights of the largest radius along the stall direction of the limit window: from a surface pixel with x >= 2049, 3 to 40
    units further along +x — the shadow ray of that pixel has to cross x planes beyond 2048, where it stalls."""
    rng = np.random.default_rng(seed)
    surface, P, _, _ = pl.surface_points(before, u, W, H)
    pts = P[surface].astype(np.float64)
    pts = pts[pts[:, 0] >= LIMIT_LR[0] + 1.0]
    assert len(pts) > 20, "the frame sees no surface in the window's upper half"
    pos = pts[rng.integers(0, len(pts), n)] + rng.uniform(-0.5, 0.5, (n, 3))
    pos[:, 0] += rng.uniform(3.0, 40.0, n)
    pos[:, 2] += rng.uniform(1.0, 6.0, n)
    return render.make_point_lights(pos, radius, rng.random((n, 3)) * 40.0 + 1.0)
