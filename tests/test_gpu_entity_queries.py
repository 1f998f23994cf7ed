"""Entity queries on the GPU (rt_trace_entities, rt_trace_entities_async, rt_pick_entities).  Every comparison is bit for bit, on
every byte of both outputs: the entity part with tests/entity_query_ref.py — which has no cull and tests every entity against every
ray — fed with the world hits of rt_trace_rays / rt_pick_pixels, the world part with those calls themselves.  Ray counts round the
256-thread workgroup and the 64-lane wave, entity counts round the kernel's 64-record batches and the 4096 limit; coherent, incoherent
and poisoned ray sets; both template arms (lr zero and not); the identity with what rt_draw_boxes / rt_draw_stamps put into the
planes; the asynchronous call, its ordering and its staging sets; every refusal; the absence of side effects; tile contexts and the
host mirror."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from raytrace_amd import _lib, abi, render
from tests import draw_boxes_ref as boxes_ref
from tests import entity_query_ref as ref
from tests import entity_query_sets as sets
from tests import stamp_edits as se

pytestmark = pytest.mark.gpu

CACHE, ACC, REP = abi.RT_FLAG_CACHE_PRIMARY, abi.RT_FLAG_ACCUMULATE, abi.RT_FLAG_REPROJECT
POSE = dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.2, sun=0.3)
SHAPES = [(100, 60), (256, 128)]
LR = (16, 0, -8)
f32 = np.float32


def _u(seed=5, lr=(0, 0, 0)):
    return po.camera_uniforms(POSE["origin"], POSE["heading"], POSE["pitch"], POSE["sun"], seed, lr)


def _ctx(scene, noise, W, H, **kw):
    kw.setdefault("flags", CACHE)
    ctx = render.Context(render.make_config(W, H, **kw))
    ctx.upload_world(*scene)
    if noise is not None:
        ctx.upload_noise(noise)
    return ctx


def _all(ctx):
    return {abi.BUFFER_NAMES[b]: ctx.readback(b) for b in range(abi.RT_BUF_COUNT)}


def _dev(records):
    a = np.ascontiguousarray(records)
    return torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], -1).copy()).cuda()


def _code(fn, *a, **kw):
    with pytest.raises(render.RtError) as e:
        fn(*a, **kw)
    return e.value.code


def make_stamps(ctx, specs=sets.SPECS):
    out = {}
    for ext, seed, fill in specs:
        mats, state = sets.stamp_arrays(ext, seed, fill)
        out[ctx.stamp_create(mats, state)] = (mats, state)
    return out


def same_records(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.view(np.uint8).reshape(got.size, -1) != want.view(np.uint8).reshape(want.size, -1)).any(axis=1))[0]
        raise AssertionError("%s: %d of %d records differ, first %s\n got  %s\n want %s" % (what, bad.size, got.size, bad[:8].tolist(), got[bad[0]], want[bad[0]]))


@pytest.fixture(scope="module")
def frame_ctx(procedural_region, blue_noise):
    """One context per frame shape (spp 1 on the small terrain fixture) with the six stamps."""
    made = {}
    for shape in SHAPES:
        ctx = _ctx(procedural_region, blue_noise, *shape, spp=1, depth=2)
        made[shape] = (ctx, make_stamps(ctx))
    yield made
    for ctx, _ in made.values():
        ctx.destroy()


# ---- ray sets -------------------------------------------------------------------------------------------------------------------------
def pixel_rays(u, W, H, n):
    """n of the frame's pixel rays, spread evenly over the frame in row-major order (coherent: neighbours in a wave are neighbours on
    the screen, and the set holds sky and terrain)."""
    d = boxes_ref.directions(u, W, H).reshape(-1, 3)
    pick = np.unique(np.linspace(0, W * H - 1, n).astype(np.int64)) if n < W * H else np.arange(W * H)
    assert pick.size == n
    o = np.repeat(np.array([u.origin[:]], dtype=f32), n, axis=0)
    return o, d[pick]


def random_rays(n, seed):
    """Seeded origins round the camera — above the terrain, inside it, outside the region — and directions all over the sphere."""
    rng = np.random.default_rng(seed)
    o = (np.array(POSE["origin"]) + rng.uniform(-40.0, 40.0, (n, 3))).astype(f32)
    d = rng.normal(size=(n, 3)).astype(f32) * f32(3.0)          # not normalised: the call does that
    return o, d


def zero_component_rays(u, n, seed):
    """Rays from round the camera with one or two direction components exactly zero (of either sign)."""
    rng = np.random.default_rng(seed)
    o = (np.array(POSE["origin"]) + rng.uniform(-3.0, 3.0, (n, 3))).astype(f32)
    d = rng.normal(size=(n, 3)).astype(f32)
    d[:, 1] = np.abs(d[:, 1]) + f32(0.5)                        # mostly along the camera's view (+y)
    kill = rng.integers(0, 4, n)
    d[kill == 0, 0] = 0.0
    d[kill == 1, 2] = -0.0
    d[kill == 2, 0], d[kill == 2, 2] = -0.0, 0.0
    d[kill == 3, 1], d[kill == 3, 0] = 0.0, 0.0
    return o, d


def poison(o, d, seed):
    """NaN, infinite, zero, huge and tiny rays at seeded lanes of an ordinary set (one ray in six)."""
    rng = np.random.default_rng(seed)
    o, d = o.copy(), d.copy()
    lanes = rng.choice(o.shape[0], o.shape[0] // 6, replace=False)
    for j, i in enumerate(lanes):
        k = int(rng.integers(0, 3))
        what = j % 8
        if what == 0: o[i, k] = np.nan
        elif what == 1: d[i, k] = np.nan
        elif what == 2: o[i, k] = np.inf
        elif what == 3: d[i, k] = -np.inf
        elif what == 4: d[i] = 0.0
        elif what == 5: d[i] *= f32(1e30)
        elif what == 6: d[i] *= f32(1e-30)
        else: o[i, k] = f32(3e38)
    return o, d, lanes


# ---- entities placed with the world in view ---------------------------------------------------------------------------------------------
def entities_for(o, d, world, nboxes, nmodels, stamps, seed, max_diag=40.0):
    """Boxes and models anchored on the rays themselves: a third in front of what the ray's world hit leaves visible, a third behind a
    terrain hit (the world occludes them), a third on rays that leave the region (reported under the sky)."""
    rng = np.random.default_rng(seed)
    o64, d64 = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    with np.errstate(all="ignore"):
        norm = np.linalg.norm(d64, axis=1)
        fine = np.isfinite(o64).all(axis=1) & np.isfinite(d64).all(axis=1) & (norm > 1e-3) & (norm < 1e3) & (np.abs(o64).max(axis=1) < 1e4)
        dist = world["distance"].astype(np.float64)
        sky = fine & (world["kind"] == abi.RT_HIT_AIR)
        ground = fine & (world["kind"] == abi.RT_HIT_SOLID) & (dist > 12.0) & (dist < 400.0)
    assert sky.any() and ground.any(), "the ray set must hold rays that leave the region and rays that meet terrain"
    n = nboxes + nmodels
    role = np.arange(n) % 3
    rng.shuffle(role)
    sky_i, ground_i = np.nonzero(sky)[0], np.nonzero(ground)[0]
    # a terrain ray carries entities in front of its hit or behind it, not both: the nearest entity of a ray decides what it reports
    front_i, behind_i = (ground_i[0::2], ground_i[1::2]) if ground_i.size > 1 else (ground_i, ground_i)
    ray = np.where(role == 2, sky_i[rng.integers(0, sky_i.size, n)],
                   np.where(role == 0, front_i[rng.integers(0, front_i.size, n)], behind_i[rng.integers(0, behind_i.size, n)]))
    a, dn = dist[ray], d64[ray] / norm[ray][:, None]
    boxes = np.zeros(nboxes, dtype=render.DRAW_BOX_DTYPE)
    half = rng.uniform(0.15, 1.0, (nboxes, 3))
    models = np.zeros(nmodels, dtype=render.DRAW_STAMP_DTYPE)
    ids = np.array(sorted(stamps), dtype=np.uint32)
    models["stamp"], models["orient"] = ids[rng.integers(0, ids.size, nmodels)], rng.integers(0, 48, nmodels)
    models["emission"] = rng.integers(0, 1 << 32, nmodels, dtype=np.uint64)
    size = np.zeros((n, 3))
    size[:nboxes] = 2.0 * half
    for i in range(nmodels):
        ext = np.array(se.placed_extent(se.extent_of(stamps[int(models["stamp"][i])][1]), int(models["orient"][i])), dtype=np.float64)
        fits = [s for s in sets.SCALES if np.linalg.norm(ext) * s <= max_diag] or [min(sets.SCALES)]   # (the 256-long stamp only at its small scales)
        models["scale"][i] = fits[int(rng.integers(0, len(fits)))]
        size[nboxes + i] = ext * float(models["scale"][i])
    diag = np.linalg.norm(size, axis=1)
    # the anchor: in front of the hit and clear of the origin, behind the hit, or anywhere within sight under the sky
    nearest = 1.2 * diag + 3.0
    t = np.where(role == 0, np.clip(a * rng.uniform(0.2, 0.7, n), nearest, np.maximum(nearest, a - diag - 2.0)),
                 np.where(role == 1, a + rng.uniform(4.0, 30.0, n) + diag, np.maximum(np.exp(rng.uniform(np.log(8.0), np.log(300.0), n)), nearest)))
    c = o64[ray] + dn * t[:, None]
    lo = c - rng.uniform(0.35, 0.65, (n, 3)) * size                                  # the anchor lies in the box, near its middle
    boxes["lo"], boxes["hi"] = lo[:nboxes].astype(f32), (lo[:nboxes] + size[:nboxes]).astype(f32)
    boxes["material"], boxes["emission"] = rng.integers(1, 1 << 21, nboxes), rng.integers(0, 1 << 32, nboxes, dtype=np.uint64)
    models["origin"] = lo[nboxes:].astype(f32)
    return boxes, models


def check_input_is_not_trivial(info, n, what):
    """The issue's three properties of a parametrisation that uses entities, asserted from the reference."""
    shown = info["hit"] & ~info["occluded"]
    assert np.count_nonzero(shown) >= 0.05 * n, "%s: %d of %d rays report an entity" % (what, np.count_nonzero(shown), n)
    assert info["occluded"].any(), "%s: no ray's entity is occluded by the world" % what
    assert info["under_sky"].any(), "%s: no reported entity lies under the sky" % what


def run_parity(ctx, stamps, o, d, nboxes, nmodels, lr, seed, what):
    world_want = ctx.trace_rays(o, d, lr)
    # (thousands of models on a few hundred rays: small ones, or every ray's nearest model stands in front of the terrain)
    boxes, models = entities_for(o, d, world_want, nboxes, nmodels, stamps, seed, 3.0 if nmodels > 1000 else 40.0) if nboxes + nmodels else (None, None)
    world, hits = ctx.trace_entities(o, d, lr, boxes, models)
    same_records(world, world_want, what + ": world part against rt_trace_rays")
    want, info = ref.trace(o, d, world_want, boxes, models, stamps, details=True)
    same_records(hits, want, what)
    if nboxes + nmodels:
        check_input_is_not_trivial(info, o.shape[0], what)
    return hits, info


# ---- 3. parity with the reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrays", [1, 63, 64, 65, 257, 5000])
@pytest.mark.parametrize("lr", [(0, 0, 0), LR], ids=["lr0", "lr"])
def test_ray_counts_equal_the_restatement(nrays, lr, frame_ctx):
    W, H = SHAPES[0]
    ctx, stamps = frame_ctx[SHAPES[0]]
    o, d = pixel_rays(_u(), W, H, max(nrays, 2))
    o, d = o[-nrays:], d[-nrays:]                            # (one ray: the frame's last pixel, under the sky)
    if nrays == 1:
        # one ray cannot be reported and occluded at once: its entities are another set's with one box on the ray itself, and of the
        # three properties the one that can hold is asked of it — the ray reports an entity, under the sky
        oo, dd = pixel_rays(_u(), W, H, 400)
        boxes, models = entities_for(oo, dd, ctx.trace_rays(oo, dd, lr), 65, 65, stamps, 7)
        centre = o[0].astype(np.float64) + ref.normalize3(d)[0].astype(np.float64) * 12.0
        boxes = np.concatenate([boxes, render.make_draw_boxes([centre - 0.5], [centre + 0.5], 0x777)])
        world, hits = ctx.trace_entities(o, d, lr, boxes, models)
        want_world = ctx.trace_rays(o, d, lr)
        same_records(world, want_world, "one ray: world")
        want, info = ref.trace(o, d, want_world, boxes, models, stamps, details=True)
        same_records(hits, want, "one ray")
        assert hits[0]["kind"] != abi.RT_ENTITY_NONE and info["under_sky"][0]
        return
    run_parity(ctx, stamps, o, d, 65, 65, lr, 100 + nrays, "%d pixel rays" % nrays)


ENTITY_COUNTS = [(0, 0), (1, 0), (0, 1), (63, 0), (0, 63), (63, 63), (64, 0), (0, 64), (64, 64), (65, 0), (0, 65), (65, 65), (130, 0), (0, 130), (130, 130),
                 (4096, 0), (0, 4096), (4096, 4096)]


@pytest.mark.parametrize("nboxes, nmodels", ENTITY_COUNTS, ids=["%db%dm" % c for c in ENTITY_COUNTS])
@pytest.mark.parametrize("rays", ["pixels", "random"])
def test_entity_counts_equal_the_restatement(rays, nboxes, nmodels, frame_ctx):
    W, H = SHAPES[0]
    ctx, stamps = frame_ctx[SHAPES[0]]
    many = max(nboxes, nmodels) == 4096
    # incoherent rays meet few entities each: their number follows the entities', so that the set's share of reporting rays holds
    n = (256 if nmodels == 4096 else 512) if many else (5000 if rays == "pixels" else min(5000, max(8 * (nboxes + nmodels), 512)))
    lr = LR if (nboxes + nmodels) % 2 else (0, 0, 0)
    o, d = pixel_rays(_u(), W, H, n) if rays == "pixels" else random_rays(n, 900 + nboxes + nmodels)
    if nboxes + nmodels == 1:
        # one entity cannot meet the three properties among rays that were there before it: the rays are aimed at it instead — from
        # round the camera (reported, under the sky), from inside the terrain behind other rays' hits (occluded), and the set's own
        world = ctx.trace_rays(o, d, lr)
        sky = np.nonzero((world["kind"] == abi.RT_HIT_AIR) & np.isfinite(o).all(axis=1))[0]
        ground = np.nonzero((world["kind"] == abi.RT_HIT_SOLID) & (world["distance"] > 5) & (world["distance"] < 300))[0]
        dn = ref.normalize3(d)
        centre = o[sky[0]].astype(np.float64) + dn[sky[0]].astype(np.float64) * 25.0
        rng = np.random.default_rng(5)
        solid_id = sorted(stamps)[1]                          # the 12 x 5 x 7 stamp is solid throughout
        if nboxes:
            boxes, models = render.make_draw_boxes([centre - 2.0], [centre + 2.0], 0x4321), None
        else:
            boxes, models = None, render.make_draw_stamps(solid_id, [centre - (3.0, 1.25, 1.75)], 0.5, 0)
        aimed = n // 3
        target = centre + rng.uniform(-1.2, 1.2, (2 * aimed, 3))
        near = o[sky[0]].astype(np.float64) + rng.uniform(-1.0, 1.0, (aimed, 3))
        g = ground[rng.integers(0, ground.size, aimed)]
        buried = world["position"][g].astype(np.float64) + dn[g].astype(np.float64) * 3.0
        o, d = o.copy(), d.copy()
        o[:aimed], d[:aimed] = near, target[:aimed] - near
        o[aimed:2 * aimed], d[aimed:2 * aimed] = buried, target[aimed:] - buried
        world_want = ctx.trace_rays(o, d, lr)
        world_got, hits = ctx.trace_entities(o, d, lr, boxes, models)
        same_records(world_got, world_want, "one entity: world")
        want, info = ref.trace(o, d, world_want, boxes, models, stamps, details=True)
        same_records(hits, want, "one entity")
        check_input_is_not_trivial(info, n, "one entity")
        return
    run_parity(ctx, stamps, o, d, nboxes, nmodels, lr, 300 + nboxes + 7 * nmodels, "%s rays, %d boxes, %d models" % (rays, nboxes, nmodels))


@pytest.mark.parametrize("lr", [(0, 0, 0), LR], ids=["lr0", "lr"])
def test_rays_that_start_inside_entities(lr, frame_ctx):
    W, H = SHAPES[0]
    ctx, stamps = frame_ctx[SHAPES[0]]
    o, d = pixel_rays(_u(), W, H, 257)
    boxes, models = entities_for(o, d, ctx.trace_rays(o, d, lr), 70, 70, stamps, 41)
    rng = np.random.default_rng(3)
    # a ray from the middle of every box and of every bounding box, towards the camera's view and away from it; the set's own rays too
    ext = np.array([se.placed_extent(se.extent_of(stamps[int(m["stamp"])][1]), int(m["orient"])) for m in models], dtype=np.float64)
    inside = np.concatenate([(boxes["lo"].astype(np.float64) + boxes["hi"]) / 2, models["origin"] + ext * models["scale"][:, None].astype(np.float64) * 0.5])
    oo = np.concatenate([inside, o]).astype(f32)
    dd = np.concatenate([rng.normal(size=inside.shape), d]).astype(f32)
    world_want = ctx.trace_rays(oo, dd, lr)
    world, hits = ctx.trace_entities(oo, dd, lr, boxes, models)
    same_records(world, world_want, "inside: world")
    want, info = ref.trace(oo, dd, world_want, boxes, models, stamps, details=True)
    same_records(hits, want, "rays from inside entities")
    own = np.arange(70)
    assert not ((hits["kind"][:70] == abi.RT_ENTITY_BOX) & (hits["index"][:70] == own)).any()       # no box is hit from inside itself
    assert not ((hits["kind"][70:140] == abi.RT_ENTITY_MODEL) & (hits["index"][70:140] == own)).any()
    check_input_is_not_trivial(info, oo.shape[0], "inside")


def test_rays_with_zero_components(frame_ctx):
    ctx, stamps = frame_ctx[SHAPES[0]]
    o, d = zero_component_rays(_u(), 300, 8)
    assert ((d == 0).sum(axis=1) == 1).any() and ((d == 0).sum(axis=1) == 2).any()
    hits, info = run_parity(ctx, stamps, o, d, 130, 130, (0, 0, 0), 55, "zero components")
    zero = (d == 0).any(axis=1)
    assert (hits["kind"][zero] != abi.RT_ENTITY_NONE).any() and (hits["kind"][zero] == abi.RT_ENTITY_NONE).any()


@pytest.mark.parametrize("lr", [(0, 0, 0), LR], ids=["lr0", "lr"])
def test_poisoned_lanes_in_a_wave_of_ordinary_rays(lr, frame_ctx):
    W, H = SHAPES[0]
    ctx, stamps = frame_ctx[SHAPES[0]]
    o, d = pixel_rays(_u(), W, H, 192)                        # three waves
    o, d, lanes = poison(o, d, 17)
    hits, info = run_parity(ctx, stamps, o, d, 100, 100, lr, 23, "poisoned lanes")
    assert (hits["kind"][lanes] == abi.RT_ENTITY_NONE).all()                   # such a ray hits no entity
    keep = np.setdiff1d(np.arange(192), lanes)
    assert (hits["kind"][keep] != abi.RT_ENTITY_NONE).sum() >= 10              # and takes nothing from its neighbours


# ---- 4. the world part ------------------------------------------------------------------------------------------------------------------
def test_world_part_and_null_world_hits(frame_ctx):
    W, H = SHAPES[1]
    ctx, stamps = frame_ctx[SHAPES[1]]
    lib = _lib.amd()
    for lr in ((0, 0, 0), LR):
        u = _u(lr=lr)
        xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2)[::7].astype(np.int32)
        picks = ctx.pick_pixels(u, xy)
        o, d = pixel_rays(u, W, H, 3000)
        boxes, models = entities_for(o, d, ctx.trace_rays(o, d, lr), 40, 40, stamps, 3)
        world, hits = ctx.pick_entities(u, xy, boxes, models)
        same_records(world, picks, "rt_pick_entities' world part against rt_pick_pixels")
        same_records(hits, ref.pick(u, xy, W, H, picks, boxes, models, stamps), "rt_pick_entities")
        # world_hits = NULL: the same entity hits
        alone = np.full(xy.shape[0], 0x5A5A5A5A, dtype=np.uint32).repeat(12).view(render.ENTITY_HIT_DTYPE)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.rt_pick_entities(ctx.handle, C.byref(u), p(xy), xy.shape[0], p(boxes), boxes.size, p(models), models.size, None, p(alone)) == abi.RT_OK
        same_records(alone, hits, "world_hits = NULL (pixels)")
        rays = np.zeros((o.shape[0], 8), dtype=f32)
        rays[:, 0:3], rays[:, 4:7] = o, d
        alone = np.full(o.shape[0], 0x5A5A5A5A, dtype=np.uint32).repeat(12).view(render.ENTITY_HIT_DTYPE)
        lr3 = (C.c_int32 * 3)(*lr)
        assert lib.rt_trace_entities(ctx.handle, p(rays), o.shape[0], lr3, p(boxes), boxes.size, p(models), models.size, None, p(alone)) == abi.RT_OK
        same_records(alone, ctx.trace_entities(o, d, lr, boxes, models)[1], "world_hits = NULL (rays)")


# ---- 5. identity with the draws ---------------------------------------------------------------------------------------------------------
def some_lights(n, seed=9):
    rng = np.random.default_rng(seed)
    out = np.zeros(6 * n, dtype=render.PROBE_LIGHT_DTYPE)
    out["light"] = rng.random((6 * n, 3), dtype=np.float32) * f32(20.0)
    return out


@pytest.mark.parametrize("kind", ["boxes", "models"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_a_pixels_entity_is_the_one_the_draw_put_there(shape, kind, frame_ctx):
    W, H = shape
    ctx, stamps = frame_ctx[shape]
    u = _u()
    ctx.draw_frame(u)
    ctx.sync()
    before = _all(ctx)
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)
    o = np.repeat(np.array([u.origin[:]], dtype=f32), W * H, axis=0)
    # D is the depth plane, bitwise, at every pixel: through a call without entities and its world hits
    world, none = ctx.pick_entities(u, xy)
    assert (none["kind"] == abi.RT_ENTITY_NONE).all()
    assert ref.world_depth(o, world).reshape(H, W).tobytes() == before["depth_f32"].tobytes()
    d = boxes_ref.directions(u, W, H).reshape(-1, 3)
    boxes, models = entities_for(o, d, world, 90 if kind == "boxes" else 0, 0 if kind == "boxes" else 90, stamps, 61)
    if kind == "boxes":
        ctx.draw_boxes(u, boxes, some_lights(90))
        models = None
    else:
        ctx.draw_stamps(u, models, some_lights(90))
        boxes = None
    after = _all(ctx)
    world2, hits = ctx.pick_entities(u, xy, boxes, models)
    same_records(world2, world, "the world part does not see the draw")
    drawn = (after["depth_f32"].view(np.uint32) != before["depth_f32"].view(np.uint32)).reshape(-1)
    is_entity = hits["kind"] == (abi.RT_ENTITY_BOX if kind == "boxes" else abi.RT_ENTITY_MODEL)
    assert np.array_equal(drawn, is_entity) and (hits["kind"][~is_entity] == abi.RT_ENTITY_NONE).all()
    assert drawn.sum() > 0.02 * W * H and (before["depth_r16"].reshape(-1)[drawn] == 65535).any() and (before["depth_r16"].reshape(-1)[drawn] != 65535).any()
    h = hits[drawn]
    assert np.array_equal(after["normal_r8"].reshape(-1)[drawn], h["normal"].astype(np.uint8))
    diff = (o[drawn] - h["position"]).astype(f32)
    depth = (boxes_ref.length3(diff[:, 0], diff[:, 1], diff[:, 2]) * f32(32.0)).astype(f32)
    assert depth.tobytes() == after["depth_f32"].reshape(-1)[drawn].tobytes()
    assert np.array_equal(after["albedo_rgba8"].reshape(W * H, -1)[drawn].view(np.uint8).reshape(-1, 4), boxes_ref.albedo_rgba8(h["material"]))


# ---- 6. the asynchronous call -----------------------------------------------------------------------------------------------------------
def _rays8(o, d):
    rays = np.zeros((o.shape[0], 8), dtype=f32)
    rays[:, 0:3], rays[:, 4:7] = o, d
    return rays


def test_async_equals_sync_and_skips_invalid_boxes(frame_ctx):
    W, H = SHAPES[0]
    ctx, stamps = frame_ctx[SHAPES[0]]
    o, d = pixel_rays(_u(), W, H, 1500)
    boxes, models = entities_for(o, d, ctx.trace_rays(o, d), 96, 96, stamps, 71)
    world, hits = ctx.trace_entities(o, d, (0, 0, 0), boxes, models)
    d_rays, d_boxes = torch.from_numpy(_rays8(o, d)).cuda(), _dev(boxes)
    d_world = torch.full((1500, 48), 0x5A, dtype=torch.uint8, device="cuda")
    d_hits = torch.full((1500, 12), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.trace_entities_async(d_rays, d_boxes, models, d_world, d_hits)
    ctx.sync()
    same_records(d_world.cpu().numpy().view(render.HIT_DTYPE).reshape(-1), world, "async world hits")
    same_records(d_hits.cpu().numpy().view(render.ENTITY_HIT_DTYPE).reshape(-1), hits, "async entity hits")
    # without world hits and without boxes; then invalid boxes, which the device skips
    d_hits.fill_(0x5A5A5A5A)
    ctx.trace_entities_async(d_rays, None, models, None, d_hits)
    ctx.sync()
    same_records(d_hits.cpu().numpy().view(render.ENTITY_HIT_DTYPE).reshape(-1), ctx.trace_entities(o, d, (0, 0, 0), None, models)[1], "async, models only")
    bad = boxes.copy()
    bad["hi"][::5, 1] = bad["lo"][::5, 1]
    bad["lo"][1::5, 0] = np.nan
    bad["hi"][2::5, 2] = 4194305.0
    valid = np.ones(96, dtype=bool)
    valid[::5] = valid[1::5] = valid[2::5] = False
    ctx.trace_entities_async(d_rays, _dev(bad), None, None, d_hits)
    ctx.sync()
    got = d_hits.cpu().numpy().view(render.ENTITY_HIT_DTYPE).reshape(-1)
    want = ctx.trace_entities(o, d, (0, 0, 0), boxes[valid], None)[1]
    want["index"] = np.where(want["kind"] == abi.RT_ENTITY_BOX, np.nonzero(valid)[0][np.minimum(want["index"], valid.sum() - 1)], want["index"])
    same_records(got, want, "invalid boxes are skipped on the device")
    assert (got["kind"] == abi.RT_ENTITY_BOX).any()
    assert _code(ctx.trace_entities, o, d, (0, 0, 0), bad, None) == abi.RT_ERR_INVALID_ARG            # the synchronous call refuses them


def test_a_query_behind_an_edit_sees_it(procedural_region, blue_noise):
    mats, mine = procedural_region
    with _ctx(procedural_region, blue_noise, 64, 40, spp=1, depth=2) as ctx:
        o, d = pixel_rays(_u(), 64, 40, 64 * 40)
        first = ctx.trace_rays(o, d)
        i = int(np.nonzero((first["kind"] == abi.RT_HIT_SOLID) & (first["distance"] > 20) & (first["texel"][:, 0] >= 0))[0][0])
        texel = tuple(int(v) for v in first["texel"][i])
        # a box just behind the surface the ray meets: occluded until the surface is edited away
        dn = ref.normalize3(d[i:i + 1])[0].astype(np.float64)
        c = o[i].astype(np.float64) + dn * (float(first["distance"][i]) + 0.45)
        boxes = render.make_draw_boxes([c - 0.2], [c + 0.2], 0x1111)
        d_rays, d_boxes = torch.from_numpy(_rays8(o[i:i + 1], d[i:i + 1])).cuda(), _dev(boxes)
        d_a = torch.zeros((1, 48), dtype=torch.uint8, device="cuda")
        d_b = torch.zeros((1, 48), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.trace_entities_async(d_rays, d_boxes, None, None, d_a)
        ctx.edit_voxels([texel], [0], [0])                   # no host wait on either side
        ctx.trace_entities_async(d_rays, d_boxes, None, None, d_b)
        ctx.sync()
        a, b = (t.cpu().numpy().view(render.ENTITY_HIT_DTYPE).reshape(-1)[0] for t in (d_a, d_b))
        assert a["kind"] == abi.RT_ENTITY_NONE and b["kind"] == abi.RT_ENTITY_BOX
        world, hits = ctx.trace_entities(o[i:i + 1], d[i:i + 1], (0, 0, 0), boxes, None)
        assert hits[0].tobytes() == b.tobytes() and tuple(int(v) for v in world[0]["texel"]) != texel


def test_a_query_straight_behind_a_capture_reads_the_whole_stamp(procedural_region, blue_noise):
    """rt_stamp_capture writes the stamp's arrays on the render stream, behind the frames; the query reads them on the query stream."""
    W, H = 256, 128
    u = _u()
    with _ctx(procedural_region, blue_noise, W, H, spp=4, depth=3) as ctx:
        o, d = pixel_rays(u, W, H, W * H)
        world = ctx.trace_rays(o, d)
        lo, ext = (0, 0, 0), (256, 256, 256)                 # the largest stamp there is — the whole region — so that the capture takes its time
        scale = 1.0 / 16.0
        sky = np.nonzero(world["kind"] == abi.RT_HIT_AIR)[0]
        anchor = o[sky[sky.size // 2]].astype(np.float64) + ref.normalize3(d)[sky[sky.size // 2]].astype(np.float64) * 40.0
        d_rays = torch.from_numpy(_rays8(o, d)).cuda()
        d_a = torch.zeros((W * H, 48), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for _ in range(3):
            ctx.draw_frame(u)                                 # the capture queues behind frames
        sid = ctx.stamp_capture(lo, ext, abi.RT_STAMP_SKIP_AIR)
        models = render.make_draw_stamps(sid, [anchor - 8.0], scale, 5)
        ctx.trace_entities_async(d_rays, None, models, None, d_a)      # no host wait in between
        ctx.sync()
        got = d_a.cpu().numpy().view(render.ENTITY_HIT_DTYPE).reshape(-1)
        want = ctx.trace_entities(o, d, (0, 0, 0), None, models)[1]    # the same query, the capture long done
        same_records(got, want, "a query straight behind rt_stamp_capture")
        mats, state = ctx.stamp_read(sid)
        same_records(got, ref.trace(o, d, world, None, models, {sid: (mats, state)}), "... and the restatement on the stamp as read back")
        assert (got["kind"] == abi.RT_ENTITY_MODEL).sum() > 100
        ctx.stamp_destroy(sid)


def test_check_entity_query_tensors_refuses_sizes_alignment_and_counts():
    rays = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    hits = torch.zeros((4, 48), dtype=torch.uint8, device="cuda")
    boxes = torch.zeros((2, 8), dtype=torch.float32, device="cuda")
    check = render.check_entity_query_tensors
    assert check(rays, boxes, hits, hits.clone(), 0) == (4, 2) and check(rays, None, None, hits, 0) == (4, 0)
    for bad_rays in (torch.zeros((4, 7), dtype=torch.float32, device="cuda"), torch.zeros((4, 8), dtype=torch.float64, device="cuda"),
                     torch.zeros(32, dtype=torch.float32, device="cuda"), torch.zeros((8, 8), dtype=torch.float32, device="cuda")[::2]):
        with pytest.raises(ValueError, match="rays must be"):
            check(bad_rays, None, None, hits, 0)
    for name, w, e in (("entity_hits", None, torch.zeros((3, 48), dtype=torch.uint8, device="cuda")),
                       ("entity_hits", None, torch.zeros((4, 12), dtype=torch.int16, device="cuda")),
                       ("world_hits", torch.zeros((5, 48), dtype=torch.uint8, device="cuda"), hits)):
        with pytest.raises(ValueError, match=name + " must be a contiguous tensor of N \\* 48 bytes"):
            check(rays, None, w, e, 0)
    with pytest.raises(ValueError, match="entity_hits must be contiguous"):
        check(rays, None, None, torch.zeros((4, 96), dtype=torch.uint8, device="cuda")[:, ::2], 0)
    off = torch.zeros(4 * 48 + 16, dtype=torch.uint8, device="cuda")
    for name, args in (("entity_hits", (rays, None, None, off[4:4 + 192])), ("world_hits", (rays, None, off[8:8 + 192], hits)),
                       ("rays", (torch.zeros(33, dtype=torch.float32, device="cuda")[1:].view(4, 8), None, None, hits)),
                       ("boxes", (rays, torch.zeros(17, dtype=torch.float32, device="cuda")[1:], None, hits))):
        with pytest.raises(ValueError, match=name + " must be 16-byte aligned"):
            check(*args, 0)
    with pytest.raises(ValueError, match="whole 32-byte"):
        check(rays, torch.zeros(12, dtype=torch.float32, device="cuda"), None, hits, 0)
    with pytest.raises(ValueError, match="at most 4096 boxes"):
        check(rays, torch.zeros((4097, 8), dtype=torch.float32, device="cuda"), None, hits, 0)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="cuda:0"):
            check(rays.to("cuda:1"), None, None, hits, 0)


def test_draw_query_and_shadow_back_to_back_read_their_own_records(procedural_region, blue_noise):
    """The three share two staging sets in call order; the query's records go to the query stream, the others' to the frame's."""
    W, H = 60, 36
    u = _u()
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)
    o, d = pixel_rays(u, W, H, W * H)
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as a, _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as b:
        stamps_a, stamps_b = make_stamps(a), make_stamps(b)
        assert sorted(stamps_a) == sorted(stamps_b)
        world = a.trace_rays(o, d)
        sets3 = [entities_for(o, d, world, 0, n, stamps_a, 80 + n)[1] for n in (40, 1100, 70)]     # the query's set makes a staging set grow
        lights = some_lights(40)
        d_lights, d_rays = _dev(lights), torch.from_numpy(_rays8(o, d)).cuda()
        d_hits = torch.zeros((W * H, 48), dtype=torch.uint8, device="cuda")
        for rounds in range(2):                                                                       # the second round finds the sets grown and in use
            a.draw_frame(u)
            torch.cuda.synchronize()
            a.draw_stamps_async(u, sets3[0], d_lights)
            a.trace_entities_async(d_rays, None, sets3[1], None, d_hits)
            a.shadow_entities_async(u, None, sets3[2], 0.75)
            a.sync()
            got_planes, got_hits = _all(a), d_hits.cpu().numpy().view(render.ENTITY_HIT_DTYPE).reshape(-1)
            b.draw_frame(u)
            b.sync()
            b.draw_stamps(u, sets3[0], lights)
            want_hits = b.trace_entities(o, d, (0, 0, 0), None, sets3[1])[1]
            b.shadow_entities(u, None, sets3[2], 0.75)
            want_planes = _all(b)
            same_records(got_hits, want_hits, "the query between a draw and a shadow pass")
            for name in want_planes:
                assert got_planes[name].tobytes() == want_planes[name].tobytes(), name
            assert (got_hits["kind"] == abi.RT_ENTITY_MODEL).sum() > 50
            assert got_planes["depth_f32"].tobytes() != _fresh(b, u)["depth_f32"].tobytes()


def _fresh(ctx, u):
    ctx.draw_frame(u)
    ctx.sync()
    return _all(ctx)


def test_stamp_destroy_straight_after_an_async_query(frame_ctx):
    W, H = SHAPES[1]
    ctx, _ = frame_ctx[SHAPES[1]]
    stamps = make_stamps(ctx, [((12, 12, 12), 31, 0.2), ((9, 9, 12), 32, 0.3)])
    o, d = pixel_rays(_u(), W, H, W * H)
    models = entities_for(o, d, ctx.trace_rays(o, d), 0, 600, stamps, 51)[1]
    want = ctx.trace_entities(o, d, (0, 0, 0), None, models)[1]
    d_rays = torch.from_numpy(_rays8(o, d)).cuda()
    d_hits = torch.zeros((W * H, 48), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.trace_entities_async(d_rays, None, models, None, d_hits)
    for s in stamps:
        ctx.stamp_destroy(s)                                   # waits for the query; the arrays are freed after it
    fill = [ctx.stamp_create(*sets.stamp_arrays((12, 12, 12), 90 + k, 1.0)) for k in range(4)]     # what reuses the freed memory is not seen
    ctx.sync()
    same_records(d_hits.cpu().numpy().view(render.ENTITY_HIT_DTYPE).reshape(-1), want, "query, then destroy")
    assert (want["kind"] == abi.RT_ENTITY_MODEL).sum() > 200
    assert _code(ctx.trace_entities, o, d, (0, 0, 0), None, models) == abi.RT_ERR_INVALID_ARG
    for s in fill:
        ctx.stamp_destroy(s)


# ---- 7. refusals and side effects -------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(procedural_region, blue_noise):
    W, H = 64, 40
    lib = _lib.amd()
    u = _u()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lr3 = (C.c_int32 * 3)(0, 0, 0)
    ctx = render.Context(render.make_config(W, H, spp=1, depth=2, flags=CACHE))
    try:
        h = ctx.handle
        rays = _rays8(*pixel_rays(u, W, H, 8))
        xy = np.array([[0, 0], [63, 39], [5, 7], [9, 9], [1, 1], [2, 2], [3, 3], [4, 4]], dtype=np.int32)
        boxes = render.make_draw_boxes([[-31, -100, 99]], [[-29, -98, 101]], 5)
        world = np.full(8, 0x5A5A5A5A, dtype=np.uint32).repeat(12).view(render.HIT_DTYPE)
        hits = np.full(8, 0x5A5A5A5A, dtype=np.uint32).repeat(12).view(render.ENTITY_HIT_DTYPE)
        untouched = (world.tobytes(), hits.tobytes())
        # no world resident: NOT_READY; count == 0 is fine all the same
        assert lib.rt_trace_entities(h, p(rays), 8, lr3, p(boxes), 1, None, 0, p(world), p(hits)) == abi.RT_ERR_NOT_READY
        assert lib.rt_pick_entities(h, C.byref(u), p(xy), 8, p(boxes), 1, None, 0, p(world), p(hits)) == abi.RT_ERR_NOT_READY
        assert lib.rt_trace_entities(h, None, 0, None, None, 0, None, 0, None, None) == abi.RT_OK
        ctx.upload_world(*procedural_region)                  # no noise and no frame are needed from here on
        stamps = make_stamps(ctx)
        models = render.make_draw_stamps(sorted(stamps)[0], [[-31, -100, 99]], 0.5, 3)
        d_rays, d_boxes = torch.from_numpy(rays).cuda(), _dev(boxes)
        d_world, d_hits = torch.full((8, 48), 0x5A, dtype=torch.uint8, device="cuda"), torch.full((8, 48), 0x5A, dtype=torch.uint8, device="cuda")
        dp = lambda t: C.c_void_p(t.data_ptr())
        torch.cuda.synchronize()
        IA = abi.RT_ERR_INVALID_ARG

        def sync_trace(rays_=p(rays), n=8, lr=lr3, b=p(boxes), nb=1, m=p(models), nm=1, w=p(world), e=p(hits)):
            return lib.rt_trace_entities(h, rays_, n, lr, b, nb, m, nm, w, e)

        def sync_pick(u_=C.byref(u), xy_=p(xy), n=8, b=p(boxes), nb=1, m=p(models), nm=1, w=p(world), e=p(hits)):
            return lib.rt_pick_entities(h, u_, xy_, n, b, nb, m, nm, w, e)

        def async_trace(rays_=dp(d_rays), n=8, lr=lr3, b=dp(d_boxes), nb=1, m=p(models), nm=1, w=dp(d_world), e=dp(d_hits)):
            return lib.rt_trace_entities_async(h, rays_, n, lr, b, nb, m, nm, w, e)

        assert sync_trace() == abi.RT_OK and sync_pick() == abi.RT_OK and async_trace() == abi.RT_OK    # the arguments are fine as they stand
        ctx.sync()
        world[:], hits[:] = np.frombuffer(untouched[0], dtype=render.HIT_DTYPE), np.frombuffer(untouched[1], dtype=render.ENTITY_HIT_DTYPE)
        d_world.fill_(0x5A)
        d_hits.fill_(0x5A)
        for call in (sync_trace, async_trace):
            assert call(rays_=None) == IA and call(lr=None) == IA and call(e=None) == IA
            assert call(b=None) == IA and call(m=None) == IA
            assert call(n=(1 << 24) + 1) == IA and call(nb=4097) == IA and call(nm=4097) == IA
            assert call(w=None) == abi.RT_OK                                                           # world_hits may be NULL
            assert call(n=0, rays_=None, lr=None, e=None, w=None) == abi.RT_OK
            assert call(n=0, nb=4097) == IA
        ctx.sync()
        hits[:] = np.frombuffer(untouched[1], dtype=render.ENTITY_HIT_DTYPE)                           # (the accepted calls wrote them)
        d_hits.fill_(0x5A)
        torch.cuda.synchronize()
        for call in (sync_trace, async_trace):
            assert call(rays_=None) == IA and call(e=None) == IA and call(b=None) == IA and call(nm=4097) == IA and call(n=(1 << 24) + 1) == IA
        assert sync_pick(u_=None) == IA and sync_pick(xy_=None) == IA and sync_pick(e=None) == IA and sync_pick(b=None) == IA and sync_pick(m=None) == IA
        assert sync_pick(n=(1 << 24) + 1) == IA and sync_pick(nb=4097) == IA and sync_pick(nm=4097) == IA
        for bad_xy in ((-1, 0), (0, -1), (W, 0), (0, H)):
            xy2 = xy.copy()
            xy2[5] = bad_xy
            assert sync_pick(xy_=p(xy2)) == IA and "pixel 5" in _lib.amd().rt_last_error(ctx.handle).decode()
        ctx.sync()
        # a model record that is not valid, with models_check's message; an invalid box in the synchronous calls
        for field, value in (("stamp", max(stamps) + 1), ("orient", 48), ("reserved", 1), ("scale", np.nan), ("scale", 64.5), ("origin", (np.inf, 0, 0))):
            bad = models.copy()
            bad[field][0] = value
            for call in (sync_trace, sync_pick, async_trace):
                assert call(m=p(bad)) == IA
                assert "model 0 has an unknown stamp id, orient >= 48" in _lib.amd().rt_last_error(ctx.handle).decode()
        bad_box = boxes.copy()
        bad_box["hi"][0, 1] = bad_box["lo"][0, 1]
        assert sync_trace(b=p(bad_box)) == IA and "box 0 is not a valid box" in _lib.amd().rt_last_error(ctx.handle).decode()
        assert sync_pick(b=p(bad_box)) == IA and "box 0 is not a valid box" in _lib.amd().rt_last_error(ctx.handle).decode()
        # device pointers that fail rt_trace_rays_async's test: host memory, misaligned memory
        assert async_trace(rays_=p(rays)) == IA and async_trace(b=p(boxes)) == IA and async_trace(w=p(world)) == IA and async_trace(e=p(hits)) == IA
        assert async_trace(rays_=C.c_void_p(d_rays.data_ptr() + 4), n=7) == IA and async_trace(e=C.c_void_p(d_hits.data_ptr() + 8), n=7) == IA
        assert async_trace(w=C.c_void_p(d_world.data_ptr() + 4), n=7) == IA
        ctx.sync()
        # nothing was written by any of them, to either output
        assert world.tobytes() == untouched[0] and hits.tobytes() == untouched[1]
        assert (d_world.cpu().numpy() == 0x5A).all() and (d_hits.cpu().numpy() == 0x5A).all()
    finally:
        ctx.destroy()


def test_a_refused_call_leaves_the_entity_hits_alone(frame_ctx):
    ctx, stamps = frame_ctx[SHAPES[0]]
    o, d = pixel_rays(_u(), *SHAPES[0], 100)
    boxes, models = entities_for(o, d, ctx.trace_rays(o, d), 10, 10, stamps, 5)
    lib, p = _lib.amd(), (lambda a: a.ctypes.data_as(C.c_void_p))
    rays = _rays8(o, d)
    hits = np.full(100, 0x5A5A5A5A, dtype=np.uint32).repeat(12).view(render.ENTITY_HIT_DTYPE)
    before = hits.tobytes()
    bad = models.copy()
    bad["orient"][7] = 48
    lr3 = (C.c_int32 * 3)(0, 0, 0)
    assert lib.rt_trace_entities(ctx.handle, p(rays), 100, lr3, p(boxes), 10, p(bad), 10, None, p(hits)) == abi.RT_ERR_INVALID_ARG
    assert "model 7" in _lib.amd().rt_last_error(ctx.handle).decode() and hits.tobytes() == before
    d_hits = torch.full((100, 48), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert lib.rt_trace_entities_async(ctx.handle, C.c_void_p(torch.from_numpy(rays).cuda().data_ptr()), 100, lr3, None, 0, p(bad), 10, None,
                                       C.c_void_p(d_hits.data_ptr())) == abi.RT_ERR_INVALID_ARG
    ctx.sync()
    assert (d_hits.cpu().numpy() == 0x5A).all()


def test_a_query_has_no_side_effects(procedural_region, blue_noise):
    W, H = 96, 64
    cams = [_u(seed=10 + k) for k in range(4)]
    for k, c in enumerate(cams):
        c.origin[0] += 0.25 * k

    def run(query):
        with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2, flags=ACC | REP | CACHE | abi.RT_FLAG_COUNTERS) as ctx:
            stamps = make_stamps(ctx)
            o, d = pixel_rays(cams[0], W, H, 2000)
            boxes, models = entities_for(o, d, ctx.trace_rays(o, d), 30, 30, stamps, 9)
            xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2)[::3].astype(np.int32)
            out = []
            for c in cams:
                ctx.draw_frame(c)
                ctx.sync()
                if query:
                    planes = _all(ctx)
                    state = (ctx.accumulation(), ctx.read_history().tobytes(), bytes(ctx.counters()))
                    ctx.trace_entities(o, d, (0, 0, 0), boxes, models)
                    ctx.pick_entities(c, xy, boxes, models)
                    assert (ctx.accumulation(), ctx.read_history().tobytes(), bytes(ctx.counters())) == state
                    after = _all(ctx)
                    assert all(after[n].tobytes() == planes[n].tobytes() for n in planes)
                out.append((_all(ctx), ctx.accumulation(), ctx.read_history().tobytes(), bytes(ctx.counters())))
            return out

    with_queries, without = run(True), run(False)
    for (pa, acc_a, hist_a, cn_a), (pb, acc_b, hist_b, cn_b) in zip(with_queries, without):
        assert acc_a == acc_b and hist_a == hist_b and cn_a == cn_b
        assert all(pa[n].tobytes() == pb[n].tobytes() for n in pb)              # the next frame's planes too


def test_a_tile_context_answers_like_a_whole_frame_one(procedural_region, blue_noise, frame_ctx):
    W, H = SHAPES[0]
    whole, stamps = frame_ctx[SHAPES[0]]
    u = _u()
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2)[::5].astype(np.int32)
    o, d = pixel_rays(u, W, H, 1000)
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2, tile_rank=1, tile_world=2) as tile:
        tile_stamps = make_stamps(tile)
        assert sorted(tile_stamps) == sorted(stamps)
        boxes, models = entities_for(o, d, whole.trace_rays(o, d), 50, 50, stamps, 13)
        for got, want in zip(tile.pick_entities(u, xy, boxes, models), whole.pick_entities(u, xy, boxes, models)):
            same_records(got, want, "tile context, pixels")
        for got, want in zip(tile.trace_entities(o, d, (0, 0, 0), boxes, models), whole.trace_entities(o, d, (0, 0, 0), boxes, models)):
            same_records(got, want, "tile context, rays")
        assert (want["kind"] != abi.RT_ENTITY_NONE).sum() > 50


def test_every_kernel_route_answers_the_same(procedural_region, blue_noise, frame_ctx):
    W, H = SHAPES[0]
    whole, stamps = frame_ctx[SHAPES[0]]
    o, d = pixel_rays(_u(), W, H, 1000)
    boxes, models = entities_for(o, d, whole.trace_rays(o, d), 50, 50, stamps, 13)
    want = whole.trace_entities(o, d, (0, 0, 0), boxes, models)
    for kernel in (abi.RT_KERNEL_MEGA, abi.RT_KERNEL_WAVEFRONT, abi.RT_KERNEL_PERSISTENT):
        with _ctx(procedural_region, None, W, H, spp=1, depth=2, kernel=kernel) as ctx:
            assert sorted(make_stamps(ctx)) == sorted(stamps)
            for got, w in zip(ctx.trace_entities(o, d, (0, 0, 0), boxes, models), want):
                same_records(got, w, "kernel %d" % kernel)


def test_the_mirror_picks_what_the_context_picks(procedural_region, blue_noise):
    W, H = 96, 64
    cfg = render.make_config(W, H, spp=1, depth=2, flags=CACHE)
    g = render.Game(args=(-30, -128, 100, 1.5707964, -0.15, 0.3))
    g.set_world(*procedural_region)
    pl = render.create_instance(cfg, g, blue_noise)
    try:
        stamps = make_stamps(pl.context)
        pl.draw_frame(g)
        pl.wait()
        u = abi.RtUniforms.from_buffer_copy(bytes(pl.uniforms()))
        xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)
        o = np.repeat(np.array([u.origin[:]], dtype=f32), W * H, axis=0)
        d = boxes_ref.directions(u, W, H).reshape(-1, 3)
        world = pl.context.pick_pixels(u, xy)
        boxes, models = entities_for(o, d, world, 25, 25, stamps, 19)
        pl.set_boxes(boxes, some_lights(25))
        pl.set_models(models, some_lights(25, seed=4))
        _, hits = pl.context.pick_entities(u, xy, boxes, models)
        on_box = int(np.nonzero(hits["kind"] == abi.RT_ENTITY_BOX)[0][0])
        on_model = int(np.nonzero(hits["kind"] == abi.RT_ENTITY_MODEL)[0][0])
        on_terrain = int(np.nonzero((hits["kind"] == abi.RT_ENTITY_NONE) & (world["kind"] == abi.RT_HIT_SOLID))[0][0])
        for i in (on_box, on_model, on_terrain):
            x, y = int(xy[i, 0]), int(xy[i, 1])
            got = pl.pick_entity(x, H - 1 - y)
            assert got["entity"].tobytes() == hits[i].tobytes() and got["hit"].tobytes() == world[i].tobytes()
            plain = pl.pick(g, x, H - 1 - y)
            assert plain["adjacent"] == got["adjacent"] and plain["world"] == got["world"] and plain["hit"].tobytes() == got["hit"].tobytes()
    finally:
        pl.close()
        g.close()
