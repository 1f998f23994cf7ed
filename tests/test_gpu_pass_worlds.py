"""The frame passes, the entity queries and the light probes on the GPU over worlds that terrain cannot give (tests/pass_worlds.py):
rt_add_lights, rt_add_lights_occluded, rt_shadow_entities, rt_draw_boxes, rt_draw_stamps, rt_trace_entities, rt_pick_entities and
rt_probe_light on the arbitrary world (every minefield value 0..30, no distance bound, surface points on 0 texels), the pyramid world
(values above 6), the limit window (rays that stall and end at RT_TRACE_LIMIT) and at regions 512 and 1024, with lr zero and not — so
that every <LOGR, LRZ> build of the kernels runs against its restatement.  Every comparison is bit for bit on all planes and on every
byte of the records.  tests/test_pass_inputs.py checks on the CPU that these inputs reach the branches they are here for; each test
prints the class counts of its own input (pytest -s shows them)."""
import numpy as np
import pytest

from oracle import pyoracle as po
from raytrace_amd import abi, render, world
from tests import adversarial_worlds as aw
from tests import draw_boxes_ref as boxes_ref
from tests import draw_stamps_ref as stamps_ref
from tests import entity_query_ref as eq
from tests import entity_shadow_ref as es
from tests import light_probe_ref as lp
from tests import light_shadow_ref as ls
from tests import pass_worlds as pw
from tests import point_light_ref as pl
from tests.test_gpu_entity_queries import pixel_rays, same_records
from tests.test_gpu_light_probes import _pixel_probes, bits
from tests.test_gpu_ray_queries import _adversarial_rays

pytestmark = pytest.mark.gpu

CACHE = abi.RT_FLAG_CACHE_PRIMARY
PLAIN, SCROLLED, ON_ZERO = pw.PLAIN, pw.SCROLLED, pw.ON_ZERO
SMALL, LARGE = pw.SHAPES
# (world, region, pose, frame shape): the worlds in turn, so that a region above 256 is built once
CASES = [("arbitrary", 256, PLAIN, SMALL), ("arbitrary", 256, SCROLLED, LARGE), ("arbitrary", 256, ON_ZERO, SMALL),
         ("arbitrary", 512, PLAIN, LARGE), ("arbitrary", 512, SCROLLED, SMALL), ("pyramid", 256, SCROLLED, SMALL), ("limit", 256, PLAIN, SMALL)]
f32 = np.float32


def _id(case):
    return "%s%d-pose%d-%dx%d" % (case[0], case[1], case[2], case[3][0], case[3][1])


def _all(ctx):
    return {abi.BUFFER_NAMES[b]: ctx.readback(b) for b in range(abi.RT_BUF_COUNT)}


def _assert_same(got, want, what=""):
    for name in want:
        if got[name].tobytes() != want[name].tobytes():
            a, b = got[name].reshape(got[name].shape[0], got[name].shape[1], -1), want[name].reshape(want[name].shape[0], want[name].shape[1], -1)
            bad = np.argwhere((a.view(np.uint8) != b.view(np.uint8)).any(axis=-1))
            raise AssertionError("%s plane %s differs at %d pixels, first (row, col) %s" % (what, name, len(bad), bad[:5].tolist()))


def _with_final(want, before):
    want["final_bgra8"] = before["final_bgra8"]
    return want


def _without_final(planes):
    return {k: v for k, v in planes.items() if k != "final_bgra8"}


class Stage:
    """The contexts of the module, one per (world, region, shape, spp, depth), each with the small stamp, and the oracle's frames."""

    def __init__(self, noise):
        self.noise, self.ctxs, self.frames = noise, {}, {}

    def ctx(self, name, R, shape, spp=1, depth=2):
        key = (name, R, shape, spp, depth)
        if key not in self.ctxs:
            ctx = render.Context(render.make_config(shape[0], shape[1], spp=spp, depth=depth, flags=CACHE, region=R))
            self.ctxs[key] = (ctx,)                  # (destroyed with the others should the upload fail)
            ctx.upload_world(*pw.world_of(name, R))
            ctx.upload_noise(self.noise)
            mats, state = es.small_stamp()
            sid = ctx.stamp_create(mats, state)
            self.ctxs[key] = (ctx, {sid: (mats, state)}, sid)
        return self.ctxs[key]

    def oracle(self, name, R, pose, shape, spp=1, depth=2):
        key = (name, R, int(pose), shape, spp, depth)
        if key not in self.frames:
            mats, mine = pw.world_of(name, R)
            self.frames[key] = po.render(mats, mine, self.noise, pw.uniforms(po, name, R, pose), shape[0], shape[1], spp, depth, region=R)[0]
        return self.frames[key]

    def frame(self, case):
        """(ctx, stamps, sid, u, before, minefield) of a case: the frame drawn anew, read back and held to the oracle's."""
        name, R, pose, shape = case
        ctx, stamps, sid = self.ctx(name, R, shape)
        u = pw.uniforms(po, name, R, pose)
        ctx.draw_frame(u)
        ctx.sync()
        before = _all(ctx)
        _assert_same(before, self.oracle(name, R, pose, shape), "%s: the frame against the oracle's," % _id(case))
        return ctx, stamps, sid, u, before, pw.world_of(name, R)[1]

    def close(self):
        for made in self.ctxs.values():
            made[0].destroy()


@pytest.fixture(scope="module")
def stage(blue_noise, native_built):
    s = Stage(blue_noise)
    yield s
    s.close()


def _lights(case, before, u, n, seed):
    """n scattered lights, radii 4..40.  In the limit window 16 have radii 4..200 (tests/test_pass_inputs.py: enough for shadow rays
    that end at the limit); of 70 the last three have radius 1024 and lie along the stall direction."""
    W, H = case[3]
    if case[0] == "limit" and n < 70:
        return pw.scatter_lights(before, u, W, H, n, seed, rmin=4.0, rmax=200.0)
    lights = pw.scatter_lights(before, u, W, H, n, seed, rmin=4.0, rmax=40.0)
    if case[0] == "limit":
        lights[-3:] = pw.limit_lights(before, u, W, H, 3, seed)
    return lights


# ---- rt_add_lights ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [16, 70])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_add_lights(case, count, stage):
    (W, H), R = case[3], case[1]
    ctx, stamps, sid, u, before, mine = stage.frame(case)
    lights = _lights(case, before, u, count, 200 + count)
    pairs = pw.light_pairs(before, u, lights, mine, W, H, R)
    print("rt_add_lights %s, %d lights: pairs %s" % (_id(case), count, pairs))
    assert pairs["visible"] > 50 and pairs["blocked"] > 50
    assert case[0] != "limit" or pairs["limit"] >= 20
    want = _with_final(pl.add_lights(_without_final(before), u, lights, mine, W, H, R), before)
    ctx.add_lights(u, lights)
    got = _all(ctx)
    _assert_same(got, want, "%s, %d lights:" % (_id(case), count))
    assert got["lighting_f32"].tobytes() != before["lighting_f32"].tobytes()


# ---- rt_add_lights_occluded ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_add_lights_occluded(case, stage):
    (W, H), R = case[3], case[1]
    ctx, stamps, sid, u, before, mine = stage.frame(case)
    lights = _lights(case, before, u, 16, 3)
    boxes, models = pw.occluders(before, u, W, H, lights, 30, 10, 3, sid)
    classes = {}
    want = _with_final(ls.add_lights_occluded(_without_final(before), u, lights, boxes, models, stamps, mine, W, H, R, classes=classes), before)
    print("rt_add_lights_occluded %s: pairs %s" % (_id(case), classes))
    assert min(classes[k] for k in ("entity_only", "world_only", "both", "visible")) > 0, classes
    ctx.add_lights_occluded(u, lights, boxes, models)
    _assert_same(_all(ctx), want, "%s:" % _id(case))
    unoccluded = pl.add_lights(_without_final(before), u, lights, mine, W, H, R)
    assert unoccluded["lighting_f32"].tobytes() != want["lighting_f32"].tobytes()


def test_add_lights_occluded_with_more_candidates_than_the_list_holds(stage):
    """100 boxes and 70 models round one light on the arbitrary world: every tile the light reaches scans every record (`overflow`)."""
    case = CASES[0]
    (W, H), R = case[3], case[1]
    ctx, stamps, sid, u, before, mine = stage.frame(case)
    lights = pw.scatter_lights(before, u, W, H, 3, 31, rmin=12.0, rmax=20.0)
    rng = np.random.default_rng(31)
    boxes = pw.boxes_at(pw.midpoints(before, u, W, H, lights[:1], 100, rng), rng, half=(0.02, 0.1))
    models = pw.models_at(pw.midpoints(before, u, W, H, lights[:1], 70, rng), sid, 31, scales=(0.0625, 0.03125))
    classes = {}
    want = _with_final(ls.add_lights_occluded(_without_final(before), u, lights, boxes, models, stamps, mine, W, H, R, classes=classes), before)
    print("rt_add_lights_occluded, overflow: pairs %s" % classes)
    assert classes["entity_only"] > 0 and classes["visible"] > 0 and classes["world_only"] > 0
    ctx.add_lights_occluded(u, lights, boxes, models)
    _assert_same(_all(ctx), want, "100 boxes and 70 models round one light:")


# ---- rt_shadow_entities -------------------------------------------------------------------------------------------------------------------
def _sun_occluders(case, before, u, sid, nboxes=40, nmodels=12, seed=3):
    W, H = case[3]
    return (pw.sun_boxes(before, u, W, H, nboxes, seed),
            es.scatter_models(before, u, W, H, nmodels, seed, sid, pw.STAMP_EXTENT, scales=(1.0, 0.125)))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_shadow_entities(case, stage):
    (W, H), R = case[3], case[1]
    ctx, stamps, sid, u, before, mine = stage.frame(case)
    boxes, models = _sun_occluders(case, before, u, sid)
    masks = es.masks(before, u, boxes, models, stamps, mine, W, H, R)
    kinds = pw.sun_kinds(before, u, mine, W, H, R)[1]
    shaded = masks["changed"] | masks["world"]
    at_limit = shaded & (kinds == es.LIMIT)
    print("rt_shadow_entities %s: pixels %s, shaded with a sun ray that ends at the limit %d" % (
        _id(case), {k: int(v.sum()) for k, v in masks.items()}, int(at_limit.sum())))
    assert min(int(masks[k].sum()) for k in ("changed", "world", "open", "sky")) > 0
    want = _with_final(es.shadow_entities(_without_final(before), u, boxes, models, stamps, mine, W, H, R, 0.75, classes=masks), before)
    ctx.shadow_entities(u, boxes, models, 0.75)
    got = _all(ctx)
    _assert_same(got, want, "%s:" % _id(case))
    assert got["lighting_f32"].tobytes() != before["lighting_f32"].tobytes()
    if case[0] == "limit":                             # no sun term to remove where the sun ray ended at the limit
        assert int(at_limit.sum()) >= 50
        for name in before:
            assert got[name][at_limit].tobytes() == before[name][at_limit].tobytes(), name


# ---- rt_draw_boxes, rt_draw_stamps and the passes on top of them ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=_id)
def test_draws_then_shadows_then_lights(case, stage):
    """The mirror's order — boxes, models, sun shadows, lights — compared after every step: the passes find entity pixels whose P' lie
    on the entities' faces, anywhere in the arbitrary world."""
    (W, H), R = case[3], case[1]
    ctx, stamps, sid, u, before, mine = stage.frame(case)
    bare = before
    boxes = es.scatter_boxes(before, u, W, H, 30, 5, lift=(0.5, 3.0))
    boxes["material"] = np.random.default_rng(5).integers(1, 1 << 21, 30)
    models = es.scatter_models(before, u, W, H, 10, 5, sid, pw.STAMP_EXTENT, scales=(1.0, 0.5), lift=(0.5, 3.0))
    box_lights, model_lights = pw.face_lights(30), pw.face_lights(10, seed=4)

    def step(what, call, restate):
        nonlocal before
        want = _with_final(restate(_without_final(before)), before)
        call()
        got = _all(ctx)
        _assert_same(got, want, "%s, %s:" % (_id(case), what))
        before = got

    step("rt_draw_boxes", lambda: ctx.draw_boxes(u, boxes, box_lights), lambda p: boxes_ref.draw_boxes(p, u, boxes, box_lights, W, H))
    step("rt_draw_stamps", lambda: ctx.draw_stamps(u, models, model_lights), lambda p: stamps_ref.draw_stamps(p, u, models, stamps, model_lights, W, H))
    entity = before["depth_f32"].view(np.uint32) != bare["depth_f32"].view(np.uint32)
    print("draws %s: entity pixels %d" % (_id(case), int(entity.sum())))
    assert int(entity.sum()) >= 20
    masks = es.masks(before, u, boxes, models, stamps, mine, W, H, R)
    assert masks["changed"][entity].any() or masks["world"][entity].any()                 # an entity shades an entity's face
    step("rt_shadow_entities", lambda: ctx.shadow_entities(u, boxes, models, 0.75),
         lambda p: es.shadow_entities(p, u, boxes, models, stamps, mine, W, H, R, 0.75, classes=masks))
    lights = pw.scatter_lights(before, u, W, H, 16, 8, rmin=4.0, rmax=40.0)
    lit = pl.add_lights(_without_final(before), u, lights, mine, W, H, R)
    assert (lit["lighting_f32"] != before["lighting_f32"]).any(axis=-1)[entity].any()     # lights reach entity pixels
    step("rt_add_lights", lambda: ctx.add_lights(u, lights), lambda p: pl.add_lights(p, u, lights, mine, W, H, R))
    step("rt_add_lights_occluded", lambda: ctx.add_lights_occluded(u, lights, boxes, models),
         lambda p: ls.add_lights_occluded(p, u, lights, boxes, models, stamps, mine, W, H, R))


# ---- entity queries -----------------------------------------------------------------------------------------------------------------------
def _query_rays(ctx, mats, mine, u, lr, W, H, R, boxes, limit):
    """1500 adversarial rays, the frame's pixel rays, and 32 rays from inside solid voxels aimed at the boxes (their world records
    hold a NaN position: the ray's first texel is 0)."""
    rng = np.random.default_rng(17)
    o, d = _adversarial_rays(rng, mats, mine, lr, 1500, R)
    if limit:                                            # (as tests/test_gpu_ray_queries.py aims them: down, round the camera)
        o[:600] = f32((lr[0] - 30.0, -128.0, 100.0)) + rng.uniform(-4, 4, (600, 3)).astype(f32)
        d[:600, 2] = -np.abs(d[:600, 2]) - f32(0.2)
    po_, pd = pixel_rays(u, W, H, W * H)
    centres = ((boxes["lo"].astype(np.float64) + boxes["hi"]) / 2)[:32]
    buried = o[-32:].astype(np.float64)                  # _adversarial_rays' origins inside solid voxels
    o2, d2 = buried.astype(f32), (centres - buried).astype(f32)
    return np.concatenate([o, po_, o2]), np.concatenate([d, pd, d2])


def _entity_queries(ctx, stamps, sid, u, before, mats, mine, W, H, R, what, limit=False):
    lr = tuple(int(x) for x in u.lr[:])
    boxes = es.scatter_boxes(before, u, W, H, 40, 9)
    boxes["material"] = np.random.default_rng(9).integers(1, 1 << 21, 40)
    models = es.scatter_models(before, u, W, H, 12, 9, sid, pw.STAMP_EXTENT, scales=(1.0, 0.5))
    o, d = _query_rays(ctx, mats, mine, u, lr, W, H, R, boxes, limit)
    world_want = ctx.trace_rays(o, d, lr)                # k_query: pinned to the oracle by tests/test_gpu_ray_queries.py
    world_got, hits = ctx.trace_entities(o, d, lr, boxes, models)
    same_records(world_got, world_want, what + ": world part against rt_trace_rays")
    want, info = eq.trace(o, d, world_want, boxes, models, stamps, details=True)
    same_records(hits, want, what + ": rt_trace_entities")
    shown = info["hit"] & ~info["occluded"]
    with np.errstate(invalid="ignore"):
        odd = (world_want["kind"] == abi.RT_HIT_LIMIT) | np.isnan(world_want["position"]).any(axis=1)
    print("entity queries %s: %d rays, entity shown %d, hidden by the world %d, NaN or limit world record %d, of those with an entity on the ray %d" % (
        what, o.shape[0], int(shown.sum()), int(info["occluded"].sum()), int(odd.sum()), int((odd & info["hit"]).sum())))
    assert shown.any() and info["occluded"].any() and (odd & info["hit"]).any()
    assert not limit or (world_want["kind"] == abi.RT_HIT_LIMIT).sum() >= 20
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)
    picks = ctx.pick_pixels(u, xy)
    pw_got, phits = ctx.pick_entities(u, xy, boxes, models)
    same_records(pw_got, picks, what + ": rt_pick_entities' world part against rt_pick_pixels")
    pwant = eq.pick(u, xy, W, H, picks, boxes, models, stamps)
    same_records(phits, pwant, what + ": rt_pick_entities")
    assert (phits["kind"] != abi.RT_ENTITY_NONE).any()


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[4], CASES[6]], ids=_id)
def test_entity_queries(case, stage):
    name, R, pose, (W, H) = case
    ctx, stamps, sid, u, before, mine = stage.frame(case)
    _entity_queries(ctx, stamps, sid, u, before, pw.world_of(name, R)[0], mine, W, H, R, _id(case), limit=name == "limit")


# ---- region 1024 --------------------------------------------------------------------------------------------------------------------------
TERRAIN_POSE = dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.2, sun=0.3)
WINDOWS_1024 = [((0, 0, 0), TERRAIN_POSE), ((64, -128, 64), dict(origin=(20.0, -200.0, 110.0), heading=1.2, pitch=-0.25, sun=0.5))]


@pytest.fixture(scope="module")
def region1024(blue_noise, native_built):
    """One context of region 1024 whose world the device generates; the window it holds is generated on demand."""
    R, (W, H) = 1024, SMALL
    ctx = render.Context(render.make_config(W, H, spp=1, depth=2, flags=CACHE, region=R))
    held = {}

    def window(lr):
        if held.get("lr") != lr:
            ctx.generate_world(world.DEFAULT_SEED, None if lr == (0, 0, 0) else tuple(c - R // 2 for c in lr))
            mine = np.empty((R, R, R), dtype=np.uint8)
            for z in range(0, R, 64):                     # in slabs: the material words that come along are 4 GiB in all
                mine[z:z + 64] = ctx.read_box((0, 0, z), (R, R, 64))[1]
            held.update(lr=lr, mine=mine)
        return held["mine"]

    try:
        ctx.upload_noise(blue_noise)
        mats, state = es.small_stamp()
        sid = ctx.stamp_create(mats, state)
        yield ctx, {sid: (mats, state)}, sid, window
    finally:
        ctx.destroy()


@pytest.mark.parametrize("lr,pose", WINDOWS_1024, ids=["lr0", "scrolled"])
def test_region_1024(lr, pose, region1024):
    """<10, true> and <10, false> of k_add_lights, k_add_lights_occluded, k_shadow_entities, k_entity_query and k_probe, once each,
    against their restatements on the terrain the device generates (the probes: against the frame's own lighting)."""
    R, (W, H) = 1024, SMALL
    ctx, stamps, sid, window = region1024
    mine = window(lr)
    u = po.camera_uniforms(pose["origin"], pose["heading"], pose["pitch"], pose["sun"], 7, lr)

    def fresh():
        ctx.draw_frame(u)
        ctx.sync()
        return _all(ctx)

    before = fresh()
    assert (before["normal_r8"] < 6).mean() > 0.3 and (before["normal_r8"] >= 6).any()
    lights = pw.scatter_lights(before, u, W, H, 16, 11, rmin=4.0, rmax=40.0)
    pairs = pw.light_pairs(before, u, lights, mine, W, H, R)
    print("region 1024 lr %s: pairs %s" % (lr, pairs))
    assert pairs["visible"] > 50 and pairs["blocked"] > 50
    ctx.add_lights(u, lights)
    _assert_same(_all(ctx), _with_final(pl.add_lights(_without_final(before), u, lights, mine, W, H, R), before), "rt_add_lights:")
    before = fresh()
    boxes, models = pw.occluders(before, u, W, H, lights, 12, 4, 11, sid)
    classes = {}
    want = _with_final(ls.add_lights_occluded(_without_final(before), u, lights, boxes, models, stamps, mine, W, H, R, classes=classes), before)
    assert classes["entity_only"] > 0 and classes["visible"] > 0 and classes["world_only"] > 0, classes
    ctx.add_lights_occluded(u, lights, boxes, models)
    _assert_same(_all(ctx), want, "rt_add_lights_occluded:")
    before = fresh()
    boxes, models = pw.sun_boxes(before, u, W, H, 12, 11), es.scatter_models(before, u, W, H, 4, 11, sid, pw.STAMP_EXTENT, scales=(1.0, 0.125))
    masks = es.masks(before, u, boxes, models, stamps, mine, W, H, R)
    print("region 1024 lr %s: pairs %s, sun pixels %s" % (lr, classes, {k: int(v.sum()) for k, v in masks.items()}))
    assert masks["changed"].any() and masks["world"].any()
    ctx.shadow_entities(u, boxes, models, 0.75)
    _assert_same(_all(ctx), _with_final(es.shadow_entities(_without_final(before), u, boxes, models, stamps, mine, W, H, R, 0.75, classes=masks), before),
                 "rt_shadow_entities:")
    before = fresh()
    _entity_queries(ctx, stamps, sid, u, before, None, mine, W, H, R, "region 1024 lr %s" % (lr,))
    xy, probes = _pixel_probes(ctx, u, W, H)
    got = ctx.probe_records(u, probes, 1, 2)
    assert bits(got["light"] / f32(16.0)).tolist() == bits(before["lighting_f32"][xy[:, 1], xy[:, 0], :3]).tolist()
    assert len(probes) >= 0.3 * W * H


# ---- rt_probe_light -------------------------------------------------------------------------------------------------------------------------
PROBE_CASES = [("arbitrary", 256, PLAIN, 2), ("arbitrary", 256, PLAIN, 5), ("arbitrary", 512, SCROLLED, 2), ("pyramid", 256, SCROLLED, 2)]


@pytest.mark.parametrize("name,R,pose,depth", PROBE_CASES, ids=["%s%d-pose%d-depth%d" % c for c in PROBE_CASES])
def test_probes_equal_the_lighting_of_frames(name, R, pose, depth, stage, blue_noise):
    """The probes of a frame's surface pixels with samples = spp = 4: light / 16 is the oracle's lighting there, bit for bit; every
    50th probe against tests/light_probe_ref.py (at region 512 through tests/ray_query_ref.py: the oracle's trace_ray is region 256
    only).  Depth 5 keeps the albedo stack in LDS, here with random material words."""
    (W, H), spp = SMALL, 4
    ctx, _, _ = stage.ctx(name, R, SMALL, spp, depth)
    mats, mine = pw.world_of(name, R)
    u = pw.uniforms(po, name, R, pose)
    ctx.draw_frame(u)
    ctx.sync()
    frame = ctx.readback_all()
    cpu = stage.oracle(name, R, pose, SMALL, spp, depth)
    _assert_same(frame, cpu, "the frame against the oracle's,")
    xy, probes = _pixel_probes(ctx, u, W, H)
    got = ctx.probe_records(u, probes, spp, depth)
    shallow = ctx.probe_records(u, probes, spp, 1)
    assert bits(got["light"] / f32(16.0)).tolist() == bits(cpu["lighting_f32"][xy[:, 1], xy[:, 0], :3]).tolist()
    deeper = np.any(bits(got["light"]) != bits(shallow["light"]), axis=-1)
    print("probes %s %d pose %d depth %d: %d of %d pixels, %d change past depth 1" % (name, R, pose, depth, len(probes), W * H, int(deeper.sum())))
    assert len(probes) >= 0.5 * W * H
    assert np.count_nonzero(deeper) >= 0.1 * len(probes)
    p = pw.poses(name, R)[int(pose)]
    lr = aw.pose_lr(p, R)
    trace = None if R == 256 else lp.restated_trace(mats, mine, lr, R)     # (the oracle's trace_ray is region 256 only)
    for i in range(0, len(probes), 50):
        light, sun = lp.probe_light(mats, mine, blue_noise, p["sun"], 7, lr, probes[i]["position"], int(probes[i]["normal"]),
                                    (int(probes[i]["cell"][0]), int(probes[i]["cell"][1])), spp, depth, trace=trace)
        nan = np.isnan(light)
        assert np.array_equal(nan, np.isnan(got[i]["light"])), (i, light, got[i])
        assert bits(got[i]["light"])[~nan].tolist() == bits(light)[~nan].tolist(), (i, light, got[i])
        assert int(got[i]["sun_samples"]) == sun, (i, sun, got[i])


def test_one_sample_probes_equal_the_frame_at_512_with_lr_zero(stage):
    """k_probe's <9, true> build, which no other probe test launches: the arbitrary world at 512, plain pose, samples = spp = 1."""
    case = CASES[3]
    W, H = case[3]
    ctx, stamps, sid, u, before, mine = stage.frame(case)
    xy, probes = _pixel_probes(ctx, u, W, H)
    got = ctx.probe_records(u, probes, 1, 2)
    assert bits(got["light"] / f32(16.0)).tolist() == bits(before["lighting_f32"][xy[:, 1], xy[:, 0], :3]).tolist()
    assert len(probes) >= 0.3 * W * H and got["light"].any()
