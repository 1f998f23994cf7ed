"""Point-light shadows of entities on the GPU (rt_add_lights_occluded, rt_add_lights_occluded_async).  Every comparison is bit for bit,
on all ten planes, with tests/light_shadow_ref.py — which has no cull and tests every occluder against every (pixel, light) pair that
passed the pair test — applied to the planes read back before the call and to the resident minefield: the batch edges of lights, boxes
and models and the two limits on frames with partial tiles, occluders put on purpose between a light and a surface it reaches, an
adversarial set for the kernel's one cull per tile (each case also alone), zero occluders against rt_add_lights, entity pixels, region
512, a scrolled window, the asynchronous call, every refusal, the absence of leaks into the next frame and the lighting history,
rt_stamp_destroy behind an enqueued call, the ordering against world edits, the host mirror and rt_bench.

The seeds of the scattered cases were picked on the CPU, with the restatement alone on the CPU oracle's frame (which the GPU's frame
equals bit for bit), so that all four classes occur; they are fixed."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from raytrace_amd import _lib, abi, render, world
from tests import entity_shadow_ref as shadow_ref
from tests import light_shadow_ref as ref
from tests import point_light_ref as pl
from tests import stamp_edits as se
from tests.draw_stamps_ref import batch as model_batch, model as one_model
from tests.pass_worlds import boxes_at, midpoints, models_at, occluders, scatter_lights  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CACHE, ACC, REP = abi.RT_FLAG_CACHE_PRIMARY, abi.RT_FLAG_ACCUMULATE, abi.RT_FLAG_REPROJECT
POSE = dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.2, sun=0.3)     # the point-light tests' pose
SHAPES = [(100, 60), (64, 40)]            # partial 8x8 tiles on both axes; whole tiles
STAMP_EXTENT = (3, 4, 5)
# (lights, boxes, models, shape) -> seed: the 64-record batch edges of each kind
CASES = {(1, 1, 0, 0): 100, (1, 63, 0, 0): 100, (1, 65, 0, 1): 105, (64, 1, 0, 1): 4, (64, 63, 0, 0): 5, (64, 65, 0, 0): 6, (65, 1, 0, 0): 7,
         (65, 63, 0, 1): 8, (65, 65, 0, 0): 9, (64, 0, 1, 0): 10, (65, 63, 1, 1): 11, (64, 0, 65, 0): 12, (65, 65, 65, 0): 13}
f32 = np.float32


def _u(seed=5, origin=None, pitch=None, lr=(0, 0, 0)):
    return po.camera_uniforms(origin or POSE["origin"], POSE["heading"], POSE["pitch"] if pitch is None else pitch, POSE["sun"], seed, lr)


def _ctx(scene, noise, W, H, **kw):
    kw.setdefault("flags", CACHE)
    ctx = render.Context(render.make_config(W, H, **kw))
    if scene is None:
        ctx.generate_world(world.DEFAULT_SEED)
    else:
        ctx.upload_world(*scene)
    ctx.upload_noise(noise)
    return ctx


def _all(ctx):
    """All ten planes."""
    return {abi.BUFFER_NAMES[b]: ctx.readback(b) for b in range(abi.RT_BUF_COUNT)}


def _mine(ctx, R=256):
    """The resident region's minefield as the device holds it, [z][y][x] texels."""
    return ctx.read_box((0, 0, 0), (R, R, R))[1]


def _assert_same(got, want, what=""):
    assert got.keys() == want.keys()
    for name in want:
        if got[name].tobytes() != want[name].tobytes():
            a, b = got[name].reshape(got[name].shape[0], got[name].shape[1], -1), want[name].reshape(want[name].shape[0], want[name].shape[1], -1)
            bad = np.argwhere((a.view(np.uint8) != b.view(np.uint8)).any(axis=-1))
            raise AssertionError("%s plane %s differs at %d pixels, first (row, col) %s" % (what, name, len(bad), bad[:5].tolist()))


def _differ(a, b):
    return any(a[k].tobytes() != b[k].tobytes() for k in a)


def _restated(before, u, lights, boxes, models, stamps, mine, W, H, R=256, classes=None):
    want = ref.add_lights_occluded({k: v for k, v in before.items() if k != "final_bgra8"}, u, lights, boxes, models, stamps, mine, W, H, R,
                                   classes=classes)
    want["final_bgra8"] = before["final_bgra8"]
    return want


def _unoccluded(before, u, lights, mine, W, H, R=256):
    want = pl.add_lights({k: v for k, v in before.items() if k != "final_bgra8"}, u, lights, mine, W, H, R)
    want["final_bgra8"] = before["final_bgra8"]
    return want


def _changed(a, b):
    return (a["lighting_f32"] != b["lighting_f32"]).any(axis=-1)


def _dev(records):
    return torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(len(records), -1).copy()).cuda()


def _code(fn, *a, **kw):
    with pytest.raises(render.RtError) as e:
        fn(*a, **kw)
    return e.value.code


def _fresh_frame(ctx, u):
    ctx.draw_frame(u)
    ctx.sync()
    return _all(ctx)


def _small_stamp(ctx):
    """The tests' small sparse stamp (ABSENT, AIR and SOLID cells) on `ctx`: ({id: (materials, state)}, id)."""
    mats, state = shadow_ref.small_stamp()
    sid = ctx.stamp_create(mats, state)
    return {sid: (mats, state)}, sid


def _nontrivial(classes, before, what=""):
    """The comparison does not pass on a trivial input: pairs only an entity blocks, pairs only the world blocks, visible pairs, sky."""
    for name in ("entity_only", "world_only", "visible"):
        assert classes[name] > 0, "%s: no pair of class '%s' (%s)" % (what, name, classes)
    assert (before["normal_r8"] >= 6).any(), "no sky"


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------------
# (scatter_lights, midpoints, boxes_at, models_at and occluders live in tests/pass_worlds.py, which tests without a GPU import too)


def case_inputs(before, u, W, H, case, seed, sid):
    """(lights, boxes, models) of a batch case; a single light is a wide one, so that it reaches more than a handful of pixels."""
    nl, nb, nm, _ = case
    lights = scatter_lights(before, u, W, H, nl, seed, rmin=10.0 if nl == 1 else 2.0)
    return (lights,) + occluders(before, u, W, H, lights, nb, nm, seed, sid)


@pytest.fixture(scope="module")
def frame_ctx(procedural_region, blue_noise):
    """One context per frame shape (spp 1, depth 2 on the small terrain fixture) with the small stamp, shared by the tests that only
    need a frame to light."""
    made = {}
    for shape in SHAPES:
        ctx = _ctx(procedural_region, blue_noise, *shape, spp=1, depth=2)
        made[shape] = (ctx,) + _small_stamp(ctx)
    yield made
    for ctx, _, _ in made.values():
        ctx.destroy()


@pytest.fixture(scope="module")
def region_mine(procedural_region):
    return procedural_region[1]


# ---- batch edges and limits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES), ids=["%dl%db%dm-%d" % c for c in sorted(CASES)])
def test_batches_equal_the_restatement(case, frame_ctx, region_mine):
    nl, nb, nm, si = case
    W, H = SHAPES[si]
    (ctx, stamps, sid), u = frame_ctx[SHAPES[si]], _u()
    before = _fresh_frame(ctx, u)
    lights, boxes, models = case_inputs(before, u, W, H, case, CASES[case], sid)
    classes = {}
    want = _restated(before, u, lights, boxes, models, stamps, region_mine, W, H, classes=classes)
    _nontrivial(classes, before, str(case))
    ctx.add_lights_occluded(u, lights, boxes, models)
    got = _all(ctx)
    _assert_same(got, want, "%d lights, %d boxes, %d models" % case[:3])
    assert _differ(want, before)


def test_one_light_with_4096_boxes(frame_ctx, region_mine):
    W, H = SHAPES[0]
    (ctx, stamps, sid), u = frame_ctx[SHAPES[0]], _u()
    before = _fresh_frame(ctx, u)
    lights = scatter_lights(before, u, W, H, 1, 2, rmin=10.0, rmax=12.0)
    rng = np.random.default_rng(21)
    boxes = np.concatenate([boxes_at(midpoints(before, u, W, H, lights, 16, rng), rng, half=(0.05, 0.2)),
                            shadow_ref.scatter_boxes(before, u, W, H, 4080, 21, lift=(0.2, 3.0))])     # a few on purpose, the rest over all the frame
    classes = {}
    want = _restated(before, u, lights, boxes, None, stamps, region_mine, W, H, classes=classes)
    assert classes["entity_only"] > 0 and classes["visible"] > 0
    ctx.add_lights_occluded(u, lights, boxes)
    _assert_same(_all(ctx), want, "1 light, 4096 boxes")


def test_1024_lights_with_one_box(frame_ctx, region_mine):
    W, H = SHAPES[1]
    (ctx, stamps, sid), u = frame_ctx[SHAPES[1]], _u()
    before = _fresh_frame(ctx, u)
    lights = scatter_lights(before, u, W, H, 1024, 22, rmin=1.0, rmax=5.0)
    rng = np.random.default_rng(22)
    boxes = boxes_at(midpoints(before, u, W, H, lights, 1, rng), rng, half=(0.5, 1.0))       # one mob-sized box among the lights
    classes = {}
    want = _restated(before, u, lights, boxes, None, stamps, region_mine, W, H, classes=classes)
    _nontrivial(classes, before, "1024 lights")
    ctx.add_lights_occluded(u, lights, boxes)
    _assert_same(_all(ctx), want, "1024 lights, 1 box")


def test_a_near_camera_fills_its_tiles(frame_ctx, region_mine):
    """The pose above sees the terrain from some 150 units: a light reaches a few pixels of a tile.  From 8 to 20 units every lane of
    a tile has pairs, every tile lists occluders and the walks run in full waves: tens of thousands of pairs an entity blocks."""
    W, H = SHAPES[0]
    (ctx, stamps, sid), u = frame_ctx[SHAPES[0]], _u()
    far = _fresh_frame(ctx, u)
    surface, P, axis, even = pl.surface_points(far, u, W, H)
    ys, xs = np.nonzero(surface & (axis == 2) & even)
    k = np.argsort(far["depth_f32"][ys, xs], kind="stable")[len(ys) // 10]                # a near pixel that faces up
    d = np.array(u.forward[:], dtype=np.float64)
    d[2] = 0.0
    o = P[ys[k], xs[k]].astype(np.float64) - 8.0 * d / np.linalg.norm(d) + np.array([0.0, 0.0, 6.0])
    near = _u(origin=tuple(float(v) for v in o), pitch=-0.6)
    before = _fresh_frame(ctx, near)
    assert (before["depth_f32"][before["normal_r8"] < 6] < 32.0 * 40.0).all()
    lights = scatter_lights(before, near, W, H, 24, 61, rmin=3.0, rmax=8.0)
    boxes, models = occluders(before, near, W, H, lights, 80, 30, 61, sid)
    classes = {}
    want = _restated(before, near, lights, boxes, models, stamps, region_mine, W, H, classes=classes)
    assert classes["entity_only"] > 5000 and classes["world_only"] > 100 and classes["visible"] > 1000
    ctx.add_lights_occluded(near, lights, boxes, models)
    _assert_same(_all(ctx), want, "a near camera")


# ---- the adversarial set for the cull -----------------------------------------------------------------------------------------------------
def _ulps(x, n):
    x = f32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, f32(np.inf) if n > 0 else f32(-np.inf))
    return x


def adversarial(before, u, W, H, mine, ctx):
    """([(name, lights, boxes or None, models or None)], stamps, ids): one light per case unless said otherwise."""
    surface, P, axis, even = pl.surface_points(before, u, W, H)
    ys, xs = np.nonzero(surface & (axis == 2) & even)                     # pixels that face up
    order = np.argsort(before["depth_f32"][ys, xs], kind="stable")
    pick = lambda k: (ys[order[(k * 97) % (len(order) // 2)]], xs[order[(k * 97) % (len(order) // 2)]])   # among the nearer half
    rows = []

    def box(lo, hi):
        b = np.zeros(1, dtype=render.DRAW_BOX_DTYPE)
        b["lo"][0], b["hi"][0], b["material"], b["emission"] = np.asarray(lo, dtype=f32), np.asarray(hi, dtype=f32), 0x1FFFFF, 0xFF000000
        return b

    # a light three units over a pixel; slabs whose near or far face lies a few ulp before and behind the light on each axis
    y, x = pick(1)
    p = P[y, x].astype(np.float64)
    L = render.make_point_lights([p + np.array([0.4, -0.3, 3.0])], 9.0, (30.0, 20.0, 10.0))
    pos = L["position"][0].astype(f32)
    for k in range(3):
        for n in (-3, -1, 0, 1, 3):
            lo, hi = pos.astype(np.float64) - 6.0, pos.astype(np.float64) + 6.0
            beyond_lo, beyond_hi = lo.copy(), hi.copy()
            beyond_lo[k] = _ulps(pos[k], n)                               # the slab starts at the light (+- n ulp) and lies beyond it
            before_lo, before_hi = lo.copy(), hi.copy()
            before_hi[k] = _ulps(pos[k], n)                               # the slab ends at the light (+- n ulp) and lies before it
            rows.append(("axis %d: a slab from the light %+d ulp on" % (k, n), L, box(beyond_lo, beyond_hi), None))
            rows.append(("axis %d: a slab up to the light %+d ulp" % (k, n), L, box(before_lo, before_hi), None))
    # boxes that touch the hull of one tile's P' bounds and the light exactly, at both corners
    ty, tx = (y // 8) * 8, (x // 8) * 8
    tile = P[ty:ty + 8, tx:tx + 8][surface[ty:ty + 8, tx:tx + 8]]
    hlo, hhi = np.minimum(tile.min(axis=0), pos), np.maximum(tile.max(axis=0), pos)
    rows.append(("a box whose low corner is the hull's high corner", L, box(hhi, hhi.astype(np.float64) + 1.0), None))
    rows.append(("a box whose high corner is the hull's low corner", L, box(hlo.astype(np.float64) - 1.0, hlo), None))
    rows.append(("a box one ulp inside the hull's high corner", L, box([_ulps(v, -1) for v in hhi], hhi.astype(np.float64) + 1.0), None))
    # a segment with two zero direction components: the light straight over the pixel, boxes over it and with a face ON its line
    y, x = pick(2)
    p = P[y, x]
    Lz = render.make_point_lights([(p[0], p[1], p[2] + f32(3.0))], 9.0, (30.0, 20.0, 10.0))
    rows.append(("d = (0, 0, 1): a box over the pixel", Lz, box((p[0] - 0.5, p[1] - 0.5, p[2] + 1.0), (p[0] + 0.5, p[1] + 0.5, p[2] + 2.0)), None))
    rows.append(("d = (0, 0, 1): lo_x == o_x", Lz, box((p[0], p[1] - 0.5, p[2] + 1.0), (p[0] + 0.5, p[1] + 0.5, p[2] + 2.0)), None))
    rows.append(("d = (0, 0, 1): hi_y == o_y", Lz, box((p[0] - 0.5, p[1] - 0.5, p[2] + 1.0), (p[0] + 0.5, p[1], p[2] + 2.0)), None))
    # a light inside a box; a box that encloses a whole tile, its light outside; a box round every surface and the light
    y, x = pick(3)
    p = P[y, x].astype(np.float64)
    Li = render.make_point_lights([p + np.array([0.0, 0.0, 2.0])], 9.0, (30.0, 20.0, 10.0))
    c = Li["position"][0].astype(np.float64)
    rows.append(("a light inside a box", Li, box(c - 0.5, c + 0.5), None))
    ty, tx = (y // 8) * 8, (x // 8) * 8
    tile = P[ty:ty + 8, tx:tx + 8][surface[ty:ty + 8, tx:tx + 8]].astype(np.float64)
    rows.append(("a box enclosing a whole tile", Li, box(tile.min(axis=0) - 0.25, tile.max(axis=0) + 0.25), None))
    pts = P[surface].astype(np.float64)
    rows.append(("a box enclosing every surface and the light", Li, box(np.minimum(pts.min(axis=0), c) - 1.0, np.maximum(pts.max(axis=0), c) + 1.0), None))
    rows.append(("coordinates at 2^22", Li, box((4194302.0, -4194304.0, 4194303.0), (4194304.0, -4194302.0, 4194304.0)), None))
    # models: the light inside a solid cell; the light inside an AIR cell whose far neighbours are solid
    solid = (np.full((2, 2, 2), 7, dtype=np.uint32), np.full((2, 2, 2), se.SOLID, dtype=np.uint8))
    state = np.full((3, 3, 3), se.SOLID, dtype=np.uint8)
    state[1, 1, 1] = se.AIR
    state[0, 1, 1] = se.ABSENT                                            # ... and an opening below the light's cell
    hollow = (np.where(state == se.SOLID, 9, 0).astype(np.uint32), state)
    ids = [ctx.stamp_create(*solid), ctx.stamp_create(*hollow)]
    stamps = {ids[0]: solid, ids[1]: hollow}
    rows.append(("a light inside a solid model cell", Li, None, model_batch([one_model(ids[0], (c - 0.75).astype(f32), 1.0, 0)])))
    rows.append(("a light inside a model's AIR cell over an opening", Li, None, model_batch([one_model(ids[1], (c - 0.75).astype(f32), 0.5, 0)])))
    return rows, stamps, ids


def test_adversarial_set_equals_the_restatement(frame_ctx, region_mine):
    W, H = SHAPES[0]
    (ctx, _, _), u = frame_ctx[SHAPES[0]], _u()
    before = _fresh_frame(ctx, u)
    rows, stamps, ids = adversarial(before, u, W, H, region_mine, ctx)
    blocked, every = {}, {}
    for name, lights, boxes, models in rows:                              # each occluder alone: a wrong cull cannot hide behind another
        before = _fresh_frame(ctx, u)
        classes = {}
        want = _restated(before, u, lights, boxes, models, stamps, region_mine, W, H, classes=classes)
        ctx.add_lights_occluded(u, lights, boxes, models)
        _assert_same(_all(ctx), want, name)
        blocked[name] = classes["entity_only"] + classes["both"]                          # the pairs an entity blocks
        every[name] = blocked[name] + classes["world_only"] + classes["visible"]          # the pairs that passed the pair test
    # the hand answers the set was built for
    for k in range(3):
        for n in (-3, -1, 0, 1, 3):
            assert blocked["axis %d: a slab up to the light %+d ulp" % (k, n)] > 0        # the light's side of the slab shades the other
    assert blocked["axis 2: a slab from the light +1 ulp on"] == 0 and blocked["axis 2: a slab from the light +3 ulp on"] == 0
    assert blocked["axis 2: a slab from the light -3 ulp on"] == every["axis 2: a slab from the light -3 ulp on"] > 0      # the light is inside
    assert blocked["a light inside a box"] == every["a light inside a box"] > 0
    assert blocked["a light inside a solid model cell"] == every["a light inside a solid model cell"] > 0
    assert 0 < blocked["a light inside a model's AIR cell over an opening"] < every["a light inside a model's AIR cell over an opening"]
    assert blocked["a box enclosing a whole tile"] > 0 and blocked["coordinates at 2^22"] == 0
    assert blocked["a box enclosing every surface and the light"] == every["a box enclosing every surface and the light"]
    assert blocked["d = (0, 0, 1): a box over the pixel"] > 0
    for name in ("a box whose low corner is the hull's high corner", "a box whose high corner is the hull's low corner"):
        assert blocked[name] == 0 and every[name] > 0
    # ... and all of them in one call, every light and every occluder together
    before = _fresh_frame(ctx, u)
    seen, lights = set(), []
    for r in rows:
        if r[1].tobytes() not in seen:
            seen.add(r[1].tobytes())
            lights.append(r[1])
    lights = np.concatenate(lights)
    boxes = np.concatenate([r[2] for r in rows if r[2] is not None])
    models = np.concatenate([r[3] for r in rows if r[3] is not None])
    ctx.add_lights_occluded(u, lights, boxes[:-2], models)                # (without the two boxes round everything)
    _assert_same(_all(ctx), _restated(before, u, lights, boxes[:-2], models, stamps, region_mine, W, H), "the adversarial set in one call")
    for s in ids:
        ctx.stamp_destroy(s)


def test_more_candidates_on_a_tile_than_the_list_holds(frame_ctx, region_mine):
    """100 boxes and 70 models round one light: every tile the light reaches lists more than 64 of a kind and scans every record."""
    W, H = SHAPES[0]
    (ctx, stamps, sid), u = frame_ctx[SHAPES[0]], _u()
    before = _fresh_frame(ctx, u)
    lights = scatter_lights(before, u, W, H, 3, 31, rmin=8.0, rmax=12.0)
    rng = np.random.default_rng(31)
    for nb, nm in ((100, 0), (10, 70), (100, 70), (64, 64), (65, 64)):
        before = _fresh_frame(ctx, u)
        boxes = boxes_at(midpoints(before, u, W, H, lights[:1], nb, rng), rng, half=(0.02, 0.1))
        models = models_at(midpoints(before, u, W, H, lights[:1], nm, rng), sid, 31, scales=(0.0625, 0.03125)) if nm else None
        # every one of them lies inside the hull of every tile the first light reaches together with its light: all are candidates there
        classes = {}
        want = _restated(before, u, lights, boxes, models, stamps, region_mine, W, H, classes=classes)
        assert classes["entity_only"] > 0 and classes["visible"] > 0
        ctx.add_lights_occluded(u, lights, boxes, models)
        _assert_same(_all(ctx), want, "%d boxes and %d models round one light" % (nb, nm))


# ---- zero occluders -------------------------------------------------------------------------------------------------------------------------
def test_zero_occluders_is_add_lights(frame_ctx, region_mine):
    W, H = SHAPES[0]
    (ctx, stamps, sid), u = frame_ctx[SHAPES[0]], _u()
    before = _fresh_frame(ctx, u)
    lights = scatter_lights(before, u, W, H, 65, 41)
    ctx.add_lights(u, lights)
    want = _all(ctx)
    assert _differ(want, before)
    for boxes, models in ((None, None), (np.zeros(0, dtype=render.DRAW_BOX_DTYPE), np.zeros(0, dtype=render.DRAW_STAMP_DTYPE))):
        _assert_same(_fresh_frame(ctx, u), before)
        ctx.add_lights_occluded(u, lights, boxes, models)
        _assert_same(_all(ctx), want, "no occluders")
    _assert_same(_fresh_frame(ctx, u), before)
    ctx.add_lights_occluded_async(u, _dev(lights))
    _assert_same(_all(ctx), want, "no occluders, async")
    # no lights: nothing is enqueued, whatever the occluders
    before = _fresh_frame(ctx, u)
    boxes, models = occluders(before, u, W, H, lights, 8, 4, 41, sid)
    ctx.add_lights_occluded(u, None, boxes, models)
    _assert_same(_all(ctx), before, "no lights")


# ---- entity pixels ------------------------------------------------------------------------------------------------------------------------
def test_entity_pixels_are_lit_and_shadowed_through_their_own_depth_and_face(frame_ctx, region_mine):
    """A box and a model drawn into the frame and then handed to the call as occluders, a light beside them: their faces turned to
    the light are lit (the segment leaves the entity), those turned away fail the pair test, and each shades the other and the ground."""
    from tests.test_gpu_draw_boxes import some_lights
    W, H = SHAPES[0]
    (ctx, stamps, sid), u = frame_ctx[SHAPES[0]], _u()
    bare = _fresh_frame(ctx, u)
    surface, P, axis, even = pl.surface_points(bare, u, W, H)
    ys, xs = np.nonzero(surface & (axis == 2) & even)
    k = np.argsort(bare["depth_f32"][ys, xs], kind="stable")[len(ys) // 10]               # a near pixel that faces up
    half = 0.05 * float(bare["depth_f32"][ys[k], xs[k]]) / 32.0                           # (the terrain is some 150 units away)
    g = P[ys[k], xs[k]].astype(np.float64)
    c = g + np.array([0.0, 0.0, half + 0.5])
    boxes = render.make_draw_boxes([c - half], [c + half], 0x1FFFFF, 0xFF000000)
    scale = 2.0 * half / 5.0
    models = model_batch([one_model(sid, (g + np.array([3.0 * half, 0.0, 0.25])).astype(f32), scale, 0)])
    ctx.draw_boxes(u, boxes, some_lights(1))
    ctx.draw_stamps(u, models, some_lights(1, seed=4))
    before = _all(ctx)
    entity = before["depth_f32"] != bare["depth_f32"]
    assert entity.sum() > 40
    lights = render.make_point_lights([c + np.array([1.5 * half, -2.5 * half, 1.5 * half]), c + np.array([-3.0 * half, 0.0, 2.0 * half])], 12.0 * half + 6.0,
                                      [(30.0, 20.0, 10.0), (5.0, 25.0, 30.0)])
    classes = {}
    want = _restated(before, u, lights, boxes, models, stamps, region_mine, W, H, classes=classes)
    assert classes["entity_only"] > 20 and classes["visible"] > 20
    ctx.add_lights_occluded(u, lights, boxes, models)
    got = _all(ctx)
    _assert_same(got, want, "entities as their own occluders")
    lit = _changed(got, before)
    assert lit[entity].any() and (~lit)[entity].any()                    # faces turned to a light, faces turned from both
    plain = _unoccluded(before, u, lights, region_mine, W, H)
    shadowed = _changed(plain, got)
    assert shadowed[~entity].sum() > 10                                   # the ground in the entities' shadows
    assert shadowed[entity].any()                                         # one entity shades the other (or a concave model itself)


# ---- regions and windows ----------------------------------------------------------------------------------------------------------------
def test_region_512(blue_noise):
    W, H = 64, 40
    u = _u()
    with _ctx(None, blue_noise, W, H, spp=1, depth=2, region=512) as big:          # the region generated on the device
        stamps, sid = _small_stamp(big)
        before = _fresh_frame(big, u)
        lights = scatter_lights(before, u, W, H, 40, 43)
        boxes, models = occluders(before, u, W, H, lights, 60, 20, 43, sid)
        mine = _mine(big, 512)
        classes = {}
        want = _restated(before, u, lights, boxes, models, stamps, mine, W, H, 512, classes=classes)
        assert classes["entity_only"] > 0 and classes["visible"] > 0
        big.add_lights_occluded(u, lights, boxes, models)
        _assert_same(_all(big), want, "region 512")


def test_a_scrolled_window_after_a_streamed_slab(procedural_region, blue_noise):
    """lr != 0: the kernel's other template.  The slab that entered at the window's far side is in the minefield the shadow rays read."""
    W, H = 100, 60
    lr = (16, 0, 0)
    u = _u(origin=(-14.0, -128.0, 100.0), lr=lr)
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        stamps, sid = _small_stamp(ctx)
        ctx.generate_slice(world.DEFAULT_SEED, 0, (128, -128, -128))                # world x 128..143 into texels 0..15
        before = _fresh_frame(ctx, u)
        mine = _mine(ctx)
        assert mine.tobytes() != procedural_region[1].tobytes()
        lights = scatter_lights(before, u, W, H, 48, 47)
        boxes, models = occluders(before, u, W, H, lights, 70, 20, 47, sid)
        classes = {}
        want = _restated(before, u, lights, boxes, models, stamps, mine, W, H, classes=classes)
        assert classes["entity_only"] > 0 and classes["visible"] > 0
        ctx.add_lights_occluded(u, lights, boxes, models)
        got = _all(ctx)
        _assert_same(got, want, "lr %s" % (lr,))
        assert _differ(got, before)


# ---- async ------------------------------------------------------------------------------------------------------------------------------
def test_async_equals_sync_and_skips_invalid_lights_and_boxes(frame_ctx, region_mine):
    W, H = SHAPES[0]
    (ctx, stamps, sid), u = frame_ctx[SHAPES[0]], _u()
    before = _fresh_frame(ctx, u)
    lights = scatter_lights(before, u, W, H, 65, 53)
    boxes, models = occluders(before, u, W, H, lights, 96, 30, 53, sid)
    bad_b = boxes.copy()
    bad_b["lo"][5][0] = np.nan
    bad_b["hi"][16][1] = bad_b["lo"][16][1]
    bad_b["hi"][27][2] = np.inf
    bad_b["lo"][38][0] = -4194305.0
    bad_b["lo"][49], bad_b["hi"][49] = boxes["hi"][49], boxes["lo"][49]
    bad_l = lights.copy()
    bad_l["radius"][3], bad_l["color"][17][1], bad_l["reserved"][30], bad_l["position"][44][0], bad_l["radius"][64] = np.nan, -1.0, 1, np.inf, 1025.0
    skipped_b, skipped_l = ~shadow_ref.boxes_ref.valid(bad_b), ~pl.valid(bad_l)
    assert np.count_nonzero(skipped_b) == 5 and np.count_nonzero(skipped_l) == 5
    ctx.add_lights_occluded_async(u, _dev(bad_l), _dev(bad_b), models)
    got_bad = _all(ctx)
    _assert_same(got_bad, _restated(before, u, bad_l, bad_b, models, stamps, region_mine, W, H), "async, invalid records")
    _assert_same(got_bad, _restated(before, u, lights[~skipped_l], boxes[~skipped_b], models, stamps, region_mine, W, H), "async, the valid records alone")
    assert _code(ctx.add_lights_occluded, u, bad_l, boxes, models) == abi.RT_ERR_INVALID_ARG
    assert _code(ctx.add_lights_occluded, u, lights, bad_b, models) == abi.RT_ERR_INVALID_ARG
    _assert_same(_all(ctx), got_bad, "after the refused calls")
    _assert_same(_fresh_frame(ctx, u), before)
    ctx.add_lights_occluded(u, lights[~skipped_l], boxes[~skipped_b], models)
    _assert_same(_all(ctx), got_bad, "sync without the invalid records")
    # ... boxes alone, models alone, and on a caller's stream
    for b, m in ((boxes, None), (None, models)):
        before3 = _fresh_frame(ctx, u)
        ctx.add_lights_occluded_async(u, _dev(lights), None if b is None else _dev(b), m)
        _assert_same(_all(ctx), _restated(before3, u, lights, b, m, stamps, region_mine, W, H), "async, one kind")
    s = torch.cuda.Stream()
    dl, db = _dev(lights), _dev(boxes)
    torch.cuda.synchronize()
    ctx.set_stream(s.cuda_stream)
    try:
        ctx.draw_frame(u)
        ctx.add_lights_occluded_async(u, dl, db, models)
        s.synchronize()
        _assert_same(_all(ctx), _restated(before, u, lights, boxes, models, stamps, region_mine, W, H), "on a caller's stream")
    finally:
        ctx.set_stream(0)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(procedural_region, blue_noise):
    W, H = 64, 40
    lib = _lib.amd()
    u = _u()
    some_l = render.make_point_lights([(-30.0, -100.0, 92.0)] * 4, 6.0, (1.0, 1.0, 1.0))
    some_b = render.make_draw_boxes([(-30.0, -100.0, 90.0)] * 8, [(-29.0, -99.0, 91.0)] * 8, 1, 0xFF000000)
    with render.Context(render.make_config(W, H, spp=1, depth=2, flags=CACHE)) as empty:
        empty.upload_noise(blue_noise)
        assert _code(empty.add_lights_occluded, u, some_l, some_b) == abi.RT_ERR_NOT_READY        # no frame, no world
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        h = ctx.handle
        stamps, sid = _small_stamp(ctx)
        assert _code(ctx.add_lights_occluded, u, some_l, some_b) == abi.RT_ERR_NOT_READY          # no frame yet
        assert _code(ctx.add_lights_occluded_async, u, _dev(some_l), _dev(some_b)) == abi.RT_ERR_NOT_READY
        before = _fresh_frame(ctx, u)
        lights = scatter_lights(before, u, W, H, 4, 3)
        boxes, models = occluders(before, u, W, H, lights, 8, 4, 3, sid)
        pl_, pb, pm = lights.ctypes.data_as(C.c_void_p), boxes.ctypes.data_as(C.c_void_p), models.ctypes.data_as(C.c_void_p)
        d_lights, d_boxes = _dev(lights), _dev(boxes)
        dl, db = C.c_void_p(d_lights.data_ptr()), C.c_void_p(d_boxes.data_ptr())
        many_l = np.concatenate([lights] * 257)[:1025].copy()
        many_b = np.concatenate([boxes] * 513)[:4097].copy()
        many_m = np.concatenate([models] * 1025)[:4097].copy()
        d_many_l, d_many_b = _dev(many_l), _dev(many_b)
        assert lib.rt_add_lights_occluded(h, C.byref(u), many_l.ctypes.data_as(C.c_void_p), 1025, pb, 8, pm, 4) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_add_lights_occluded_async(h, C.byref(u), C.c_void_p(d_many_l.data_ptr()), 1025, db, 8, pm, 4) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_add_lights_occluded(h, C.byref(u), pl_, 4, many_b.ctypes.data_as(C.c_void_p), 4097, None, 0) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_add_lights_occluded_async(h, C.byref(u), dl, 4, C.c_void_p(d_many_b.data_ptr()), 4097, None, 0) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_add_lights_occluded(h, C.byref(u), pl_, 4, None, 0, many_m.ctypes.data_as(C.c_void_p), 4097) == abi.RT_ERR_INVALID_ARG
        for call, l, b in ((lib.rt_add_lights_occluded, pl_, pb), (lib.rt_add_lights_occluded_async, dl, db)):
            assert call(h, None, l, 4, b, 8, pm, 4) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), None, 4, b, 8, pm, 4) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), l, 4, None, 8, pm, 4) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), l, 4, b, 8, None, 4) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), None, 0, None, 8, None, 0) == abi.RT_ERR_INVALID_ARG      # a NULL array is refused with no light too
            assert call(h, C.byref(u), None, 0, b, 8, pm, 4) == abi.RT_OK                        # no lights: nothing to do
            assert call(h, C.byref(u), None, 0, None, 0, None, 0) == abi.RT_OK
        # host memory and unaligned device memory are not what the asynchronous call takes
        assert lib.rt_add_lights_occluded_async(h, C.byref(u), pl_, 4, db, 8, None, 0) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_add_lights_occluded_async(h, C.byref(u), dl, 4, pb, 8, None, 0) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_add_lights_occluded_async(h, C.byref(u), dl, 4, C.c_void_p(d_boxes.data_ptr() + 4), 7, None, 0) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_add_lights_occluded_async(h, C.byref(u), C.c_void_p(d_lights.data_ptr() + 4), 3, db, 8, None, 0) == abi.RT_ERR_INVALID_ARG
        for field, k, value in (("lo", 1, np.nan), ("lo", 0, 4194305.0), ("hi", 2, np.inf), ("hi", 0, -1.0e6)):
            bad = boxes.copy()
            bad[field][5][k] = value
            assert _code(ctx.add_lights_occluded, u, lights, bad, models) == abi.RT_ERR_INVALID_ARG, (field, value)
        for field, value in (("radius", 0.0), ("radius", np.nan), ("reserved", 1)):
            bad = lights.copy()
            bad[field][2] = value
            assert _code(ctx.add_lights_occluded, u, bad, boxes, models) == abi.RT_ERR_INVALID_ARG, (field, value)
        for field, value in (("stamp", 999), ("orient", 48), ("scale", 0.001), ("scale", 65.0), ("reserved", 1), ("scale", np.nan)):
            bad = models.copy()
            bad[field][2] = value
            assert _code(ctx.add_lights_occluded, u, lights, boxes, bad) == abi.RT_ERR_INVALID_ARG, (field, value)
            assert _code(ctx.add_lights_occluded_async, u, d_lights, d_boxes, bad) == abi.RT_ERR_INVALID_ARG, (field, value)
        _assert_same(_all(ctx), before, "after the rejected calls")
        ctx.add_lights_occluded(u, lights, boxes, models)                                       # and the context still works
        _assert_same(_all(ctx), _restated(before, u, lights, boxes, models, stamps, procedural_region[1], W, H))
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2, tile_rank=0, tile_world=2) as tiles:
        tiles.draw_frame(u)
        tiles.sync()
        assert _code(tiles.add_lights_occluded, u, some_l, some_b) == abi.RT_ERR_UNIMPLEMENTED
        d_l, d_b = _dev(some_l), _dev(some_b)
        assert lib.rt_add_lights_occluded_async(tiles.handle, C.byref(u), C.c_void_p(d_l.data_ptr()), 4, C.c_void_p(d_b.data_ptr()), 8, None,
                                                0) == abi.RT_ERR_UNIMPLEMENTED
    with render.Context(render.make_config(W, H, spp=1, depth=2, flags=CACHE)) as no_world:
        no_world.upload_noise(blue_noise)
        assert _code(no_world.add_lights_occluded, u, some_l, some_b) == abi.RT_ERR_NOT_READY


def test_no_lights_drop_no_prepass_and_a_call_does(procedural_region, blue_noise):
    """RT_FLAG_TIMING_ALL counts a frame's launches: a frame that reuses its slot's prepass has one fewer."""
    W, H = 136, 72
    u = _u()
    with _ctx(procedural_region, blue_noise, W, H, spp=4, depth=2, kernel=abi.RT_KERNEL_PATHS, flags=CACHE | abi.RT_FLAG_TIMING_ALL) as ctx:
        stamps, sid = _small_stamp(ctx)

        def frame_launches():
            ctx.draw_frame(u)
            ctx.sync()
            return int(ctx.timing().other_launches)

        frame_launches()                                                 # (the first frame also builds the tables)
        ctx.denoise(True)                                                # writes the lighting plane: the next frame runs its prepass
        ctx.sync()
        ctx.timing()
        fresh, again = frame_launches(), frame_launches()
        assert again < fresh                                             # the second frame reused the slot's prepass
        before = _all(ctx)
        lights = scatter_lights(before, u, W, H, 8, 13)
        boxes, models = occluders(before, u, W, H, lights, 24, 8, 13, sid)
        ctx.add_lights_occluded(u, lights[:0], boxes, models)
        ctx.sync()
        assert int(ctx.timing().other_launches) == 0                     # nothing enqueued
        assert frame_launches() == again                                 # ... and the prepass is still the slot's
        ctx.add_lights_occluded(u, lights, boxes, models)
        ctx.sync()
        assert int(ctx.timing().other_launches) == 1                     # one launch for lights, boxes and models together
        assert frame_launches() == fresh                                 # the call dropped the prepass


# ---- no leak into the next frame ------------------------------------------------------------------------------------------------------
def test_the_light_does_not_leak_into_the_next_frame(procedural_region, blue_noise):
    """A still camera.  The persistent route with cached primaries skips the prepass of a frame whose camera and world are unchanged:
    a slot whose lighting the call wrote must not be taken for one that still holds its prepass."""
    W, H = 136, 72
    u = _u()
    kw = dict(spp=4, depth=2, kernel=abi.RT_KERNEL_PATHS, flags=CACHE)
    with _ctx(procedural_region, blue_noise, W, H, **kw) as clean:
        for _ in range(2):
            clean.draw_frame(u)
        clean.sync()
        want = _all(clean)
    with _ctx(procedural_region, blue_noise, W, H, **kw) as ctx:
        stamps, sid = _small_stamp(ctx)
        before = _fresh_frame(ctx, u)
        lights = scatter_lights(before, u, W, H, 24, 13)
        boxes, models = occluders(before, u, W, H, lights, 40, 12, 13, sid)
        ctx.add_lights_occluded(u, lights, boxes, models)
        after = _all(ctx)
        assert np.count_nonzero(_changed(after, before)) > 20
        _assert_same(after, _restated(before, u, lights, boxes, models, stamps, procedural_region[1], W, H), "the lit frame")
        _assert_same(_fresh_frame(ctx, u), want, "the frame after the lights")


def test_history_of_a_reprojecting_context_is_untouched(procedural_region, blue_noise):
    W, H = 96, 64
    kw = dict(spp=1, depth=2, flags=ACC | REP | CACHE)
    cams = [_u(seed=10 + k, origin=(-30.0 + 0.25 * min(k, 2), -128.0, 100.0 - 0.1 * min(k, 2))) for k in range(5)]   # moves, then holds still
    with _ctx(procedural_region, blue_noise, W, H, **kw) as clean, _ctx(procedural_region, blue_noise, W, H, **kw) as ctx:
        stamps, sid = _small_stamp(ctx)
        for k, u in enumerate(cams):
            want = _fresh_frame(clean, u)
            before = _fresh_frame(ctx, u)
            _assert_same(before, want, "frame %d before its lights" % k)
            if k < 3:                                               # the next two frames follow the last call
                lights = scatter_lights(before, u, W, H, 16, 17 + k)
                boxes, models = occluders(before, u, W, H, lights, 30, 10, 17 + k, sid)
                ctx.add_lights_occluded(u, lights, boxes, models)
                after = _all(ctx)
                assert np.count_nonzero(_changed(after, before)) > 20
                _assert_same(after, _restated(before, u, lights, boxes, models, stamps, procedural_region[1], W, H), "frame %d" % k)
            assert np.array_equal(ctx.read_history(), clean.read_history())
            assert ctx.accumulation() == clean.accumulation()
        assert len(np.unique(clean.read_history())) > 1


# ---- rt_stamp_destroy behind an enqueued call ---------------------------------------------------------------------------------------------
def test_stamp_destroy_straight_after_an_async_call(frame_ctx, region_mine):
    W, H = SHAPES[1]
    (ctx, _, _), u = frame_ctx[SHAPES[1]], _u()
    mats, state = shadow_ref.small_stamp(seed=9, extent=(6, 5, 6))
    sid = ctx.stamp_create(mats, state)
    stamps = {sid: (mats, state)}
    before = _fresh_frame(ctx, u)
    lights = scatter_lights(before, u, W, H, 32, 51)
    rng = np.random.default_rng(51)
    models = models_at(midpoints(before, u, W, H, lights, 200, rng), sid, 51, extent=(6, 5, 6), scales=(0.25, 0.125))
    d = _dev(lights)
    torch.cuda.synchronize()
    ctx.draw_frame(u)                                                  # the call queues behind a frame
    ctx.add_lights_occluded_async(u, d, None, models)
    ctx.stamp_destroy(sid)                                             # waits for the call; the arrays are freed after it
    fill = [ctx.stamp_create(np.ones((12, 12, 12), dtype=np.uint32), np.full((12, 12, 12), se.SOLID, dtype=np.uint8)) for _ in range(4)]
    got = _all(ctx)
    want = _restated(before, u, lights, None, models, stamps, region_mine, W, H)
    _assert_same(got, want, "call, then destroy")
    assert _differ(want, _unoccluded(before, u, lights, region_mine, W, H))
    assert _code(ctx.add_lights_occluded, u, lights, None, models) == abi.RT_ERR_INVALID_ARG
    for s in fill:
        ctx.stamp_destroy(s)


# ---- ordering against world changes ---------------------------------------------------------------------------------------------------
def test_world_edits_and_lights_keep_their_order_without_a_host_sync(procedural_region, blue_noise):
    W, H = 100, 60
    u = _u()
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        before = _fresh_frame(ctx, u)
        open_mine = _mine(ctx)
        surface, P, axis, even = pl.surface_points(before, u, W, H)
        ys, xs = np.nonzero(surface & (axis == 2) & even)
        k = np.argsort(before["depth_f32"][ys, xs], kind="stable")[len(ys) // 10]           # a near pixel that faces up
        p = P[ys[k], xs[k]].astype(np.float64)
        lights = render.make_point_lights([p + np.array([0.0, 0.0, 20.0])], 60.0, (900.0, 600.0, 300.0))
        c = p + np.array([4.0, 0.0, 2.5])
        boxes = render.make_draw_boxes([c - 1.0], [c + 1.0], 1, 0xFF000000)                 # an entity beside the light's line
        # a roof one voxel thick, 33 x 33, five units up: the world shades what lies under it from the light above
        r = np.floor(p + np.array([0.0, 0.0, 5.0])).astype(int)
        gx, gy = np.meshgrid(np.arange(r[0] - 16, r[0] + 17), np.arange(r[1] - 16, r[1] + 17))
        xyz = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, r[2])], axis=-1) + 128
        n = len(xyz)
        ctx.edit_voxels(xyz, np.full(n, 0x1FFFFF, dtype=np.uint32), np.ones(n, dtype=bool))    # no sync: the launch reads the minefield the edit leaves
        ctx.add_lights_occluded(u, lights, boxes)
        got = _all(ctx)
        roofed_mine = _mine(ctx)
        assert roofed_mine.tobytes() != open_mine.tobytes()
        roofed, unroofed = (_restated(before, u, lights, boxes, None, {}, m, W, H) for m in (roofed_mine, open_mine))
        assert np.count_nonzero(_changed(unroofed, before)) > np.count_nonzero(_changed(roofed, before)) + 5
        assert _differ(unroofed, _unoccluded(before, u, lights, open_mine, W, H))           # the entity shades something too
        _assert_same(got, roofed, "edit, then lights")
        # the other way round: the asynchronous call, then an edit that removes the roof
        before2 = _fresh_frame(ctx, u)
        dl, db = _dev(lights), _dev(boxes)
        torch.cuda.synchronize()
        ctx.add_lights_occluded_async(u, dl, db)
        ctx.edit_voxels(xyz, np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=bool))
        ctx.sync()
        got2 = _all(ctx)
        after_mine = _mine(ctx)
        assert after_mine.tobytes() != roofed_mine.tobytes()
        _assert_same(got2, _restated(before2, u, lights, boxes, None, {}, roofed_mine, W, H), "lights, then edit")
        assert _differ(got2, _restated(before2, u, lights, boxes, None, {}, after_mine, W, H))


# ---- the mirror and the bench binary ------------------------------------------------------------------------------------------------------
def test_the_mirror_hands_its_entities_to_the_lights_step(procedural_region, blue_noise):
    from tests.test_gpu_draw_boxes import some_lights
    W, H = 96, 64
    cfg = render.make_config(W, H, spp=1, depth=2, flags=CACHE)
    g = render.Game(args=(-30, -128, 100, 1.5707964, -0.15, 0.3))
    g.set_world(*procedural_region)
    p = render.create_instance(cfg, g, blue_noise)
    p.enable_post_passes(faithful=True)
    p.draw_frame(g)
    p.wait()
    mats, state = shadow_ref.small_stamp()
    mirror_sid = p.context.stamp_create(mats, state)
    first = _all(p.context)
    u0 = abi.RtUniforms.from_buffer_copy(bytes(p.uniforms()))
    lights = scatter_lights(first, u0, W, H, 12, 37, rmin=6.0, rmax=12.0)
    boxes, models = occluders(first, u0, W, H, lights, 40, 12, 37, mirror_sid)
    box_lights, model_lights = some_lights(40), some_lights(12, seed=4)
    p.set_boxes(boxes, box_lights)
    p.set_models(models, model_lights)
    p.set_lights(lights)
    p.enable_entity_shadows(0.75)
    finals, uniforms = [], []
    for on in (False, True, False):
        p.enable_light_shadows(on)
        p.draw_frame(g)
        p.wait()
        uniforms.append(abi.RtUniforms.from_buffer_copy(bytes(p.uniforms())))
        finals.append(p.context.readback(abi.RT_BUF_FINAL_BGRA8))
    p.close()
    g.close()
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        sid = ctx.stamp_create(mats, state)
        mine = models.copy()
        mine["stamp"] = sid
        ctx.draw_frame(u0)
        for u, on, final in zip(uniforms, (False, True, False), finals):
            ctx.draw_frame(u)
            ctx.draw_boxes(u, boxes, box_lights)
            ctx.draw_stamps(u, mine, model_lights)
            ctx.shadow_entities(u, boxes, mine, 0.75)                                       # the order stays boxes, models, sun shadows, lights, denoise
            if on:
                ctx.add_lights_occluded(u, lights, boxes, mine)
            else:
                ctx.add_lights(u, lights)
            ctx.denoise(faithful=True)
            ctx.finalize()
            assert np.array_equal(ctx.readback(abi.RT_BUF_FINAL_BGRA8), final), "light shadows %s" % on
    assert np.count_nonzero((finals[0] != finals[1]).any(axis=-1)) > 30


def test_rt_bench_light_shadows_runs_and_reports(native_built):
    exe = os.path.join(ROOT, "raytrace_amd", "rt_bench")
    r = subprocess.run([exe, "--width", "128", "--height", "96", "--light-shadows", "--lights", "32", "--boxes", "64", "--models", "16"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["light_shadows"] == 32 and j["boxes"] == 64 and j["models"] == 16 and j["launches_per_call"] == 1.0
    assert j["add_lights_occluded_device_ms"] > 0 and j["add_lights_occluded_call_ms"] > 0 and j["add_lights_device_ms"] > 0
    assert j["pixels_shadowed"] > 10
    r = subprocess.run([exe, "--width", "128", "--height", "96", "--light-shadows", "--boxes", "64", "--occluders-far"], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["light_shadows"] == 64 and j["far"] == 1 and j["pixels_shadowed"] == 0
