"""Entity shadows on the GPU (rt_shadow_entities, rt_shadow_entities_async).  Every comparison is bit for bit, on all ten planes, with
tests/entity_shadow_ref.py — which has no cull, tests every occluder against every surface pixel and steps every world ray from the
shader's lines — applied to the planes read back before the call and to the minefield read back from the device: the batch sizes
round the kernel's 64-record batches and the 4096 limit on frames with partial tiles, boxes and models together, an adversarial set
(each occluder also alone), region 512, a scrolled window after a streamed slab, the filtered plane, the asynchronous call, every
refusal, the absence of leaks into the next frame and the lighting history, two frames in flight, the ordering against world edits,
every kernel route, rt_stamp_destroy behind an enqueued call, the host mirror and rt_bench.

The seeds of the scattered cases were picked on the CPU, with the restatement alone on the CPU oracle's frame (which the GPU's frame
equals bit for bit), so that all four classes of pixels occur; they are fixed."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from raytrace_amd import _lib, abi, render, world
from tests import entity_shadow_ref as ref
from tests import stamp_edits as se

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CACHE, ACC, REP, IN_FLIGHT_2 = abi.RT_FLAG_CACHE_PRIMARY, abi.RT_FLAG_ACCUMULATE, abi.RT_FLAG_REPROJECT, abi.RT_FLAG_FRAMES_IN_FLIGHT_2
POSE = dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.2, sun=0.3)     # the point-light tests' pose
SHAPES = [(100, 60), (64, 40)]            # partial 8x8 tiles on both axes; whole tiles
STAMP_EXTENT = (3, 4, 5)
# (boxes, models) -> seed per shape: the 64-record batch edges, the limit, and both kinds in one call
CASES = {(1, 0): (13, 51), (63, 0): (363, 363), (64, 0): (364, 364), (65, 0): (365, 365), (130, 0): (430, 430), (4096, 0): (4396, 4396),
         (0, 1): (2, 2), (0, 64): (564, 564), (0, 65): (565, 565), (70, 40): (610, 610)}
f32 = np.float32


def _u(seed=5, origin=None, pitch=None, lr=(0, 0, 0), sun=None):
    return po.camera_uniforms(origin or POSE["origin"], POSE["heading"], POSE["pitch"] if pitch is None else pitch,
                              POSE["sun"] if sun is None else sun, seed, lr)


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


def _restated(before, u, boxes, models, stamps, mine, W, H, R=256, strength=1.0, classes=None):
    want = ref.shadow_entities({k: v for k, v in before.items() if k != "final_bgra8"}, u, boxes, models, stamps, mine, W, H, R, strength,
                               classes=classes)
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
    """The tests' small sparse stamp on `ctx`: ({id: (materials, state)}, id)."""
    mats, state = ref.small_stamp()
    sid = ctx.stamp_create(mats, state)
    return {sid: (mats, state)}, sid


@pytest.fixture(scope="module")
def frame_ctx(procedural_region, blue_noise):
    """One context per frame shape (spp 1, depth 2 on the small terrain fixture) with the small stamp, shared by the tests that only
    need a frame to shade."""
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


def scattered(before, u, W, H, nboxes, nmodels, seed, sid):
    boxes = ref.scatter_boxes(before, u, W, H, nboxes, seed) if nboxes else None
    models = ref.scatter_models(before, u, W, H, nmodels, seed, sid, STAMP_EXTENT, scales=(1.0, 0.125)) if nmodels else None
    return boxes, models


# ---- shapes and counts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES), ids=["%db%dm" % c for c in sorted(CASES)])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_batches_equal_the_restatement(shape, case, frame_ctx, region_mine):
    W, H = shape
    (ctx, stamps, sid), u = frame_ctx[shape], _u()
    before = _fresh_frame(ctx, u)
    boxes, models = scattered(before, u, W, H, case[0], case[1], CASES[case][SHAPES.index(shape)], sid)
    classes = ref.masks(before, u, boxes, models, stamps, region_mine, W, H)
    for name in ("changed", "world", "open", "sky"):                      # the comparison does not pass on a trivial input
        assert classes[name].any(), "no pixel of class '%s'" % name
    ctx.shadow_entities(u, boxes, models)
    got = _all(ctx)
    _assert_same(got, _restated(before, u, boxes, models, stamps, region_mine, W, H, classes=classes), "%d boxes, %d models" % case)
    assert not _changed(got, before)[~classes["changed"]].any()          # (a changed pixel that was black already keeps its bits)


def test_strength_scales_the_term(frame_ctx, region_mine):
    W, H = SHAPES[0]
    (ctx, stamps, sid), u = frame_ctx[SHAPES[0]], _u()
    results = []
    for strength in (1.0, 0.375):
        before = _fresh_frame(ctx, u)
        boxes, models = scattered(before, u, W, H, 70, 40, 610, sid)
        ctx.shadow_entities(u, boxes, models, strength)
        results.append(_all(ctx))
        _assert_same(results[-1], _restated(before, u, boxes, models, stamps, region_mine, W, H, strength=strength), "strength %g" % strength)
    assert _differ(results[0], results[1])


# ---- the adversarial set ----------------------------------------------------------------------------------------------------------------
def adversarial(before, u, W, H, mine, ctx):
    """[(name, boxes or None, models or None, stamps)]."""
    surface, P, axis, even = ref.surface_points(before, u, W, H)
    s = ref.sun_of(u)[0].astype(np.float64)
    ys, xs = np.nonzero(surface)
    lit = np.zeros(surface.shape, dtype=bool)
    lit[surface] = ref.trace_kind(mine, 256, (0, 0, 0), P[surface], ref.sun_of(u)[0]) == ref.AIR
    ly, lx = np.nonzero(lit & (axis == 2) & even)                       # sunlit pixels that face up
    pick = lambda k: P[ly[(k * 331) % len(ly)], lx[(k * 331) % len(ly)]].astype(np.float64)
    out = []

    def box(name, lo, hi):
        b = np.zeros(1, dtype=render.DRAW_BOX_DTYPE)
        b["lo"][0], b["hi"][0], b["material"], b["emission"] = np.asarray(lo, dtype=f32), np.asarray(hi, dtype=f32), 0x1FFFFF, 0xFF000000
        out.append((name, b, None, {}))

    p = pick(1)
    box("a box containing a pixel's P'", p - 0.75, p + 0.75)
    p = pick(2)
    box("a box whose low face lies on a pixel's P' plane", (p[0] - 1.0, p[1] - 1.0, f32(p[2])), (p[0] + 1.0, p[1] + 1.0, p[2] + 1.0))
    p = pick(3)
    box("a box whose high face lies on a pixel's P' plane", (p[0] - 1.0, p[1] - 1.0, p[2] - 1.0), (p[0] + 1.0, p[1] + 1.0, f32(p[2])))
    # the bounds of one 8x8 tile's P': a box whose low corner IS the bounds' high corner, and one a step along the sun from it
    ty, tx = (ly[len(ly) // 2] // 8) * 8, (lx[len(ly) // 2] // 8) * 8
    tile = P[ty:ty + 8, tx:tx + 8][surface[ty:ty + 8, tx:tx + 8]]
    blo, bhi = tile.min(axis=0), tile.max(axis=0)
    box("a box touching the tile bounds' corner", bhi, bhi.astype(np.float64) + 1.0)
    box("a box whose high corner is the tile bounds' low corner", blo.astype(np.float64) - 1.0, blo)
    p = pick(4)
    box("a box behind every pixel it could shade (t_out < 0)", p - 4.0 * s - 0.5, p - 4.0 * s + 0.5)
    box("coordinates at 2^22", (4194302.0, -4194304.0, 4194303.0), (4194304.0, -4194302.0, 4194304.0))
    box("a box that spans the frame's surfaces", P[surface].min(axis=0).astype(np.float64) - 1.0, P[surface].max(axis=0).astype(np.float64) + 1.0)
    # models: the smallest and the largest scale, and an all-AIR model
    mats, state = ref.small_stamp()
    sid = ctx.stamp_create(mats, state)
    air = ctx.stamp_create(np.zeros_like(mats), np.full_like(state, se.AIR))
    stamps = {sid: (mats, state), air: (np.zeros_like(mats), np.full_like(state, se.AIR))}
    p = pick(5)
    tiny = ref.stamps_ref.batch([ref.stamps_ref.model(sid, (p + s * 0.05 - 0.008).astype(f32), 1.0 / 256.0, 13)])
    out.append(("a model at scale 2^-8", None, tiny, stamps))
    p = pick(6)
    out.append(("a model at scale 64", None, ref.stamps_ref.batch([ref.stamps_ref.model(sid, (p + s * 200.0 - 96.0).astype(f32), 64.0, 29)]), stamps))
    p = pick(7)
    out.append(("a model at scale 64 that contains the pixels", None, ref.stamps_ref.batch([ref.stamps_ref.model(sid, (p - 100.0).astype(f32), 64.0, 6)]), stamps))
    out.append(("an all-AIR model", None, ref.stamps_ref.batch([ref.stamps_ref.model(air, (p + s * 3.0 - 1.5).astype(f32), 1.0, 0)]), stamps))
    return out, (sid, air)


def test_adversarial_set_equals_the_restatement(frame_ctx, region_mine):
    W, H = SHAPES[0]
    (ctx, _, _), u = frame_ctx[SHAPES[0]], _u()
    before = _fresh_frame(ctx, u)
    rows, made = adversarial(before, u, W, H, region_mine, ctx)
    stamps = rows[-1][3]
    counts = {}
    for name, boxes, models, _ in rows:                                   # each occluder alone: a wrong cull cannot hide behind another
        before = _fresh_frame(ctx, u)
        classes = ref.masks(before, u, boxes, models, stamps, region_mine, W, H)
        ctx.shadow_entities(u, boxes, models)
        _assert_same(_all(ctx), _restated(before, u, boxes, models, stamps, region_mine, W, H, classes=classes), name)
        counts[name] = int(classes["changed"].sum() + classes["world"].sum())
    assert counts["a box containing a pixel's P'"] > 0 and counts["a box that spans the frame's surfaces"] == int(classes["sky"].size - classes["sky"].sum())
    assert counts["a box behind every pixel it could shade (t_out < 0)"] == 0 and counts["coordinates at 2^22"] == 0 and counts["an all-AIR model"] == 0
    assert counts["a model at scale 64"] > 0 and counts["a model at scale 64 that contains the pixels"] > 0
    # ... and all of them in one call
    before = _fresh_frame(ctx, u)
    boxes = np.concatenate([r[1] for r in rows if r[1] is not None])
    models = np.concatenate([r[2] for r in rows if r[2] is not None])
    ctx.shadow_entities(u, boxes, models)
    _assert_same(_all(ctx), _restated(before, u, boxes, models, stamps, region_mine, W, H), "the adversarial set in one call")
    for s in made:
        ctx.stamp_destroy(s)


def test_a_sun_direction_with_a_zero_component(frame_ctx, region_mine):
    """sun_angle = 0 gives s_y == 0 exactly: the slab test's zero-direction rule and the cull's run on the device."""
    W, H = SHAPES[0]
    (ctx, stamps, sid), u = frame_ctx[SHAPES[0]], _u(sun=0.0)
    assert ref.sun_of(u)[0][1] == 0.0
    before = _fresh_frame(ctx, u)
    boxes, models = scattered(before, u, W, H, 130, 30, 77, sid)
    surface, P, _, _ = ref.surface_points(before, u, W, H)
    edge = boxes[:8].copy()                                               # boxes whose y slab starts or ends AT a pixel's P'_y
    pts = P[surface][:: max(1, int(surface.sum()) // 8)][:8]
    edge["lo"][:, 1], edge["hi"][:, 1] = pts[:, 1], pts[:, 1] + f32(1.5)
    edge["lo"][:, [0, 2]], edge["hi"][:, [0, 2]] = pts[:, [0, 2]] - f32(0.5), pts[:, [0, 2]] + f32(40.0)
    boxes = np.concatenate([boxes, edge])
    classes = ref.masks(before, u, boxes, models, stamps, region_mine, W, H)
    assert classes["changed"].sum() > 10 and classes["open"].sum() > 10
    ctx.shadow_entities(u, boxes, models)
    _assert_same(_all(ctx), _restated(before, u, boxes, models, stamps, region_mine, W, H, classes=classes), "s_y == 0")


def test_an_entity_shades_its_own_averted_faces(frame_ctx, region_mine):
    """A box drawn by rt_draw_boxes and then used as its own occluder: the faces turned from the sun change, those turned to it do not."""
    W, H = SHAPES[0]
    (ctx, _, _), u = frame_ctx[SHAPES[0]], _u()
    bare = _fresh_frame(ctx, u)
    surface, P, axis, even = ref.surface_points(bare, u, W, H)
    lit = np.zeros(surface.shape, dtype=bool)
    lit[surface] = ref.trace_kind(region_mine, 256, (0, 0, 0), P[surface], ref.sun_of(u)[0]) == ref.AIR
    ys, xs = np.nonzero(lit & (axis == 2) & even)
    k = np.argsort(bare["depth_f32"][ys, xs], kind="stable")[len(ys) // 10]               # a near sunlit pixel that faces up
    half = 0.06 * float(bare["depth_f32"][ys[k], xs[k]]) / 32.0                           # (the terrain is some 150 units away)
    c = P[ys[k], xs[k]].astype(np.float64) + np.array([0.0, 0.0, half + 1.0])            # a box one unit above it
    boxes = render.make_draw_boxes([c - half], [c + half], 0x1FFFFF, 0xFF000000)
    face = np.zeros(6, dtype=render.PROBE_LIGHT_DTYPE)
    face["light"] = 10.0
    ctx.draw_boxes(u, boxes, face)
    before = _all(ctx)
    entity = before["depth_f32"] != bare["depth_f32"]
    assert entity.sum() > 30
    classes = ref.masks(before, u, boxes, None, {}, region_mine, W, H)
    ctx.shadow_entities(u, boxes)
    got = _all(ctx)
    _assert_same(got, _restated(before, u, boxes, None, {}, region_mine, W, H, classes=classes), "an entity as its own occluder")
    s = ref.sun_of(u)[0]
    normal = np.minimum(before["normal_r8"].astype(int), 5)
    facing = np.where(normal % 2 == 0, s[normal // 2], -s[normal // 2]) > 0               # the face looks at the sun
    changed = _changed(got, before)
    assert (entity & ~facing).sum() > 5 and (entity & facing).sum() > 5
    assert classes["open"][entity & facing].all()                         # a face turned to the sun leaves its own box
    # a face turned from it re-enters it — but for a sliver along the edge the ray leaves by: P' is 1/32 off the face, so the ray
    # needs (1/32) / s_k to come back, and within about s_j / s_k / 32 (0.1 units here) of that edge it has passed the box by then
    assert (~classes["open"])[entity & ~facing].sum() > 0.9 * (entity & ~facing).sum()
    assert changed[entity & ~facing].any() and np.array_equal(changed[entity], classes["changed"][entity])   # ... and goes dark where the world lets the sun in
    assert changed[~entity].any()                                         # and the box shades the ground behind it


def test_a_frame_that_is_all_sky_keeps_every_bit(frame_ctx):
    W, H = SHAPES[0]
    (ctx, stamps, sid), u = frame_ctx[SHAPES[0]], _u(pitch=1.2)
    before = _fresh_frame(ctx, u)
    assert (before["depth_r16"] == 65535).all()
    o = np.array(u.origin[:]) + 5.0 * np.array(u.forward[:])
    ctx.shadow_entities(u, render.make_draw_boxes([o - 1.0], [o + 1.0], 1, 0xFF000000))
    _assert_same(_all(ctx), before, "all sky")


# ---- regions and windows ----------------------------------------------------------------------------------------------------------------
def test_region_512(blue_noise):
    W, H = 64, 40
    u = _u()
    with _ctx(None, blue_noise, W, H, spp=1, depth=2, region=512) as big:          # the region generated on the device
        stamps, sid = _small_stamp(big)
        before = _fresh_frame(big, u)
        boxes, models = scattered(before, u, W, H, 130, 40, 41, sid)
        mine = _mine(big, 512)
        big.shadow_entities(u, boxes, models)
        got = _all(big)
        _assert_same(got, _restated(before, u, boxes, models, stamps, mine, W, H, 512), "region 512")
        assert np.count_nonzero(_changed(got, before)) > 10


def test_a_scrolled_window_after_a_streamed_slab(procedural_region, blue_noise):
    """lr != 0: the kernel's other template.  The slab that entered at the window's far side is in the minefield the sun rays read."""
    W, H = 100, 60
    lr = (16, 0, 0)
    u = _u(origin=(-14.0, -128.0, 100.0), lr=lr)
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        stamps, sid = _small_stamp(ctx)
        ctx.generate_slice(world.DEFAULT_SEED, 0, (128, -128, -128))                # world x 128..143 into texels 0..15
        before = _fresh_frame(ctx, u)
        mine = _mine(ctx)
        assert mine.tobytes() != procedural_region[1].tobytes()
        boxes, models = scattered(before, u, W, H, 200, 40, 43, sid)
        ctx.shadow_entities(u, boxes, models)
        got = _all(ctx)
        _assert_same(got, _restated(before, u, boxes, models, stamps, mine, W, H), "lr %s" % (lr,))
        assert np.count_nonzero(_changed(got, before)) > 10
        # a camera that sees the slab, and one box over every surface: the pixels at x = 128 .. 143 lie outside the window of lr = 0,
        # where their sun rays would leave at once; here they are traced through the slab
        u2 = _u(origin=(40.0, -128.0, 100.0), lr=lr)
        before = _fresh_frame(ctx, u2)
        surface, P, _, _ = ref.surface_points(before, u2, W, H)
        pts = P[surface].astype(np.float64)
        assert (pts[:, 0] > 128.5).sum() > 10
        boxes = render.make_draw_boxes([pts.min(axis=0) - 1.0], [pts.max(axis=0) + 1.0], 1, 0xFF000000)
        ctx.shadow_entities(u2, boxes)
        got = _all(ctx)
        _assert_same(got, _restated(before, u2, boxes, None, stamps, mine, W, H), "lr %s, every surface pixel shaded" % (lr,))
        zero = _u(origin=(40.0, -128.0, 100.0))
        assert _differ(_restated(before, zero, boxes, None, stamps, mine, W, H), got)            # lr is read


# ---- the filtered plane ------------------------------------------------------------------------------------------------------------------
def test_after_the_denoise_each_plane_gets_the_change_in_its_own_representation(frame_ctx, region_mine, blue_noise):
    W, H = SHAPES[0]
    (ctx, stamps, sid), u = frame_ctx[SHAPES[0]], _u()
    raw = _fresh_frame(ctx, u)
    ctx.denoise(faithful=True)
    before = _all(ctx)
    assert before["lighting_rgba16"].tobytes() != raw["lighting_rgba16"].tobytes() and before["lighting_f32"].tobytes() == raw["lighting_f32"].tobytes()
    boxes, models = scattered(before, u, W, H, 130, 40, 53, sid)
    ctx.shadow_entities(u, boxes, models)
    got = _all(ctx)
    _assert_same(got, _restated(before, u, boxes, models, stamps, region_mine, W, H), "after rt_denoise")
    ch = _changed(got, before)
    assert ch.sum() > 10 and (got["lighting_rgba16"][ch] != before["lighting_rgba16"][ch]).any()
    ctx.finalize()
    fin = po.finalize(got["albedo_rgba8"], got["emission_rgba8"], got["fog_rgba8"], got["lighting_rgba16"], got["depth_r16"], blue_noise)
    assert np.array_equal(ctx.readback(abi.RT_BUF_FINAL_BGRA8), fin)


# ---- async ------------------------------------------------------------------------------------------------------------------------------
def test_async_equals_sync_and_skips_invalid_boxes(frame_ctx, region_mine):
    W, H = SHAPES[0]
    (ctx, stamps, sid), u = frame_ctx[SHAPES[0]], _u()
    before = _fresh_frame(ctx, u)
    boxes, models = scattered(before, u, W, H, 96, 40, 7, sid)
    bad = boxes.copy()
    bad["lo"][5][0] = np.nan
    bad["hi"][16][1] = bad["lo"][16][1]
    bad["hi"][27][2] = np.inf
    bad["lo"][38][0] = -4194305.0
    bad["lo"][49], bad["hi"][49] = boxes["hi"][49], boxes["lo"][49]
    skipped = ~ref.boxes_ref.valid(bad)
    assert np.count_nonzero(skipped) == 5
    ctx.shadow_entities_async(u, _dev(bad), models)
    got_bad = _all(ctx)
    _assert_same(got_bad, _restated(before, u, bad, models, stamps, region_mine, W, H), "async, invalid records")
    _assert_same(got_bad, _restated(before, u, boxes[~skipped], models, stamps, region_mine, W, H), "async, the valid records alone")
    assert _code(ctx.shadow_entities, u, bad, models) == abi.RT_ERR_INVALID_ARG
    _assert_same(_all(ctx), got_bad, "after the refused call")
    before2 = _fresh_frame(ctx, u)
    _assert_same(before2, before)
    ctx.shadow_entities(u, boxes[~skipped], models)
    _assert_same(_all(ctx), got_bad, "sync without the invalid boxes")
    # ... boxes alone, models alone, and on a caller's stream
    for b, m in ((boxes, None), (None, models)):
        before3 = _fresh_frame(ctx, u)
        ctx.shadow_entities_async(u, None if b is None else _dev(b), m)
        _assert_same(_all(ctx), _restated(before3, u, b, m, stamps, region_mine, W, H), "async, one kind")
    s = torch.cuda.Stream()
    d = _dev(boxes)
    torch.cuda.synchronize()
    ctx.set_stream(s.cuda_stream)
    try:
        ctx.draw_frame(u)
        ctx.shadow_entities_async(u, d, models, 0.5)
        s.synchronize()
        _assert_same(_all(ctx), _restated(before, u, boxes, models, stamps, region_mine, W, H, strength=0.5), "on a caller's stream")
    finally:
        ctx.set_stream(0)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(procedural_region, blue_noise):
    W, H = 64, 40
    lib = _lib.amd()
    u = _u()
    some = render.make_draw_boxes([(-30.0, -100.0, 90.0)] * 8, [(-29.0, -99.0, 91.0)] * 8, 1, 0xFF000000)
    with render.Context(render.make_config(W, H, spp=1, depth=2, flags=CACHE)) as empty:
        empty.upload_noise(blue_noise)
        assert _code(empty.shadow_entities, u, some) == abi.RT_ERR_NOT_READY                # no frame, no world
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        h = ctx.handle
        stamps, sid = _small_stamp(ctx)
        assert _code(ctx.shadow_entities, u, some) == abi.RT_ERR_NOT_READY                  # no frame yet
        assert _code(ctx.shadow_entities_async, u, _dev(some)) == abi.RT_ERR_NOT_READY
        before = _fresh_frame(ctx, u)
        boxes, models = scattered(before, u, W, H, 8, 4, 3, sid)
        pb, pm = boxes.ctypes.data_as(C.c_void_p), models.ctypes.data_as(C.c_void_p)
        d_boxes = _dev(boxes)
        db = C.c_void_p(d_boxes.data_ptr())
        many = np.concatenate([boxes] * 513)[:4097].copy()
        d_many = _dev(many)
        many_models = np.concatenate([models] * 1025)[:4097].copy()
        assert lib.rt_shadow_entities(h, C.byref(u), many.ctypes.data_as(C.c_void_p), 4097, None, 0, 1.0) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_shadow_entities_async(h, C.byref(u), C.c_void_p(d_many.data_ptr()), 4097, None, 0, 1.0) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_shadow_entities(h, C.byref(u), None, 0, many_models.ctypes.data_as(C.c_void_p), 4097, 1.0) == abi.RT_ERR_INVALID_ARG
        for call, p in ((lib.rt_shadow_entities, pb), (lib.rt_shadow_entities_async, db)):
            assert call(h, None, p, 8, pm, 4, 1.0) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), None, 8, pm, 4, 1.0) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), p, 8, None, 4, 1.0) == abi.RT_ERR_INVALID_ARG
            assert call(h, C.byref(u), None, 0, None, 0, 1.0) == abi.RT_OK                  # no occluders need no arrays
            for strength in (0.0, -0.5, 1.0000001, np.nan, np.inf, -np.inf):
                assert call(h, C.byref(u), p, 8, pm, 4, strength) == abi.RT_ERR_INVALID_ARG, strength
        # host memory and unaligned device memory are not what the asynchronous call takes
        assert lib.rt_shadow_entities_async(h, C.byref(u), pb, 8, None, 0, 1.0) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_shadow_entities_async(h, C.byref(u), C.c_void_p(d_boxes.data_ptr() + 4), 7, None, 0, 1.0) == abi.RT_ERR_INVALID_ARG
        for field, k, value in (("lo", 1, np.nan), ("lo", 0, 4194305.0), ("hi", 2, np.inf), ("hi", 0, -1.0e6)):
            bad = boxes.copy()
            bad[field][5][k] = value
            assert _code(ctx.shadow_entities, u, bad, models) == abi.RT_ERR_INVALID_ARG, (field, value)
        for field, value in (("stamp", 999), ("orient", 48), ("scale", 0.001), ("scale", 65.0), ("reserved", 1), ("scale", np.nan)):
            bad = models.copy()
            bad[field][2] = value
            assert _code(ctx.shadow_entities, u, boxes, bad) == abi.RT_ERR_INVALID_ARG, (field, value)
            assert _code(ctx.shadow_entities_async, u, d_boxes, bad) == abi.RT_ERR_INVALID_ARG, (field, value)
        _assert_same(_all(ctx), before, "after the rejected calls")
        ctx.shadow_entities(u, boxes, models)                                               # and the context still works
        _assert_same(_all(ctx), _restated(before, u, boxes, models, stamps, procedural_region[1], W, H))
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2, tile_rank=0, tile_world=2) as tiles:
        tiles.draw_frame(u)
        tiles.sync()
        assert _code(tiles.shadow_entities, u, some) == abi.RT_ERR_UNIMPLEMENTED
        d_some = _dev(some)
        assert lib.rt_shadow_entities_async(tiles.handle, C.byref(u), C.c_void_p(d_some.data_ptr()), 8, None, 0, 1.0) == abi.RT_ERR_UNIMPLEMENTED


def test_no_occluders_drop_no_prepass_and_a_call_does(procedural_region, blue_noise):
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
        boxes, models = scattered(_all(ctx), u, W, H, 24, 8, 13, sid)
        ctx.shadow_entities(u, boxes[:0], models[:0])
        ctx.sync()
        assert int(ctx.timing().other_launches) == 0                     # nothing enqueued
        assert frame_launches() == again                                 # ... and the prepass is still the slot's
        ctx.shadow_entities(u, boxes, models)
        ctx.sync()
        assert int(ctx.timing().other_launches) == 1                     # one launch for boxes and models together
        assert frame_launches() == fresh                                 # the call dropped the prepass


# ---- no leak into the next frame ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["paths", "paths-2-in-flight", "frame"])
def test_the_shadow_does_not_leak_into_the_next_frame(route, procedural_region, blue_noise):
    """A still camera.  The persistent route with cached primaries skips the prepass of a frame whose camera and world are unchanged:
    a slot whose lighting rt_shadow_entities wrote must not be taken for one that still holds its prepass.  With two frames in flight
    the call shades the frame drawn last and leaves the other slot alone.  (Multi-sample frames: the planes hold a mean of samples.)"""
    W, H = 136, 72
    u = _u()
    in_flight = 2 if route == "paths-2-in-flight" else 1
    kw = dict(spp=4, depth=2, kernel=abi.RT_KERNEL_PATHS, flags=CACHE | (IN_FLIGHT_2 if in_flight == 2 else 0))
    if route == "frame":
        kw = dict(spp=1, depth=2, kernel=abi.RT_KERNEL_FRAME, flags=CACHE)
    nframes = 2 if in_flight == 1 else 3
    with _ctx(procedural_region, blue_noise, W, H, **kw) as clean:
        for _ in range(nframes):
            clean.draw_frame(u)
        clean.sync()
        want = _all(clean)
    with _ctx(procedural_region, blue_noise, W, H, **kw) as ctx:
        assert ctx.info().frames_in_flight == in_flight
        stamps, sid = _small_stamp(ctx)
        for k in range(nframes - 1):
            before = _fresh_frame(ctx, u)
            boxes, models = scattered(before, u, W, H, 100, 30, 13 + k, sid)
            ctx.shadow_entities(u, boxes, models)
            after = _all(ctx)
            assert np.count_nonzero(_changed(after, before)) > 20
            _assert_same(after, _restated(before, u, boxes, models, stamps, procedural_region[1], W, H), "frame %d" % k)
        _assert_same(_fresh_frame(ctx, u), want, "the frame after the shadows")


def test_history_of_a_reprojecting_context_is_untouched(procedural_region, blue_noise):
    W, H = 96, 64
    kw = dict(spp=1, depth=2, flags=ACC | REP | CACHE)
    cams = [_u(seed=10 + k, origin=(-30.0 + 0.25 * min(k, 2), -128.0, 100.0 - 0.1 * min(k, 2))) for k in range(6)]   # moves, then holds still
    with _ctx(procedural_region, blue_noise, W, H, **kw) as clean, _ctx(procedural_region, blue_noise, W, H, **kw) as ctx:
        stamps, sid = _small_stamp(ctx)
        for k, u in enumerate(cams):
            want = _fresh_frame(clean, u)
            before = _fresh_frame(ctx, u)
            _assert_same(before, want, "frame %d before its shadows" % k)
            if k < 3:                                               # the next three frames follow the last call
                boxes, models = scattered(before, u, W, H, 100, 30, 17 + k, sid)
                ctx.shadow_entities(u, boxes, models)
                after = _all(ctx)
                assert np.count_nonzero(_changed(after, before)) > 20
                _assert_same(after, _restated(before, u, boxes, models, stamps, procedural_region[1], W, H), "frame %d" % k)
            assert np.array_equal(ctx.read_history(), clean.read_history())
            assert ctx.accumulation() == clean.accumulation()
        assert len(np.unique(clean.read_history())) > 1


# ---- ordering against world changes ---------------------------------------------------------------------------------------------------
def test_world_edits_and_shadows_keep_their_order_without_a_host_sync(procedural_region, blue_noise):
    W, H = 100, 60
    u = _u()
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        before = _fresh_frame(ctx, u)
        open_mine = _mine(ctx)
        surface, P, axis, even = ref.surface_points(before, u, W, H)
        s = ref.sun_of(u)[0].astype(np.float64)
        lit = np.zeros(surface.shape, dtype=bool)
        lit[surface] = ref.trace_kind(open_mine, 256, (0, 0, 0), P[surface], ref.sun_of(u)[0]) == ref.AIR
        ys, xs = np.nonzero(lit & (axis == 2) & even)
        k = np.argsort(before["depth_f32"][ys, xs], kind="stable")[len(ys) // 10]           # a near sunlit pixel that faces up
        p = P[ys[k], xs[k]].astype(np.float64)
        c = p + 8.0 * s
        boxes = render.make_draw_boxes([c - 3.0], [c + 3.0], 1, 0xFF000000)                 # an entity eight units up the sun's line
        # a roof one voxel thick, 17 x 17, sixteen units up the sun's line: the world shades what the entity shades
        r = np.floor(p + 16.0 * s).astype(int)
        gx, gy = np.meshgrid(np.arange(r[0] - 8, r[0] + 9), np.arange(r[1] - 8, r[1] + 9))
        xyz = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, r[2])], axis=-1) + 128
        n = len(xyz)
        ctx.edit_voxels(xyz, np.full(n, 0x1FFFFF, dtype=np.uint32), np.ones(n, dtype=bool))    # no sync: the launch reads the minefield the edit leaves
        ctx.shadow_entities(u, boxes)
        got = _all(ctx)
        roofed_mine = _mine(ctx)
        assert roofed_mine.tobytes() != open_mine.tobytes()
        roofed, unroofed = _restated(before, u, boxes, None, {}, roofed_mine, W, H), _restated(before, u, boxes, None, {}, open_mine, W, H)
        assert np.count_nonzero(_changed(unroofed, before)) > np.count_nonzero(_changed(roofed, before)) + 5
        _assert_same(got, roofed, "edit, then shadows")
        # the other way round: the asynchronous call, then an edit that removes the roof
        before2 = _fresh_frame(ctx, u)
        d = _dev(boxes)
        torch.cuda.synchronize()
        ctx.shadow_entities_async(u, d)
        ctx.edit_voxels(xyz, np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=bool))
        ctx.sync()
        got2 = _all(ctx)
        after_mine = _mine(ctx)
        assert after_mine.tobytes() != roofed_mine.tobytes()
        _assert_same(got2, _restated(before2, u, boxes, None, {}, roofed_mine, W, H), "shadows, then edit")
        assert _differ(got2, _restated(before2, u, boxes, None, {}, after_mine, W, H))


# ---- every route ------------------------------------------------------------------------------------------------------------------------
def test_every_route_shades_the_same_frame(procedural_region, blue_noise):
    W, H = 100, 60
    u = _u()
    results, used = [], []
    routes = (abi.RT_KERNEL_FRAME, abi.RT_KERNEL_PATHS, abi.RT_KERNEL_PERSISTENT, abi.RT_KERNEL_WAVEFRONT, abi.RT_KERNEL_MEGA)
    boxes = models = stamps = None
    for kernel in routes:
        with _ctx(procedural_region, blue_noise, W, H, spp=2, depth=2, kernel=kernel) as ctx:
            st, sid = _small_stamp(ctx)
            before = _fresh_frame(ctx, u)
            used.append(ctx.kernel_in_use())
            if boxes is None:
                boxes, models = scattered(before, u, W, H, 130, 40, 29, sid)
                stamps = st
            assert sid == int(models["stamp"][0])                        # (a fresh context hands out the same first id)
            ctx.shadow_entities(u, boxes, models)
            results.append((before, _all(ctx)))
    assert used == list(routes)
    _assert_same(results[0][1], _restated(results[0][0], u, boxes, models, stamps, procedural_region[1], W, H), "k_frame")
    assert np.count_nonzero(_changed(results[0][1], results[0][0])) > 20
    for before, after in results[1:]:
        _assert_same(before, results[0][0], "the routes' frames")
        _assert_same(after, results[0][1], "the routes' frames with shadows")


# ---- rt_stamp_destroy behind an enqueued call ---------------------------------------------------------------------------------------------
def test_stamp_destroy_straight_after_an_async_call(frame_ctx, region_mine):
    W, H = SHAPES[1]
    (ctx, _, _), u = frame_ctx[SHAPES[1]], _u()
    mats, state = ref.small_stamp(seed=9, extent=(9, 9, 12))
    sid = ctx.stamp_create(mats, state)
    stamps = {sid: (mats, state)}
    before = _fresh_frame(ctx, u)
    models = ref.scatter_models(before, u, W, H, 300, 51, sid, (9, 9, 12), scales=(0.25, 0.125))
    ctx.draw_frame(u)                                                  # the call queues behind a frame
    ctx.shadow_entities_async(u, None, models)
    ctx.stamp_destroy(sid)                                             # waits for the call; the arrays are freed after it
    fill = [ctx.stamp_create(np.ones((12, 12, 12), dtype=np.uint32), np.full((12, 12, 12), se.SOLID, dtype=np.uint8)) for _ in range(4)]
    got = _all(ctx)
    _assert_same(got, _restated(before, u, None, models, stamps, region_mine, W, H), "call, then destroy")
    assert np.count_nonzero(_changed(got, before)) > 10
    assert _code(ctx.shadow_entities, u, None, models) == abi.RT_ERR_INVALID_ARG
    for s in fill:
        ctx.stamp_destroy(s)


# ---- the mirror and the bench binary ------------------------------------------------------------------------------------------------------
def test_the_mirror_shades_between_its_models_and_its_lights(procedural_region, blue_noise):
    from tests.test_gpu_draw_boxes import some_lights
    W, H = 96, 64
    cfg = render.make_config(W, H, spp=1, depth=2, flags=CACHE)
    g = render.Game(args=(-30, -128, 100, 1.5707964, -0.15, 0.3))
    g.set_world(*procedural_region)
    p = render.create_instance(cfg, g, blue_noise)
    p.enable_post_passes(faithful=True)
    p.draw_frame(g)
    p.wait()
    mats, state = ref.small_stamp()
    mirror_sid = p.context.stamp_create(mats, state)
    first = _all(p.context)
    u0 = abi.RtUniforms.from_buffer_copy(bytes(p.uniforms()))
    boxes, models = scattered(first, u0, W, H, 40, 12, 37, mirror_sid)
    box_lights, model_lights = some_lights(40), some_lights(12, seed=4)
    lights = render.make_point_lights(ref.surface_points(first, u0, W, H)[1][H // 3, W // 2][None] + np.array([[0.0, 0.0, 2.0]]), 9.0, (30.0, 20.0, 10.0))
    p.set_boxes(boxes, box_lights)
    p.set_models(models, model_lights)
    p.set_lights(lights)
    finals, uniforms = [], []
    for strength in (0.0, 0.75):
        p.enable_entity_shadows(strength)
        p.draw_frame(g)
        p.wait()
        uniforms.append(abi.RtUniforms.from_buffer_copy(bytes(p.uniforms())))
        finals.append(p.context.readback(abi.RT_BUF_FINAL_BGRA8))
    for bad in (-0.1, 1.5, np.nan):
        with pytest.raises(render.RtError):
            p.enable_entity_shadows(bad)
    p.close()
    g.close()
    with _ctx(procedural_region, blue_noise, W, H, spp=1, depth=2) as ctx:
        sid = ctx.stamp_create(mats, state)
        mine = models.copy()
        mine["stamp"] = sid
        ctx.draw_frame(u0)
        for u, strength, final in zip(uniforms, (0.0, 0.75), finals):
            ctx.draw_frame(u)
            ctx.draw_boxes(u, boxes, box_lights)
            ctx.draw_stamps(u, mine, model_lights)
            if strength:
                ctx.shadow_entities(u, boxes, mine, strength)
            ctx.add_lights(u, lights)
            ctx.denoise(faithful=True)
            ctx.finalize()
            assert np.array_equal(ctx.readback(abi.RT_BUF_FINAL_BGRA8), final), "strength %g" % strength
    assert np.count_nonzero((finals[0] != finals[1]).any(axis=-1)) > 30


def test_rt_bench_shadows_runs_and_reports(native_built):
    exe = os.path.join(ROOT, "raytrace_amd", "rt_bench")
    r = subprocess.run([exe, "--width", "128", "--height", "96", "--shadows", "64"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["shadows"] == 64 and j["launches_per_call"] == 1.0 and j["shadow_entities_device_ms"] > 0 and j["shadow_entities_call_ms"] > 0
    assert j["pixels_changed"] > 10
    r = subprocess.run([exe, "--width", "128", "--height", "96", "--shadows", "32", "--shadow-models", "--model-scale", "0.5"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["shadows"] == 32 and j["shadow_models"] == 1 and j["launches_per_call"] == 1.0 and j["pixels_changed"] > 0
    bad = subprocess.run([exe, "--shadows", "4097"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--shadows" in bad.stderr
