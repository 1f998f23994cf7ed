"""rt_edit_shapes on the GPU, against the numpy restatement of tests/shape_edits.py and the oracle: the resident region byte for byte
(rt_read_box) and the nibble maps (RT_SELFTEST_SCENE_MAPS) after shape batches at R = 256, 512 and 1024, on the generated world and
on arbitrary minefield values (which show the chunks that were rebuilt); equivalence with rt_edit_voxels; frames and picks on the
edited world; stream ordering against frames in flight and on a caller's stream; the accumulation reset and the boxes kept for a
history that goes on; rejections."""
import ctypes as C

import numpy as np
import pytest

from raytrace_amd import abi, render, world
from oracle import pyoracle as po
from tests import edit_history_ref as er
from tests import shape_edits as se
from tests import voxel_edits as ve
from tests.test_gpu_accumulation import _peek
from tests.test_gpu_edit_history import _ctx as _history_ctx, _frame as _history_frame
from tests.test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

MAPS = abi.RT_SELFTEST_SCENE_MAPS
CACHE = abi.RT_FLAG_CACHE_PRIMARY
W, H = 64, 64
POSE = dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.25, sun=0.3)


def _u(seed=3, **kw):
    p = dict(POSE)
    p.update(kw)
    return po.camera_uniforms(p["origin"], p["heading"], p["pitch"], p["sun"], seed)


def _ctx(region, noise=None, R=256, **kw):
    ctx = render.Context(render.make_config(W, H, region=R, **kw))
    ctx.upload_world(*region)
    if noise is not None:
        ctx.upload_noise(noise)
    return ctx


def _edit(ctx, shapes):
    """The restatement's rows are RtShapeEdit's bytes."""
    assert se.SHAPE_DTYPE == render.SHAPE_DTYPE
    ctx.edit_shapes(se.batch(shapes))


def _arbitrary_region(R):
    """Minefield values 0..30 and material words with no order in them, one 128^3 block repeated (about a thirtieth is occupied)."""
    rng = np.random.default_rng(R + 1)
    n = R // 128
    mine = np.tile(rng.integers(0, 31, size=(128, 128, 128), dtype=np.uint8), (n, n, n))
    mats = np.tile(rng.integers(0, 2 ** 32, size=(128, 128, 128), dtype=np.uint64).astype(np.uint32), (n, n, n))
    return mats, mine


@pytest.fixture(scope="module")
def regions(procedural_region):
    made = {("generated", 256): procedural_region}

    def get(kind, R):
        if (kind, R) not in made:
            made[(kind, R)] = world.generate_region(world.DEFAULT_SEED, region=R) if kind == "generated" else _arbitrary_region(R)
        return made[(kind, R)]
    return get


def _random_shapes(R, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        where, solid, word = int(rng.integers(0, 3)), int(rng.integers(0, 2)), int(rng.integers(0, 2 ** 32))
        if rng.random() < 0.5:
            lo = rng.integers(-20, R + 10, size=3)
            hi = lo + rng.integers(0, (70 if i % 25 == 0 else 12), size=3)
            out.append(se.box(lo, hi, word, solid, where))
        else:
            d = int(rng.integers(0, 140 if i % 25 == 1 else 30))
            out.append(se.sphere(rng.integers(-40, 2 * R + 40, size=3), d * d - int(rng.integers(0, 2)) * (d > 0), word, solid, where))
    return out


def _batches(R):
    """(name, shapes, what the batch is there for) in the order they are applied: the smallest batches that can go wrong."""
    far, n = R - 1, R // 64
    return [
        ("a one-voxel box", [se.box((5, 6, 7), (5, 6, 7), 0x11, 1)], 1),
        ("exactly one chunk, carved", [se.box((64, 64, 64), (127, 127, 127), 0x22, 0)], 1),
        ("2 x 2 x 2 on a chunk corner", [se.box((R - 65, 191, 63), (R - 64, 192, 64), 0x33, 1)], 8),
        ("b0 = 0, odd centre: one voxel", [se.sphere((141, 141, 2 * far + 1), 0, 0x44, 1)], 1),
        ("b0 = 0, even centre: no texel passes the axis, so nothing is touched", [se.sphere((140, 141, 141), 0, 0x45, 1)], "untouched"),
        ("b0 = 1, even centre: a chunk is touched and nothing is selected", [se.sphere((2 * R - 140, 140, 140), 1, 0x46, 1)], "rebuilt"),
        ("paint in the carved chunk: touched, nothing to select", [se.box((64, 64, 64), (100, 100, 100), 0x47, 1, se.SOLID)], "same"),
        ("radius 3.5 on a chunk corner", [se.sphere((256, 256, 256), 49, 0x55, 1)], 8),
        ("spheres centred beyond the region, clipped", [se.sphere((-21, 2 * far + 9, 300), 60 * 60, 0x66, 1),
                                                        se.sphere((2 * R + 30, 100, 100), 31 * 31, 0x67, 0)], None),
        ("wholly outside", [se.box((R, 0, 0), (R + 9, 9, 9), 0x77, 1), se.sphere((-100, -100, -100), 50 * 50, 0x78, 1),
                            se.box((-4 * R, -4 * R, -4 * R), (4 * R, 4 * R, -1), 0x79, 0)], "untouched"),
        ("two overlapping boxes, the last wins", [se.box((30, 190, 100), (75, 200, 140), 0x88, 1), se.box((60, 195, 120), (90, 210, 160), 0x99, 0)], None),
        ("fill the air, paint the solid, carve", [se.box((120, 120, R - 70), (140, 135, far), 0xA1, 1, se.AIR),
                                                  se.box((120, 120, R - 70), (140, 135, far), 0xA2, 1, se.SOLID),
                                                  se.sphere((261, 255, 2 * R - 60), 24 * 24, 0xA3, 0)], None),
        ("300 random shapes", _random_shapes(R, 300, R), None),
        ("the whole region", [se.box((0, 0, 0), (far, far, far), 0xB0B, 1)], n ** 3),
    ]


@pytest.mark.parametrize("kind", ["generated", "arbitrary"])
@pytest.mark.parametrize("R", [256, 512])
def test_region_bytes_and_maps_after_shape_batches(regions, R, kind):
    mats, mine = (a.copy() for a in regions(kind, R))
    with _ctx((mats, mine), R=R) as ctx:
        assert ctx.selftest(MAPS) == 0
        for name, shapes, expect in _batches(R):
            before = mine.copy() if isinstance(expect, str) else None
            touched = se.apply_shapes(mats, mine, se.batch(shapes))
            _edit(ctx, shapes)
            gm, gf = ctx.read_box((0, 0, 0), (R, R, R))
            assert np.array_equal(gf, mine), "%s: minefield differs at %d voxels" % (name, int(np.count_nonzero(gf != mine)))
            assert np.array_equal(gm, mats), "%s: materials differ at %d voxels" % (name, int(np.count_nonzero(gm != mats)))
            assert ctx.selftest(MAPS) == 0, name
            # what the batch is there for
            if expect == "untouched":
                assert touched == [] and np.array_equal(before, mine), name
            elif expect == "rebuilt":      # (the generated world is pack_into's own: a rebuild gives the bytes it had; arbitrary values show it)
                assert len(touched) == 1 and (kind == "generated") == np.array_equal(before, mine), name
            elif expect == "same":
                assert len(touched) == 1 and np.array_equal(before, mine), name
            elif expect is not None:
                assert len(touched) == expect, name
        assert not gf.any() and (gm == 0xB0B).all()


def test_region_bytes_at_1024_on_a_world_the_host_never_held(native_built):
    """rt_generate_world, then the chunk row x = 64..384 read back: one box and one sphere across chunks 2 and 3, which share a coarse
    nibble-map word, against the restatement applied to the bytes read."""
    R = 1024
    y0, z0 = 448, 512                                                 # (the default window's terrain surface runs through this row)
    with render.Context(render.make_config(W, H, region=R)) as ctx:
        ctx.generate_world(world.DEFAULT_SEED)
        mats, mine = ctx.read_box((64, y0, z0), (320, 64, 64))
        assert 0 < np.count_nonzero(mine == 0) < mine.size
        shapes = [se.box((150, y0 + 10, z0), (230, y0 + 40, z0 + 30), 0xC1, 1, se.AIR),
                  se.sphere((2 * 192, 2 * y0 + 64, 2 * z0 + 61), 55 * 55, 0xC2, 0)]
        assert se.apply_shapes(mats, mine, se.batch(shapes), origin=(64, y0, z0), region=R) == [(2, y0 // 64, z0 // 64), (3, y0 // 64, z0 // 64)]
        _edit(ctx, shapes)
        gm, gf = ctx.read_box((64, y0, z0), (320, 64, 64))
        assert np.array_equal(gf, mine) and np.array_equal(gm, mats)
        assert (gm == 0xC2).any() and not (gf[:, :, :64] != mine[:, :, :64]).any()
        assert ctx.selftest(MAPS) == 0


def test_shapes_equal_the_enumerated_voxel_edits(regions):
    """Two contexts on the same arbitrary world: in every chunk these shapes touch they select a voxel, so rt_edit_voxels with one
    record per selected voxel rebuilds the same chunks."""
    mats, mine = regions("arbitrary", 256)
    shapes = se.batch([se.box((60, 60, 60), (70, 70, 70), 1, 1), se.sphere((131, 131, 131), 81, 2, 0), se.box((0, 200, 250), (255, 201, 255), 3, 1, se.AIR),
                       se.sphere((256, 256, 256), 49, 4, 1, se.AIR), se.box((60, 60, 60), (70, 70, 70), 5, 0, se.SOLID)])
    xyz, words, solid, touched = se.enumerate_records(mats, mine, shapes)
    assert sorted(set(map(tuple, (xyz >> 6).tolist()))) == touched and len(touched) >= 12
    with _ctx((mats, mine)) as a, _ctx((mats, mine)) as b:
        a.edit_shapes(shapes)
        b.edit_voxels(xyz, words, solid)
        (am, af), (bm, bf) = a.read_box((0, 0, 0), (256, 256, 256)), b.read_box((0, 0, 0), (256, 256, 256))
        assert np.array_equal(af, bf) and np.array_equal(am, bm) and not np.array_equal(af, mine)
        assert a.selftest(MAPS) == 0


# ---- frames and queries ---------------------------------------------------------------------------------------------------------
def _scene_shapes():
    """A wall in front of the default camera, a crater in the ground ahead of it and a slab overhead."""
    word = po.lib().rt_oracle_pack_material(200, 120, 60, 0)
    return [se.box((88, 38, 223), (107, 38, 237), word, 1), se.sphere((197, 141, 301), 49 * 49, 0, 0),
            se.box((68, 8, 248), (127, 27, 248), word, 1, se.AIR)]


@pytest.fixture(scope="module")
def edited_256(procedural_region):
    m2, f2 = (a.copy() for a in procedural_region)
    assert len(se.apply_shapes(m2, f2, se.batch(_scene_shapes()))) >= 3
    return m2, f2


@pytest.mark.parametrize("spp", [1, 2])
def test_frames_see_the_shapes(procedural_region, blue_noise, edited_256, spp):
    u = _u()
    cpu, _ = po.render(*edited_256, blue_noise, u, W, H, spp, 3)
    old, _ = po.render(*procedural_region, blue_noise, u, W, H, spp, 3)
    assert any(not np.array_equal(old[k], cpu[k]) for k in cpu)       # the pose does look at the shapes
    with _ctx(procedural_region, blue_noise, spp=spp, depth=3) as ctx:
        _edit(ctx, _scene_shapes())
        ctx.draw_frame(u)
        ctx.sync()
        _compare(ctx.readback_all(), cpu)


def test_a_pick_through_a_carved_hole_sees_what_lies_behind(procedural_region):
    """A wall across the view, then a hole carved round the centre ray: the pick equals that of a context which was given the
    restatement's world outright, and lies behind the wall."""
    u = _u()
    wall = se.box((40, 40, 180), (160, 42, 255), 0xABCDE, 1)
    hole = se.sphere((2 * 98 + 1, 2 * 41 + 1, 2 * 218 + 1), 21 * 21, 0, 0)
    xy = np.array([(W // 2, H // 2), (W // 2 + 1, H // 2), (3, H - 3)])
    m1, f1 = (a.copy() for a in procedural_region)
    se.apply_shapes(m1, f1, se.batch([wall]))
    m2, f2 = m1.copy(), f1.copy()
    se.apply_shapes(m2, f2, se.batch([hole]))
    with _ctx(procedural_region) as ctx, _ctx((m1, f1)) as walled, _ctx((m2, f2)) as holed:
        _edit(ctx, [wall])
        first = ctx.pick_pixels(u, xy)
        assert first.tobytes() == walled.pick_pixels(u, xy).tobytes()
        assert first["kind"][0] == abi.RT_HIT_SOLID and first["material"][0] == 0xABCDE and 40 <= first["texel"][0][1] <= 42
        _edit(ctx, [hole])
        second = ctx.pick_pixels(u, xy)
        assert second.tobytes() == holed.pick_pixels(u, xy).tobytes()
        assert second["material"][0] != 0xABCDE and (second["kind"][0] != abi.RT_HIT_SOLID or second["distance"][0] > first["distance"][0] + 1)


# ---- ordering ---------------------------------------------------------------------------------------------------------------
def test_frames_in_flight_see_the_region_of_their_call(procedural_region, blue_noise, edited_256):
    u = _u()
    with _ctx(procedural_region, blue_noise, spp=3, depth=2, flags=CACHE | abi.RT_FLAG_FRAMES_IN_FLIGHT_2) as ctx:
        ctx.draw_frame(u)
        first = {b: ctx.device_ptr(b) for b in range(abi.RT_BUF_FINAL_BGRA8)}
        _edit(ctx, _scene_shapes())
        ctx.draw_frame(u)
        assert first != {b: ctx.device_ptr(b) for b in range(abi.RT_BUF_FINAL_BGRA8)}
        ctx.sync()
        second = ctx.readback_all()
        before = _peek(first, W, H)
    _compare(before, po.render(*procedural_region, blue_noise, u, W, H, 3, 2)[0])
    _compare(second, po.render(*edited_256, blue_noise, u, W, H, 3, 2)[0])


def test_caller_stream_orders_shapes_between_frames(procedural_region, blue_noise, edited_256):
    import torch
    import bench
    u = _u()
    s = torch.cuda.Stream(device=0)
    with _ctx(procedural_region, blue_noise, spp=2, depth=2, flags=CACHE) as ctx:
        ctx.set_stream(s.cuda_stream)
        ctx.draw_frame(u)
        first = {}
        for b in range(abi.RT_BUF_FINAL_BGRA8):      # copies enqueued on s before the shapes
            dt, ch = abi.BUFFER_FORMATS[b]
            t = torch.as_tensor(bench._DevArray(ctx.device_ptr(b), W * H * ch * np.dtype(dt).itemsize), device=torch.device("cuda", 0))
            with torch.cuda.stream(s):
                first[b] = t.clone()
        _edit(ctx, _scene_shapes())
        ctx.draw_frame(u)
        ctx.sync()
        s.synchronize()
        second = ctx.readback_all()
        before = {}
        for b, t in first.items():
            dt, ch = abi.BUFFER_FORMATS[b]
            before[abi.BUFFER_NAMES[b]] = t.cpu().numpy().view(dt).reshape((H, W, ch) if ch > 1 else (H, W))
        ctx.set_stream(0)
    _compare(before, po.render(*procedural_region, blue_noise, u, W, H, 2, 2)[0])
    _compare(second, po.render(*edited_256, blue_noise, u, W, H, 2, 2)[0])


def test_shapes_voxel_edits_and_slabs_apply_in_call_order(procedural_region):
    """The three kinds of change across one chunk, each undoing part of the one before: the staging sets are shared and used in turn."""
    mats, mine = procedural_region
    om, of = world.generate_region(world.DEFAULT_SEED + 3)
    m2, f2 = mats.copy(), mine.copy()
    shape1, shape2 = [se.box((64, 64, 64), (127, 127, 100), 0x51, 1)], [se.sphere((200, 200, 190), 40 * 40, 0x52, 0, se.SOLID)]
    xyz = np.stack(np.meshgrid(np.arange(80, 120), np.arange(90, 110), np.arange(70, 100), indexing="ij"), axis=-1).reshape(-1, 3)
    with _ctx(procedural_region) as ctx:
        se.apply_shapes(m2, f2, se.batch(shape1))
        _edit(ctx, shape1)
        ve.apply_edits(m2, f2, xyz, np.full(len(xyz), 0x53, np.uint32), np.zeros(len(xyz), bool))
        ctx.edit_voxels(xyz, np.full(len(xyz), 0x53, np.uint32), np.zeros(len(xyz), bool))
        se.apply_shapes(m2, f2, se.batch(shape2))
        _edit(ctx, shape2)
        m2[:, :, 96:112], f2[:, :, 96:112] = om[:, :, 96:112], of[:, :, 96:112]
        ctx.upload_slice(0, 96, np.ascontiguousarray(om[:, :, 96:112]), np.ascontiguousarray(of[:, :, 96:112]))
        se.apply_shapes(m2, f2, se.batch(shape1))
        _edit(ctx, shape1)
        gm, gf = ctx.read_box((0, 0, 0), (256, 256, 256))
        assert np.array_equal(gf, f2) and np.array_equal(gm, m2)
        assert ctx.selftest(MAPS) == 0


# ---- accumulation and history ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [1, 2])
def test_a_touching_call_restarts_the_accumulation_and_no_other(procedural_region, blue_noise, edited_256, spp):
    seed = 11
    outside = [se.box((256, 0, 0), (300, 9, 9), 1, 1), se.sphere((40, 41, 41), 0, 2, 1)]
    with _ctx(procedural_region, blue_noise, spp=spp, depth=2, flags=CACHE | abi.RT_FLAG_ACCUMULATE) as ctx:
        ctx.draw_frame(_u(seed))
        ctx.draw_frame(_u(seed + spp))
        assert ctx.accumulation() == (2, 2 * spp)
        _edit(ctx, [])                                            # count == 0
        _edit(ctx, outside)                                       # no chunk is touched
        ctx.draw_frame(_u(seed + 2 * spp))
        assert ctx.accumulation() == (3, 3 * spp)
        _edit(ctx, _scene_shapes())
        ctx.draw_frame(_u(seed + 3 * spp))
        assert ctx.accumulation() == (1, spp)
        ctx.sync()
        got = ctx.readback_all()
        _edit(ctx, outside)
        ctx.draw_frame(_u(seed + 4 * spp))
        assert ctx.accumulation() == (2, 2 * spp)
        ctx.sync()
        got2 = ctx.readback_all()
        # a chunk that is touched though nothing in it is selected restarts the sum as well
        _edit(ctx, [se.box((0, 0, 250), (3, 3, 255), 9, 1, se.SOLID)])
        ctx.draw_frame(_u(seed + 5 * spp))
        assert ctx.accumulation() == (1, spp)
    _compare(got, po.render(*edited_256, blue_noise, _u(seed + 3 * spp), W, H, spp, 2)[0])
    _compare(got2, po.render(*edited_256, blue_noise, _u(seed + 3 * spp), W, H, 2 * spp, 2)[0])


def _walk_shapes(ctx, walk, shapes):
    """The shapes on the context and on edit_history_ref's Walk: the restatement's world, and its pending boxes put into the
    history's set by rt_edit_voxels' rule (a call that touches nothing leaves it alone; more than sixteen empty and mark it)."""
    _edit(ctx, shapes)
    if not walk.owned:
        walk.mats, walk.mine, walk.owned = walk.mats.copy(), walk.mine.copy(), True
    se.apply_shapes(walk.mats, walk.mine, se.batch(shapes))
    h, new = walk.h, se.pending_boxes(se.batch(shapes), walk.R)
    if new and h.radius == 0:
        h.valid = False
    elif new and not h.overflowed:
        if len(h.boxes) + len(new) > er.MAX_BOXES:
            h.boxes, h.overflowed = [], True
        else:
            h.boxes += new
    assert ctx.edit_boxes_pending() == h.pending()


# a pillar as a box, a dent beside it as a sphere, and two shapes that leave no box: where the main sequence has its edit
HISTORY_SHAPES = [se.box(er.PILLAR[:3], tuple(o + e - 1 for o, e in zip(er.PILLAR[:3], er.PILLAR[3:])), er.WORD, 1),
                  se.sphere((2 * 104 + 1, 2 * 136 + 1, 2 * 141 + 1), 7 * 7, 0, 0), se.box((256, 0, 0), (260, 5, 5), 1, 1), se.sphere((40, 41, 41), 0, 2, 1)]


def test_a_kept_history_takes_one_box_per_shape(procedural_region, blue_noise):
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, er.RADIUS)
    ops = er.main_ops()
    modes = []
    with _history_ctx(procedural_region, blue_noise) as ctx:
        for k, op in enumerate(ops):
            if op[0] == "edit":
                _walk_shapes(ctx, walk, HISTORY_SHAPES[2:])                     # nothing is touched: nothing waits
                assert ctx.edit_boxes_pending() == (0, False)
                _walk_shapes(ctx, walk, HISTORY_SHAPES)
                assert ctx.edit_boxes_pending() == (2, False)
                lo, hi = walk.h.boxes[1]
                assert lo.tolist() == [101, 133, 138] and hi.tolist() == [107, 139, 144]
            else:
                _history_frame(ctx, walk, op[1], "frame %d" % k)
                modes.append(walk.h.mode)
        assert modes == ["restart", "moved", "moved", "moved", "moved_boxes", "moved", "moved", "still"]
        assert ctx.accumulation() == (8, 8)


def test_seventeen_shapes_overflow_and_the_frame_restarts(procedural_region, blue_noise):
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, er.RADIUS)
    ops = er.frames((0, 1))
    singles = [se.box(p, p, er.WORD, 1) for p in ((90 + 4 * (i % 4), 124 + 4 * (i // 4), 143) for i in range(17))]
    with _history_ctx(procedural_region, blue_noise) as ctx:
        for k, op in enumerate(ops):
            _history_frame(ctx, walk, op[1], "frame %d" % k)
        _walk_shapes(ctx, walk, singles[:10])
        _walk_shapes(ctx, walk, singles[10:16] + HISTORY_SHAPES[2:])
        assert ctx.edit_boxes_pending() == (16, False)
        _history_frame(ctx, walk, er.pose(2, step=2), "sixteen boxes")
        assert walk.h.mode == "moved_boxes"
        _walk_shapes(ctx, walk, singles)
        assert ctx.edit_boxes_pending() == (0, True)
        _walk_shapes(ctx, walk, HISTORY_SHAPES)                                  # (an overflowed set takes no more)
        assert ctx.edit_boxes_pending() == (0, True)
        _history_frame(ctx, walk, er.pose(3, step=3), "after the overflow")
        assert walk.h.mode == "restart" and ctx.accumulation() == (1, 1)


def test_rt_bench_times_a_shape_before_every_frame(native_built):
    """rt_bench --edit-shape: the four edit timing fields of --edits, two launches per call, and the shape's name in the JSON line."""
    import json
    import os
    import subprocess
    from tests.conftest import ROOT
    exe = os.path.join(ROOT, "raytrace_amd", "rt_bench")
    for shape in ("sphere:8", "box:64"):
        r = subprocess.run([exe, "--width", "64", "--height", "64", "--frames", "6", "--edit-shape", shape], cwd=ROOT, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert j["edit_shape"] == shape and j["edits"] == 0 and j["frames"] == 6 and j["edit_launches_per_call"] == 2.0
        assert j["edit_device_ms_per_call"] > 0 and j["edit_wall_ms_per_call"] >= j["edit_host_ms_per_call"] > 0
    bad = subprocess.run([exe, "--edit-shape", "cone:3"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--edit-shape" in bad.stderr


# ---- rejections -------------------------------------------------------------------------------------------------------------
def _bad_shapes(R):
    def spoil(s, **kw):
        s = s.copy()
        for k, v in kw.items():
            s[k] = v
        return s
    bx, sp = se.box((1, 1, 1), (9, 9, 9), 7, 1), se.sphere((21, 21, 21), 49, 7, 1)
    return [spoil(bx, kind=2), spoil(bx, where=3), spoil(sp, reserved=1), spoil(bx, a=(-4 * R - 1, 1, 1)), spoil(sp, a=(21, 4 * R + 1, 21)),
            spoil(bx, b=(9, 9, 4 * R + 1)), spoil(bx, a=(1, 1, -4 * R - 1), b=(9, 9, -4 * R - 1)), spoil(bx, b=(9, 0, 9)),
            spoil(sp, b=(-1, 0, 0)), spoil(sp, b=(2 ** 26 + 1, 0, 0)), spoil(sp, b=(49, 1, 0)), spoil(sp, b=(49, 0, -1))]


def test_rejected_shapes_change_nothing(procedural_region, blue_noise):
    mats, mine = procedural_region
    lib = render._lib.amd()
    good = se.batch([se.box((3, 4, 5), (3, 4, 5), 7, 1), se.sphere((201, 201, 201), 9, 8, 1)])
    ptr = lambda a: a.ctypes.data_as(C.POINTER(abi.RtShapeEdit))
    with render.Context(render.make_config(W, H)) as ctx:
        with pytest.raises(render.RtError) as e:
            ctx.edit_shapes(good)
        assert e.value.code == abi.RT_ERR_NOT_READY
        ctx.edit_shapes(good[:0])                                                # count == 0 asks for nothing, not even a world
    with _history_ctx(procedural_region, blue_noise) as ctx:
        ctx.edit_shapes(good[:1])
        assert ctx.edit_boxes_pending() == (1, False)
        for k, bad in enumerate(_bad_shapes(256)):
            assert not se.valid(bad, 256), k
            for batch in (se.batch([bad]), se.batch([good[1], bad]), se.batch([bad, good[1]])):
                with pytest.raises(render.RtError) as e:
                    ctx.edit_shapes(batch)
                assert e.value.code == abi.RT_ERR_INVALID_ARG, k
        many = np.repeat(good[1:], 4097)
        assert lib.rt_edit_shapes(ctx.handle, ptr(many), 4097) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_edit_shapes(ctx.handle, None, 1) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_edit_shapes(None, ptr(good), 2) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_edit_shapes(ctx.handle, None, 0) == abi.RT_OK
        assert ctx.edit_boxes_pending() == (1, False)
        gm, gf = ctx.read_box((0, 0, 0), (256, 256, 256))
        m2, f2 = mats.copy(), mine.copy()
        se.apply_shapes(m2, f2, good[:1])
        assert np.array_equal(gf, f2) and np.array_equal(gm, m2)
        assert ctx.selftest(MAPS) == 0
        # the limits themselves are accepted: 4096 shapes, coordinates at +-4R, the largest sphere
        edge = se.batch([se.box((-1024, -1024, -1024), (1024, 1024, 0), 5, 1, se.SOLID), se.sphere((1024, -1024, 1024), 2 ** 26, 6, 0, se.AIR)])
        ctx.edit_shapes(np.concatenate([np.repeat(good[1:], 4094), edge]))
        se.apply_shapes(m2, f2, np.concatenate([good[1:], edge]))
        gm, gf = ctx.read_box((0, 0, 0), (256, 256, 256))
        assert np.array_equal(gf, f2) and np.array_equal(gm, m2)
