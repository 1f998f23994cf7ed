"""rt_edit_voxels on the GPU, against the numpy restatement of tests/voxel_edits.py and the oracle: the resident region byte for
byte (rt_read_box) and the nibble maps (RT_SELFTEST_SCENE_MAPS) after edit batches at R = 256, 512 and 1024; frames of every kernel
on the edited world; stream ordering against frames in flight, slabs and a caller's stream; the accumulation reset; rejections."""
import ctypes as C

import numpy as np
import pytest

from raytrace_amd import abi, render, world
from oracle import pyoracle as po
from tests import voxel_edits as ve
from tests.test_gpu_parity import _cached_counters, _compare

pytestmark = pytest.mark.gpu

MAPS = abi.RT_SELFTEST_SCENE_MAPS
CNT, CACHE = abi.RT_FLAG_COUNTERS, abi.RT_FLAG_CACHE_PRIMARY
POSE = dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.25, sun=0.3)
W, H = 96, 64


def _u(seed=3, **kw):
    p = dict(POSE)
    p.update(kw)
    return po.camera_uniforms(p["origin"], p["heading"], p["pitch"], p["sun"], seed)


def _ctx(region, noise=None, R=256, W=64, H=64, **kw):
    ctx = render.Context(render.make_config(W, H, region=R, **kw))
    ctx.upload_world(*region)
    if noise is not None:
        ctx.upload_noise(noise)
    return ctx


def _batches(R, rng):
    """(name, xyz, words, solid) batches of the region-bytes test."""
    out = []
    corners = [(x, y, z) for x in (0, 63, 64, R - 1) for y in (0, 64, R - 64) for z in (0, 127, R - 1)]
    faces = [(0, R // 2, 77), (R - 1, 3, R // 3), (50, 0, 9), (11, R - 1, 200 % R), (130 % R, 17, 0), (R // 2 + 1, R - 2, R - 1)]
    pts = np.array(corners + faces)
    out.append(("corners and faces", pts, rng.integers(0, 2 ** 32, len(pts), dtype=np.uint64), rng.random(len(pts)) < 0.5))
    z, y, x = np.mgrid[0:64, 0:64, 0:64]
    cube = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    emptied = cube + (64, 64, 0)
    filled = cube + (R - 128, 0, 64)
    out.append(("emptied and filled chunks", np.concatenate([emptied, filled]),
                np.concatenate([np.zeros(len(cube), np.uint64), np.full(len(cube), 0x12345, np.uint64)]),
                np.concatenate([np.zeros(len(cube), bool), np.ones(len(cube), bool)])))
    dup = np.array([(7, 9, 11)] * 5 + [(70, 9, 11)] * 4 + [(7, 9, 11)])
    out.append(("duplicates", dup, np.arange(10, dtype=np.uint64) + 100, np.array([1, 0, 1, 1, 0, 0, 1, 1, 0, 1], bool)))
    pts = rng.integers(0, R, size=(100000, 3))
    out.append(("1e5 random", pts, rng.integers(0, 2 ** 32, len(pts), dtype=np.uint64), rng.random(len(pts)) < 0.3))
    return out


@pytest.mark.parametrize("R", [256, 512])
def test_region_bytes_and_maps_after_edit_batches(R, native_built):
    rng = np.random.default_rng(R)
    mats, mine = world.generate_region(world.DEFAULT_SEED, region=R)
    mats, mine = mats.copy(), mine.copy()
    with _ctx((mats, mine), R=R) as ctx:
        assert ctx.selftest(MAPS) == 0
        for name, xyz, words, solid in _batches(R, rng):
            ve.apply_edits(mats, mine, xyz, words.astype(np.uint32), solid)
            ctx.edit_voxels(xyz, words.astype(np.uint32), solid)
            gm, gf = ctx.read_box((0, 0, 0), (R, R, R))
            assert np.array_equal(gf, mine), "%s: minefield differs at %d voxels" % (name, int(np.count_nonzero(gf != mine)))
            assert np.array_equal(gm, mats), "%s: materials differ at %d voxels" % (name, int(np.count_nonzero(gm != mats)))
            assert ctx.selftest(MAPS) == 0, name


def test_region_bytes_at_1024_and_a_shared_coarse_word(native_built):
    """At R = 1024 a coarse nibble-map word (8 cubes of 16^3) spans two chunks along x: chunks 2 and 3 share theirs.  The region is
    empty (minefield 6) except for arbitrary values 0..30 in the chunks the test reads."""
    R = 1024
    rng = np.random.default_rng(1024)
    mats = np.zeros((R, R, R), np.uint32)
    mine = np.full((R, R, R), 6, np.uint8)
    y0, z0 = 320, 448
    box = (slice(z0, z0 + 64), slice(y0, y0 + 64), slice(64, 384))             # chunks x = 1..5 of one row
    mine[box] = rng.integers(0, 31, size=mine[box].shape, dtype=np.uint8)
    mine[z0:z0 + 64, y0:y0 + 64, 192:256] = 0                                   # chunk 3 full
    mats[box] = rng.integers(0, 2 ** 32, size=mats[box].shape, dtype=np.uint64).astype(np.uint32)
    with _ctx((mats, mine), R=R) as ctx:
        assert ctx.selftest(MAPS) == 0
        batches = [np.array([(128, y0, z0), (255, y0 + 63, z0 + 63), (200, y0 + 5, z0 + 6)]),   # chunk 2 and 3 (shared word)
                   rng.integers(0, 64, size=(20000, 3)) + (128, y0, z0),
                   rng.integers(0, 64, size=(20000, 3)) + (192, y0, z0),
                   np.array([(1023, 1023, 1023), (0, 0, 0), (1023, 0, 512)])]
        for k, xyz in enumerate(batches):
            words = rng.integers(0, 2 ** 32, len(xyz), dtype=np.uint64).astype(np.uint32)
            solid = rng.random(len(xyz)) < (0.9 if k == 2 else 0.4)
            ve.apply_edits(mats, mine, xyz, words, solid)
            ctx.edit_voxels(xyz, words, solid)
            gm, gf = ctx.read_box((64, y0, z0), (320, 64, 64))                 # touched chunks 2, 3 and untouched 1, 4, 5
            assert np.array_equal(gf, mine[box]) and np.array_equal(gm, mats[box]), k
            for c in [(0, 0, 0), (R - 64, R - 64, R - 64), (R - 64, 0, 512)]:
                gm, gf = ctx.read_box(c, (64, 64, 64))
                sl = (slice(c[2], c[2] + 64), slice(c[1], c[1] + 64), slice(c[0], c[0] + 64))
                assert np.array_equal(gf, mine[sl]) and np.array_equal(gm, mats[sl]), (k, c)
            assert ctx.selftest(MAPS) == 0, k


def _scene_edits(R=256):
    """A wall of blocks in front of the default camera, a hole in the ground below it and a floating slab: edits the frames see."""
    h = R // 2
    pts, solid = [], []
    for z in range(h + 95, h + 110):
        for x in range(h - 40, h - 20):
            pts.append((x, h - 90, z))
            solid.append(True)
    for z in range(h - 5, h + 95):
        for y in range(h - 70, h - 50):
            for x in range(h - 40, h - 10, 3):
                pts.append((x, y, z))
                solid.append(False)
    for x in range(h - 60, h):
        for y in range(h - 120, h - 100):
            pts.append((x, y, h + 120))
            solid.append(True)
    words = [po.lib().rt_oracle_pack_material(40 + (i % 50), 120, 100 - (i % 70), 0) for i in range(len(pts))]
    return np.array(pts), np.array(words, np.uint32), np.array(solid)


@pytest.fixture(scope="module")
def edited_256(procedural_region):
    mats, mine = procedural_region
    m2, f2 = mats.copy(), mine.copy()
    xyz, words, solid = _scene_edits()
    touched = ve.apply_edits(m2, f2, xyz, words, solid)
    assert len(touched) >= 3
    return (xyz, words, solid), (m2, f2)


RUNS = [(abi.RT_KERNEL_DEFAULT, CNT), (abi.RT_KERNEL_FRAME, CACHE | CNT), (abi.RT_KERNEL_PATHS, CACHE | CNT),
        (abi.RT_KERNEL_PERSISTENT, CNT), (abi.RT_KERNEL_MEGA, CNT), (abi.RT_KERNEL_WAVEFRONT, CNT)]


@pytest.mark.parametrize("kernel,flags", RUNS)
def test_frames_of_every_kernel_see_the_edits(procedural_region, blue_noise, edited_256, kernel, flags):
    (xyz, words, solid), (m2, f2) = edited_256
    spp, depth = 2, 3
    u = _u()
    cpu, ccn = po.render(m2, f2, blue_noise, u, W, H, spp, depth)
    old, _ = po.render(*procedural_region, blue_noise, u, W, H, spp, depth)
    assert any(not np.array_equal(old[k], cpu[k]) for k in cpu)       # the pose does look at the edits
    with _ctx(procedural_region, blue_noise, W=W, H=H, spp=spp, depth=depth, kernel=kernel, flags=flags) as ctx:
        ctx.edit_voxels(xyz, words, solid)
        ctx.draw_frame(u)
        ctx.sync()
        gpu, gcn = ctx.readback_all(), ctx.counters()
    _compare(gpu, cpu)
    want = _cached_counters(m2, f2, blue_noise, u, W, H, spp, depth, ccn) if flags & CACHE else ccn.as_dict()
    assert gcn.as_dict() == want


def _peek(ptrs, stream=None):
    """Copies of the planes behind device pointers (enqueued on `stream` when given, so ordered against the context's work there)."""
    import torch
    import bench
    out = {}
    for b, ptr in ptrs.items():
        dt, ch = abi.BUFFER_FORMATS[b]
        n = W * H * ch * np.dtype(dt).itemsize
        t = torch.as_tensor(bench._DevArray(ptr, n), device=torch.device("cuda", 0))
        if stream is not None:
            with torch.cuda.stream(stream):
                t = t.clone()
        out[abi.BUFFER_NAMES[b]] = t
    return out


def _host(planes):
    out = {}
    for b, name in abi.BUFFER_NAMES.items():
        if name in planes:
            dt, ch = abi.BUFFER_FORMATS[b]
            out[name] = planes[name].cpu().numpy().view(dt).reshape((H, W, ch) if ch > 1 else (H, W))
    return out


@pytest.mark.parametrize("kernel", [abi.RT_KERNEL_DEFAULT, abi.RT_KERNEL_PATHS, abi.RT_KERNEL_PERSISTENT])
def test_frames_in_flight_see_the_region_of_their_call(procedural_region, blue_noise, edited_256, kernel):
    (xyz, words, solid), (m2, f2) = edited_256
    spp, depth = 3, 2
    u = _u()
    with _ctx(procedural_region, blue_noise, W=W, H=H, spp=spp, depth=depth, kernel=kernel,
              flags=CACHE | abi.RT_FLAG_FRAMES_IN_FLIGHT_2) as ctx:
        ctx.draw_frame(u)
        first = {b: ctx.device_ptr(b) for b in range(abi.RT_BUF_FINAL_BGRA8)}
        ctx.edit_voxels(xyz, words, solid)
        ctx.draw_frame(u)
        ctx.sync()
        second = ctx.readback_all()
        before = _host(_peek(first))
    _compare(before, po.render(*procedural_region, blue_noise, u, W, H, spp, depth)[0])
    _compare(second, po.render(m2, f2, blue_noise, u, W, H, spp, depth)[0])


def test_slab_edit_slab_apply_in_call_order(procedural_region, blue_noise):
    """Slab (z 64..79), then edits inside that slab and chunk, then a slab across the same chunk (x 96..111) that overwrites part
    of the edits: the region and the frame are those of the three changes applied in call order."""
    mats, mine = procedural_region
    om, of = world.generate_region(world.DEFAULT_SEED + 3)
    m2, f2 = mats.copy(), mine.copy()
    rng = np.random.default_rng(4)
    xyz = rng.integers(0, 16, size=(3000, 3)) * (5, 5, 1) % 64 + (64, 64, 64)
    words = rng.integers(1, 2 ** 21, len(xyz), dtype=np.uint64).astype(np.uint32)
    solid = rng.random(len(xyz)) < 0.6
    u = _u(origin=(-20.0, -100.0, 40.0), pitch=-0.4)
    with _ctx(procedural_region, blue_noise, W=W, H=H, spp=2, depth=2, flags=CACHE | abi.RT_FLAG_FRAMES_IN_FLIGHT_2) as ctx:
        ctx.draw_frame(u)
        m2[64:80], f2[64:80] = om[64:80], of[64:80]
        ctx.upload_slice(2, 64, np.ascontiguousarray(om[64:80]), np.ascontiguousarray(of[64:80]))
        ve.apply_edits(m2, f2, xyz, words, solid)
        ctx.edit_voxels(xyz, words, solid)
        m2[:, :, 96:112], f2[:, :, 96:112] = om[:, :, 96:112], of[:, :, 96:112]
        ctx.upload_slice(0, 96, np.ascontiguousarray(om[:, :, 96:112]), np.ascontiguousarray(of[:, :, 96:112]))
        ctx.draw_frame(u)
        ctx.sync()
        got = ctx.readback_all()
        gm, gf = ctx.read_box((0, 0, 0), (256, 256, 256))
        assert np.array_equal(gf, f2) and np.array_equal(gm, m2)
        assert ctx.selftest(MAPS) == 0
    _compare(got, po.render(m2, f2, blue_noise, u, W, H, 2, 2)[0])


def test_caller_stream_orders_edits_between_frames(procedural_region, blue_noise, edited_256):
    import torch
    (xyz, words, solid), (m2, f2) = edited_256
    u = _u()
    s = torch.cuda.Stream(device=0)
    with _ctx(procedural_region, blue_noise, W=W, H=H, spp=2, depth=2, flags=CACHE) as ctx:
        ctx.set_stream(s.cuda_stream)
        ctx.draw_frame(u)
        first = _peek({b: ctx.device_ptr(b) for b in range(abi.RT_BUF_FINAL_BGRA8)}, stream=s)   # copies enqueued on s before the edit
        ctx.edit_voxels(xyz, words, solid)
        ctx.draw_frame(u)
        ctx.sync()
        s.synchronize()
        second = ctx.readback_all()
        before = _host(first)
        ctx.set_stream(0)
    _compare(before, po.render(*procedural_region, blue_noise, u, W, H, 2, 2)[0])
    _compare(second, po.render(m2, f2, blue_noise, u, W, H, 2, 2)[0])


@pytest.mark.parametrize("spp", [1, 2])
def test_an_edit_restarts_the_accumulation(procedural_region, blue_noise, edited_256, spp):
    (xyz, words, solid), (m2, f2) = edited_256
    seed = 11
    with _ctx(procedural_region, blue_noise, W=W, H=H, spp=spp, depth=2, flags=CACHE | abi.RT_FLAG_ACCUMULATE) as ctx:
        ctx.draw_frame(_u(seed))
        ctx.draw_frame(_u(seed + spp))
        assert ctx.accumulation() == (2, 2 * spp)
        ctx.edit_voxels(np.zeros((0, 3), int), [], [])          # count == 0: no reset
        ctx.draw_frame(_u(seed + 2 * spp))
        assert ctx.accumulation() == (3, 3 * spp)
        ctx.edit_voxels(xyz, words, solid)
        ctx.draw_frame(_u(seed + 3 * spp))
        assert ctx.accumulation() == (1, spp)
        ctx.sync()
        got = ctx.readback_all()
        ctx.edit_voxels(np.zeros((0, 3), int), [], [])
        ctx.draw_frame(_u(seed + 4 * spp))
        assert ctx.accumulation() == (2, 2 * spp)
        ctx.sync()
        got2 = ctx.readback_all()
    _compare(got, po.render(m2, f2, blue_noise, _u(seed + 3 * spp), W, H, spp, 2)[0])
    _compare(got2, po.render(m2, f2, blue_noise, _u(seed + 3 * spp), W, H, 2 * spp, 2)[0])


def test_rejected_edits_change_nothing(procedural_region, native_built):
    mats, mine = procedural_region
    lib = render._lib.amd()
    with render.Context(render.make_config(64, 64)) as ctx:
        with pytest.raises(render.RtError) as e:
            ctx.edit_voxels([(1, 2, 3)], [5], [1])
        assert e.value.code == abi.RT_ERR_NOT_READY
        with pytest.raises(render.RtError) as e:
            ctx.read_box((0, 0, 0), (1, 1, 1))
        assert e.value.code == abi.RT_ERR_NOT_READY
        ctx.upload_world(mats, mine)
        good = ve.edit_records([(3, 4, 5), (100, 100, 100)], [7, 8], [1, 1])
        for bad in (ve.edit_records([(3, 4, 5), (256, 0, 0)], [7, 8], [1, 1]),
                    ve.edit_records([(3, 4, 5), (0, 0, 300)], [7, 8], [1, 1]),
                    ve.edit_records([(3, 4, 5), (10, 10, 10)], [7, 8], [1, 1], reserved=[0, 1])):
            with pytest.raises(render.RtError) as e:
                ctx.edit_records(bad)
            assert e.value.code == abi.RT_ERR_INVALID_ARG
        # count above 2^24 is refused before the records are read
        assert lib.rt_edit_voxels(ctx.handle, good.ctypes.data_as(C.POINTER(abi.RtVoxelEdit)), (1 << 24) + 1) == abi.RT_ERR_INVALID_ARG
        for origin, extent in (((0, 0, 0), (257, 1, 1)), ((-1, 0, 0), (1, 1, 1)), ((255, 255, 255), (1, 2, 1)), ((0, 0, 0), (0, 1, 1))):
            with pytest.raises(render.RtError) as e:
                ctx.read_box(origin, extent)
            assert e.value.code == abi.RT_ERR_INVALID_ARG
        gm, gf = ctx.read_box((0, 0, 0), (256, 256, 256))
        assert np.array_equal(gf, mine) and np.array_equal(gm, mats)
        assert ctx.selftest(MAPS) == 0
        before = ctx.info().device_bytes
        ctx.edit_records(good)
        assert ctx.info().device_bytes == before + (64 << 10)   # the first batch's staging set (64 KiB at least) counts
        ctx.edit_records(good)
        gm, gf = ctx.read_box((0, 0, 0), (64, 64, 64))
        assert gm[5, 4, 3] == 7 and gf[5, 4, 3] == 0
