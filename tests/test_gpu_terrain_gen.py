"""rt_generate_world / rt_generate_slice on the GPU: the region they leave equals the host generator's byte for byte (whole regions,
windows that are not 64-aligned, boxes of a 1024^3 region, streamed slabs of the host manager's move lists), with consistent nibble
maps; frames drawn on it equal frames on the uploaded world; ordering against frames in flight, queries, edits, accumulation and a
caller's stream; rejections; and the Pipeline / Game options built on them."""
import numpy as np
import pytest

from raytrace_amd import abi, render, world
from oracle import pyoracle as po
from tests import voxel_edits as ve
from tests.test_gpu_voxel_edits import RUNS, _host, _peek

pytestmark = pytest.mark.gpu

MAPS = abi.RT_SELFTEST_SCENE_MAPS
CACHE = abi.RT_FLAG_CACHE_PRIMARY
SEEDS = [world.DEFAULT_SEED, 7, 0xC0FFEE0123456789]
W, H = 96, 64


def _u(seed=3, **kw):
    p = dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.25, sun=0.3)
    p.update(kw)
    return po.camera_uniforms(p["origin"], p["heading"], p["pitch"], p["sun"], seed)


def _whole(ctx, R):
    return ctx.read_box((0, 0, 0), (R, R, R))


def _same(got, want, what=""):
    assert np.array_equal(got[1], want[1]), "minefield differs at %d voxels %s" % (int(np.count_nonzero(got[1] != want[1])), what)
    assert np.array_equal(got[0], want[0]), "materials differ at %d voxels %s" % (int(np.count_nonzero(got[0] != want[0])), what)


@pytest.mark.parametrize("R", [256, 512])
def test_whole_region_equals_the_host_generator(R, native_built):
    with render.Context(render.make_config(64, 64, region=R)) as ctx:
        for seed in SEEDS:
            ctx.generate_world(seed)
            _same(_whole(ctx, R), world.generate_region(seed, region=R), "seed %#x" % seed)
            assert ctx.selftest(MAPS) == 0


@pytest.mark.parametrize("R,lo", [(256, (-112, 48, -144)), (256, (16, -208, 80)), (512, (-240, 112, -304)), (512, (1008, -48, 16))])
def test_unaligned_windows_equal_the_toroidal_region(R, lo, native_built):
    with render.Context(render.make_config(64, 64, region=R)) as ctx:
        ctx.generate_world(world.DEFAULT_SEED, lo)
        _same(_whole(ctx, R), world.toroidal_region(tuple(v + R // 2 for v in lo), region=R), str(lo))
        assert ctx.selftest(MAPS) == 0


def test_region_1024_boxes_and_maps(native_built):
    R = 1024
    cs = world.ChunkStorage("", world.DEFAULT_SEED)
    with render.Context(render.make_config(64, 64, region=R)) as ctx:
        ctx.generate_world(world.DEFAULT_SEED)
        assert ctx.selftest(MAPS) == 0
        # world chunks (texel = world + 512): corners, surface chunks, a deep one and the all-air top
        for c in [(-8, -8, -8), (7, 7, 7), (0, 0, 0), (-1, 3, 1), (5, -6, 2), (2, 2, -1), (-8, 7, 0), (7, -8, 1)]:
            m, f = cs.borrow_packed_chunk_data(*c)
            got = ctx.read_box(tuple(64 * v + 512 for v in c), (64, 64, 64))
            _same(got, (m, f), str(c))
    cs.close()
    # a window across a 64-block edge on every axis, its box across the texel wrap
    lo = (-496, 16, -528)
    with render.Context(render.make_config(64, 64, region=R)) as ctx:
        ctx.generate_world(world.DEFAULT_SEED, lo)
        assert ctx.selftest(MAPS) == 0
        t0 = (1000, 480, 0)
        got = ctx.read_box(t0, (24, 64, 40))
        t = [np.arange(t0[a], t0[a] + (24, 64, 40)[a]) for a in range(3)]
        v = [lo[a] + ((t[a] - lo[a] - 512) % R) for a in range(3)]
        want = (np.zeros((40, 64, 24), np.uint32), np.zeros((40, 64, 24), np.uint8))
        cs = world.ChunkStorage("", world.DEFAULT_SEED)
        for cz in np.unique(v[2] // 64):
            for cy in np.unique(v[1] // 64):
                for cx in np.unique(v[0] // 64):
                    m, f = cs.borrow_packed_chunk_data(cx, cy, cz)
                    sel = [np.nonzero(v[a] // 64 == c)[0] for a, c in enumerate((cx, cy, cz))]
                    loc = np.ix_(*[v[a][sel[a]] % 64 for a in (2, 1, 0)])
                    want[0][np.ix_(sel[2], sel[1], sel[0])] = m[loc]
                    want[1][np.ix_(sel[2], sel[1], sel[0])] = f[loc]
        _same(got, want, "box across the wrap")
        cs.close()


MOVES = [
    (256, [(0, 1)] * 3),
    (256, [(1, 0)] * 2),
    (256, [(0, 1)] * 17),
    (256, [(0, 1), (2, 1), (0, 1), (1, 0), (2, 0), (0, 0)]),
    (512, [(0, 1)] * 2 + [(2, 0)] * 3 + [(1, 1)] * 33),    # +y past a whole region: across the wrap
]


@pytest.mark.parametrize("R,moves", MOVES)
def test_slices_replay_the_host_manager(R, moves, native_built):
    t = world.HostTerrainUploadManager(region=R)
    with render.Context(render.make_config(64, 64, region=R)) as ctx:
        ctx.generate_world(world.DEFAULT_SEED)
        for axis, inc in moves:
            (t.request_increase if inc else t.request_decrease)(axis)
        while t.pending():
            axis, lo = t.next_window()
            ctx.generate_slice(world.DEFAULT_SEED, axis, lo)
            t.setup_next_request()
        _same(_whole(ctx, R), t.region())
        assert ctx.selftest(MAPS) == 0
    t.close()


@pytest.mark.parametrize("kernel,flags", RUNS + [(abi.RT_KERNEL_DEFAULT, CACHE | abi.RT_FLAG_ACCUMULATE)])
def test_frames_on_a_generated_world_equal_frames_on_the_uploaded_one(procedural_region, blue_noise, kernel, flags):
    spp, depth = 2, 3
    out = []
    for gen in (False, True):
        with render.Context(render.make_config(W, H, spp=spp, depth=depth, kernel=kernel, flags=flags)) as ctx:
            if gen:
                ctx.generate_world(world.DEFAULT_SEED)
            else:
                ctx.upload_world(*procedural_region)
            ctx.upload_noise(blue_noise)
            for s in (3, 5):
                ctx.draw_frame(_u(s))
            ctx.sync()
            out.append((ctx.readback_all(), ctx.counters().as_dict() if flags & abi.RT_FLAG_COUNTERS else None))
    (a, ca), (b, cb) = out
    for name in a:
        assert np.array_equal(a[name], b[name], equal_nan=True), name
    assert ca == cb


@pytest.mark.parametrize("R,frames,camera,want", [
    (256, 5, (60, -100, 70, 1.6, -0.2, 0.3), [(16, 0, 0), (32, 0, 0), (48, 0, 0), (48, 0, 16), (48, 0, 32)]),
    (512, 3, (120, -200, 140, 1.6, -0.2, 0.3), [(16, 0, 0), (32, 0, 0), (48, 0, 0)]),
])
def test_pipeline_streams_on_the_device(blue_noise, R, frames, camera, want):
    g = render.Game(args=camera)
    g.use_device_world(world.DEFAULT_SEED, region=R)
    cfg = render.make_config(64, 48, spp=1, depth=2, region=R)
    p = render.create_instance(cfg, g, blue_noise)
    p.enable_terrain_streaming(world.DEFAULT_SEED, on_device=True)
    seen = []
    for frame in range(frames):
        p.draw_frame(g)
        p.wait()
        u = p.uniforms()
        seen.append(tuple(u.lr))
        mats, mine = world.toroidal_region(tuple(u.lr), region=R)
        cpu, _ = po.render(mats, mine, blue_noise, u, 64, 48, 1, 2, region=R)
        gpu = p.context.readback_all()
        for name in cpu:
            assert np.array_equal(gpu[name], cpu[name], equal_nan=True), (frame, name)
    assert seen == want
    p.close()
    g.close()


def test_game_device_world_draws_the_generated_world(blue_noise):
    frames = []
    for device in (False, True):
        g = render.Game(args=(-30, -128, 100, 1.5707964, -0.25, 0.3))
        (g.use_device_world if device else g.generate_world)(world.DEFAULT_SEED + 1, region=256)
        p = render.create_instance(render.make_config(64, 48, spp=2, depth=2), g, blue_noise)
        p.draw_frame(g)
        p.wait()
        frames.append(p.context.readback_all())
        p.close()
        g.close()
    for name in frames[0]:
        assert np.array_equal(frames[0][name], frames[1][name], equal_nan=True), name


# ---- ordering ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def other_world(native_built):
    return world.generate_region(world.DEFAULT_SEED + 3)


def test_frames_in_flight_see_the_world_of_their_call(procedural_region, other_world, blue_noise):
    spp, depth = 3, 2
    u = _u()
    with render.Context(render.make_config(W, H, spp=spp, depth=depth, flags=CACHE | abi.RT_FLAG_FRAMES_IN_FLIGHT_2)) as ctx:
        ctx.upload_world(*procedural_region)
        ctx.upload_noise(blue_noise)
        ctx.draw_frame(u)
        first = {b: ctx.device_ptr(b) for b in range(abi.RT_BUF_FINAL_BGRA8)}
        ctx.generate_world(world.DEFAULT_SEED + 3)
        ctx.draw_frame(u)
        ctx.sync()
        second = ctx.readback_all()
        before = _host(_peek(first))
    for got, region in ((before, procedural_region), (second, other_world)):
        cpu = po.render(*region, blue_noise, u, W, H, spp, depth)[0]
        for name in cpu:
            assert np.array_equal(got[name], cpu[name], equal_nan=True), name


def test_query_before_edit_after_and_accumulation(procedural_region, other_world, blue_noise):
    import torch
    rng = np.random.default_rng(5)
    n = 4096
    o = np.column_stack([rng.uniform(-100, 100, n), rng.uniform(-100, 100, n), rng.uniform(20, 160, n)]).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7] = o, d
    with render.Context(render.make_config(W, H, spp=1, depth=2, flags=CACHE | abi.RT_FLAG_ACCUMULATE)) as ctx:
        ctx.generate_world(world.DEFAULT_SEED)
        ctx.upload_noise(blue_noise)
        want_old = ctx.trace_rays(o, d)
        dev_rays = torch.from_numpy(rays).cuda()
        hits = torch.zeros((n, 12), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.trace_rays_async(dev_rays, hits)
        ctx.generate_world(world.DEFAULT_SEED + 3)
        ctx.sync()
        got = hits.cpu().numpy()
        assert np.array_equal(got.view(np.uint8).reshape(n, 48), np.ascontiguousarray(want_old).view(np.uint8).reshape(n, 48))
        # edits apply on top of the generated world
        m2, f2 = other_world[0].copy(), other_world[1].copy()
        xyz = rng.integers(0, 256, size=(2000, 3))
        words = rng.integers(1, 2 ** 21, len(xyz), dtype=np.uint64).astype(np.uint32)
        solid = rng.random(len(xyz)) < 0.5
        ve.apply_edits(m2, f2, xyz, words, solid)
        ctx.edit_voxels(xyz, words, solid)
        _same(_whole(ctx, 256), (m2, f2))
        assert ctx.selftest(MAPS) == 0
        # accumulation restarts after a generate
        ctx.draw_frame(_u(11))
        ctx.draw_frame(_u(12))
        assert ctx.accumulation() == (2, 2)
        ctx.generate_world(world.DEFAULT_SEED)
        ctx.draw_frame(_u(13))
        assert ctx.accumulation() == (1, 1)
        ctx.sync()
        got = ctx.readback_all()
    cpu = po.render(*procedural_region, blue_noise, _u(13), W, H, 1, 2)[0]
    for name in cpu:
        assert np.array_equal(got[name], cpu[name], equal_nan=True), name


def test_caller_stream_orders_generates_between_frames(procedural_region, other_world, blue_noise):
    import torch
    u = _u()
    s = torch.cuda.Stream(device=0)
    with render.Context(render.make_config(W, H, spp=2, depth=2, flags=CACHE)) as ctx:
        ctx.set_stream(s.cuda_stream)
        ctx.generate_world(world.DEFAULT_SEED)
        ctx.upload_noise(blue_noise)
        ctx.draw_frame(u)
        first = _peek({b: ctx.device_ptr(b) for b in range(abi.RT_BUF_FINAL_BGRA8)}, stream=s)
        ctx.generate_world(world.DEFAULT_SEED + 3)
        ctx.draw_frame(u)
        ctx.sync()
        s.synchronize()
        second = ctx.readback_all()
        before = _host(first)
        ctx.set_stream(0)
    for got, region in ((before, procedural_region), (second, other_world)):
        cpu = po.render(*region, blue_noise, u, W, H, 2, 2)[0]
        for name in cpu:
            assert np.array_equal(got[name], cpu[name], equal_nan=True), name


def test_rejections_change_nothing(procedural_region, native_built):
    with render.Context(render.make_config(64, 64)) as ctx:
        with pytest.raises(render.RtError) as e:
            ctx.generate_slice(world.DEFAULT_SEED, 0, (-128, -128, -128))
        assert e.value.code == abi.RT_ERR_NOT_READY
        ctx.upload_world(*procedural_region)
        probe = ctx.read_box((64, 32, 0), (96, 80, 128))
        for call in (lambda: ctx.generate_slice(world.DEFAULT_SEED, 3, (0, 0, 0)),
                     lambda: ctx.generate_slice(world.DEFAULT_SEED, -1, (0, 0, 0)),
                     lambda: ctx.generate_slice(world.DEFAULT_SEED, 1, (8, 0, 0)),
                     lambda: ctx.generate_world(world.DEFAULT_SEED, (0, -136, 0)),
                     lambda: ctx.generate_world(world.DEFAULT_SEED, (2 ** 31 - 240, 0, 0)),
                     lambda: ctx.generate_world(world.DEFAULT_SEED, (0, 0, -2 ** 31 - 16)),
                     lambda: ctx.generate_slice(world.DEFAULT_SEED, 2, (0, 0, 2 ** 31 - 8)),
                     lambda: ctx.generate_slice(world.DEFAULT_SEED, 0, (0, 2 ** 31 - 240, 0))):
            with pytest.raises(render.RtError) as e:
                call()
            assert e.value.code == abi.RT_ERR_INVALID_ARG
        got = ctx.read_box((64, 32, 0), (96, 80, 128))
        _same(got, probe)
        assert ctx.selftest(MAPS) == 0
        # the edges of the int32 range are accepted
        ctx.generate_world(world.DEFAULT_SEED, (2 ** 31 - 256, -2 ** 31, 0))
        assert ctx.selftest(MAPS) == 0
        # ... and hold the host's terrain there: the surface chunk in the corner, which ends at 2^31 in x and starts at -2^31 in y
        c = (2 ** 25 - 1, -2 ** 25, 0)
        cs = world.ChunkStorage("", world.DEFAULT_SEED)
        want = cs.borrow_packed_chunk_data(*c)
        cs.close()
        assert (want[1] == 0).any() and (want[1] != 0).any()
        _same(ctx.read_box(tuple((64 * v + 128) % 256 for v in c), (64, 64, 64)), want, "chunk %s" % (c,))
