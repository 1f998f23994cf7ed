"""Ray queries on the GPU (rt_trace_rays, rt_trace_rays_async, rt_pick_pixels): every RtRayHit field against the oracle's trace_ray
on adversarial rays and worlds and on batches of every size, picks against the planes of frames drawn by the oracle and by every kernel, the
pick -> edit loop, the absence of side effects on accumulating frames, and the rejections."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from raytrace_amd import abi, render, world
from tests import adversarial_worlds as aw
from tests import ray_query_ref as rq
from tests.shader_trace import length3
from tests.test_ray_query_contract import assert_float_bits, oracle_kind, seeded_rays

pytestmark = pytest.mark.gpu

def _ctx(mats, mine, W=64, H=40, R=256, noise=None, **kw):
    """A context with the region resident."""
    ctx = render.Context(render.make_config(W, H, region=R, **kw))
    ctx.upload_world(mats, mine)
    if noise is not None:
        ctx.upload_noise(noise)
    return ctx


def _oracle_check(mats, mine, o, d, hits, lr, idx):
    """hits[idx] against pyoracle.trace_ray, every field; the texel holds the material word on solid hits."""
    m3, f3 = mats.reshape(256, 256, 256), mine.reshape(256, 256, 256)
    for i in idx:
        h, g = po.trace_ray(mats, mine, o[i], d[i], lr), hits[i]
        assert_float_bits(g["position"], h.position[:])
        assert_float_bits(g["distance"], h.distance)
        assert (int(g["normal"]), int(g["kind"]), int(g["material"]), int(g["iterations"]), int(g["border_fetches"])) == (
            h.normal, oracle_kind(h), h.packed_material, h.iterations, h.border_fetches), (i, o[i], d[i])
        t = tuple(int(v) for v in g["texel"])
        if g["kind"] == abi.RT_HIT_SOLID and t != (-1, -1, -1):
            assert m3[t[2], t[1], t[0]] == g["material"] and f3[t[2], t[1], t[0]] == 0
        else:
            assert t == (-1, -1, -1) and g["material"] == 0


def _adversarial_rays(rng, mats, mine, lr, n, R=256):
    o, d = seeded_rays(rng, n, R)
    o += np.float32(lr)
    # origins inside solid voxels, rays grazing voxel edges and corners, axis-aligned rays on integer planes
    if R == 256:
        solid = np.argwhere(mine.reshape(256, 256, 256) == 0)
    else:   # (the larger regions: solid voxels among seeded texels, not a list of every one)
        t = rng.integers(0, R, (1 << 16, 3))
        solid = t[mine.reshape(R, R, R)[t[:, 0], t[:, 1], t[:, 2]] == 0]
    pick = solid[rng.integers(0, len(solid), 32)][:, ::-1] - R // 2 + np.float32(lr)
    o[-32:] = pick + np.float32(0.25)
    g = (rng.integers(-100, 100, (32, 3)) * (R // 256)).astype(np.float32) + np.float32(lr)
    o[-64:-32] = g
    d[-64:-48] = np.float32([1, 1, 0])
    d[-48:-32] = np.float32([1, -1, 1])
    return o, d


WORLDS = ["procedural", "scrolled", "limit", "arbitrary"]


def _world(name, procedural_region):
    if name == "procedural":
        return procedural_region + ((0, 0, 0),)
    if name == "scrolled":
        lr = (48, 0, 32)
        return world.toroidal_region(lr) + (lr,)
    if name == "limit":
        lr = (2048, 0, 0)
        return world.toroidal_region(lr) + (lr,)
    mats, mine, _, _ = aw.arbitrary_world(256, seed=3)
    return mats.reshape(-1), mine.reshape(-1), (0, 0, 0)


@pytest.mark.parametrize("name", WORLDS)
def test_arbitrary_rays_match_the_oracle(name, procedural_region):
    mats, mine, lr = _world(name, procedural_region)
    rng = np.random.default_rng(17)
    o, d = _adversarial_rays(rng, mats, mine, lr, 1500)
    if name == "limit":
        o[:600] = np.float32((lr[0] - 30.0, -128.0, 100.0)) + rng.uniform(-4, 4, (600, 3)).astype(np.float32)
        d[:600, 2] = -np.abs(d[:600, 2]) - np.float32(0.2)
    with _ctx(mats, mine) as ctx:
        hits = ctx.trace_rays(o, d, lr)
    _oracle_check(mats, mine, o, d, hits, lr, range(len(o)))
    if name == "limit":
        assert np.count_nonzero(hits["kind"] == abi.RT_HIT_LIMIT) > 0
    m3, f3 = mats.reshape(256, 256, 256), mine.reshape(256, 256, 256)
    for i in range(0, len(o), 50):   # the texel against the restatement
        r = rq.trace_ray(m3, f3, o[i], d[i], lr)
        assert tuple(int(v) for v in hits[i]["texel"]) == r["texel"], i


def test_batch_sizes_and_a_large_batch(procedural_region):
    mats, mine = procedural_region
    rng = np.random.default_rng(23)
    n_big = 1 << 20
    o, d = seeded_rays(rng, n_big)
    with _ctx(mats, mine) as ctx:
        full = ctx.trace_rays(o, d)
        for n in (1, 63, 64, 65, 255, 256, 257, 65537):
            part = ctx.trace_rays(o[:n], d[:n])
            assert part.tobytes() == full[:n].tobytes(), n
            idx = sorted(set(range(min(n, 70))) | set(range(max(0, n - 3), n)))
            _oracle_check(mats, mine, o, d, part, (0, 0, 0), idx)
    _oracle_check(mats, mine, o, d, full, (0, 0, 0), rng.choice(n_big, 1500, replace=False))


# ---- picks against frames ------------------------------------------------------------------------------------------------------
KERNELS = [abi.RT_KERNEL_FRAME, abi.RT_KERNEL_PERSISTENT, abi.RT_KERNEL_PATHS, abi.RT_KERNEL_MEGA, abi.RT_KERNEL_WAVEFRONT]


def _check_picks_against_planes(hits, planes, u, W, H):
    hits = hits.reshape(H, W)
    air = hits["kind"] == abi.RT_HIT_AIR
    assert np.array_equal(air, planes["depth_r16"] == 0xFFFF)
    assert np.array_equal(np.where(air, abi_normal_air(), hits["normal"]).astype(np.uint8), planes["normal_r8"])
    m = hits["material"]
    alb = np.stack([(m >> 14) & 0x7F, (m >> 7) & 0x7F, m & 0x7F], axis=-1).astype(np.float32) / np.float32(127.0)
    alb = np.where(air[..., None], np.float32(1.0), alb)
    for c in range(3):   # rtm_unorm(x, 255): round-to-nearest of x * 255 (raytrace.comp:371-375)
        want = [po.unorm(float(v), 255.0) for v in alb[..., c].ravel()]
        assert np.array_equal(np.array(want).reshape(H, W), planes["albedo_rgba8"][..., c])
    origin = np.float32(u.origin[:])
    for y in range(H):
        for x in range(W):
            if air[y, x]:
                continue
            p = hits[y, x]["position"]
            dep = np.float32(length3([np.float32(origin[a] - p[a]) for a in range(3)]) * np.float32(32.0))
            assert_float_bits(dep, planes["depth_f32"][y, x])


def abi_normal_air():
    return 16   # RT_NORMAL_AIR (raytrace.comp:369)


CASES = [("256", 256, dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.2, sun=0.3, lr=(0, 0, 0))),
         ("512 scrolled", 512, dict(origin=(60.0 * 2, -20.0 * 2, 40.0 * 2), heading=2.2, pitch=-0.3, sun=0.5, lr=(32, -64, 32))),
         ("below the region", 256, dict(origin=(-30.0, -200.0, 40.0), heading=np.pi / 2, pitch=-0.1, sun=0.2, lr=(0, 0, 0)))]


@pytest.fixture(scope="module")
def region512_q(native_built):
    return world.generate_region(world.DEFAULT_SEED, region=512)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_picks_match_the_frames(case, procedural_region, region512_q, blue_noise):
    _, R, pose = case
    mats, mine = region512_q if R == 512 else procedural_region
    u = po.camera_uniforms(pose["origin"], pose["heading"], pose["pitch"], pose["sun"], 9, pose["lr"])
    W, H = 64, 40
    cpu, _ = po.render(mats, mine, blue_noise, u, W, H, 1, 2, region=R)
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2)
    picks = {}
    for kernel in KERNELS:
        if kernel == abi.RT_KERNEL_WAVEFRONT and R != 256:
            continue   # (region 256 only)
        with _ctx(mats, mine, W, H, R, noise=blue_noise, kernel=kernel) as ctx:
            ctx.draw_frame(u)
            hits = ctx.pick_pixels(u, xy)
            gpu = ctx.readback_all()
        for name in ("normal_r8", "albedo_rgba8", "depth_r16", "depth_f32"):
            assert np.array_equal(gpu[name].view(np.uint8), cpu[name].view(np.uint8)), (kernel, name)
        picks[kernel] = hits.tobytes()
    assert len(set(picks.values())) == 1
    _check_picks_against_planes(hits, cpu, u, W, H)
    if R == 256:
        # every 97th pixel pixels against the oracle's trace_ray from the start the frame uses
        for i in range(0, W * H, 97):
            x, y = xy[i]
            r = po.trace_ray(mats, mine, *_primary(u, x, y, W, H, R), pose["lr"])
            assert_float_bits(hits[i]["position"], r.position[:])
            assert int(hits[i]["kind"]) == oracle_kind(r) and int(hits[i]["material"]) == r.packed_material


def _primary(u, x, y, W, H, R):
    """primary_ray (raytrace.comp:296-297,306-315) restated with the exact helpers."""
    from tests.shader_trace import normalize3
    f32 = np.float32
    sx = f32(f32(f32(x) / f32(W)) * f32(2.0)) - f32(1.0)
    sy = f32(f32(f32(y) / f32(H)) * f32(2.0)) - f32(1.0)
    d = [f32(f32(f32(u.forward[a]) + f32(f32(u.right[a]) * sx)) + f32(f32(u.up[a]) * sy)) for a in range(3)]
    d = normalize3(d)
    s = [f32(v) for v in u.origin[:]]
    if -s[1] > f32(R / 2):
        space = f32(-s[1] - f32(R / 2))
        k = f32(f32(space / d[1]) + f32(0.0001))
        s = [f32(s[a] + f32(d[a] * k)) for a in range(3)]
    return s, d


def test_picks_on_a_tile_context(procedural_region, blue_noise):
    mats, mine = procedural_region
    u = po.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 9)
    W, H = 64, 40
    cpu, _ = po.render(mats, mine, blue_noise, u, W, H, 1, 2)
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2)
    with _ctx(mats, mine, W, H, noise=blue_noise, tile_world=2, tile_rank=1) as ctx:
        hits = ctx.pick_pixels(u, xy)
    _check_picks_against_planes(hits, cpu, u, W, H)


# ---- pick -> edit ---------------------------------------------------------------------------------------------------------------
def _edited_oracle(mats, mine, xyz, words, solid):
    """The oracle's view after an edit: the material word, and pack_into of the touched chunk (rt_edit_voxels' contract)."""
    from tests import voxel_edits as ve
    m, f = mats.reshape(256, 256, 256).copy(), mine.reshape(256, 256, 256).copy()
    ve.apply_edits(m, f, np.array([xyz]), np.array([words], np.uint32), np.array([bool(solid)]))
    return m.reshape(-1), f.reshape(-1)


def test_pick_then_edit_loop(procedural_region, blue_noise):
    import torch
    mats, mine = (a.copy() for a in procedural_region)
    u = po.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 9)
    W, H = 64, 40
    x, y = W // 2, H // 2
    o_d = _primary(u, x, y, W, H, 256)
    for mode in ("sync", "async", "user stream"):
        with _ctx(mats, mine, W, H, noise=blue_noise) as ctx:
            cur_m, cur_f = mats.copy(), mine.copy()
            stream = None
            if mode == "user stream":
                stream = torch.cuda.Stream()
                ctx.set_stream(stream.cuda_stream)
            rays = torch.tensor(np.concatenate([o_d[0], [0], o_d[1], [0]]).astype(np.float32)[None], device="cuda")
            hits_t = torch.zeros((1, 48), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()

            def query():
                if mode == "sync":
                    return ctx.pick_pixels(u, [(x, y)])[0]
                ctx.trace_rays_async(rays, hits_t)
                if stream is not None:
                    stream.synchronize()
                else:
                    ctx.sync()
                return hits_t.cpu().numpy().view(render.HIT_DTYPE).reshape(-1)[0]

            for step in range(3):
                h = query()
                r = po.trace_ray(cur_m, cur_f, o_d[0], o_d[1])
                assert_float_bits(h["position"], r.position[:])
                assert int(h["kind"]) == abi.RT_HIT_SOLID and int(h["material"]) == r.packed_material, (mode, step)
                t = tuple(int(v) for v in h["texel"])
                # break it: the pick now returns the next surface
                ctx.edit_voxels([t], [0], [0])
                cur_m, cur_f = _edited_oracle(cur_m, cur_f, t, 0, 0)
                h2 = query()
                r2 = po.trace_ray(cur_m, cur_f, o_d[0], o_d[1])
                assert_float_bits(h2["position"], r2.position[:])
                assert tuple(int(v) for v in h2["texel"]) != t
                # place a block in front of the face the first pick crossed: the pick returns it
                adj = tuple(int(v) for v in render.adjacent_texel(t, int(h["normal"])))
                ctx.edit_voxels([adj], [0x1234], [1])
                cur_m, cur_f = _edited_oracle(cur_m, cur_f, adj, 0x1234, 1)
                h3 = query()
                r3 = po.trace_ray(cur_m, cur_f, o_d[0], o_d[1])
                assert_float_bits(h3["position"], r3.position[:])
                assert tuple(int(v) for v in h3["texel"]) == adj and int(h3["material"]) == 0x1234
                # remove the placed block again and dig on
                ctx.edit_voxels([adj], [0], [0])
                cur_m, cur_f = _edited_oracle(cur_m, cur_f, adj, 0, 0)
            if stream is not None:
                ctx.set_stream(None)


def test_pipeline_pick(blue_noise):
    game = render.Game()
    game.generate_world()
    cfg = render.make_config(64, 40)
    pipe = render.create_instance(cfg, game, blue_noise)
    try:
        pipe.draw_frame(game)
        pipe.wait()
        u = pipe.uniforms()
        for x, yt in ((32, 20), (0, 0), (63, 39), (10, 30)):
            p = pipe.pick(game, x, yt)
            h = pipe.context.pick_pixels(u, [(x, int(render.row_from_bottom(yt, 40)))])[0]
            assert p["hit"].tobytes() == h.tobytes()
            if p["kind"] == abi.RT_HIT_SOLID:
                assert p["adjacent"] == tuple(int(v) for v in render.adjacent_texel(p["texel"], p["normal"]))
                assert p["world"] == tuple(int(v) for v in render.texel_to_world(p["texel"], tuple(u.lr[:])))
    finally:
        pipe.close()


# ---- no side effects ------------------------------------------------------------------------------------------------------------
def test_queries_do_not_disturb_accumulating_frames(procedural_region, blue_noise):
    mats, mine = procedural_region
    u = po.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 9)
    W, H, K = 64, 40, 4
    flags = abi.RT_FLAG_FRAMES_IN_FLIGHT_2 | abi.RT_FLAG_ACCUMULATE | abi.RT_FLAG_COUNTERS | abi.RT_FLAG_TIMING
    rng = np.random.default_rng(2)
    o, d = seeded_rays(rng, 5000)
    runs = []
    for interleave in (False, True):
        with _ctx(mats, mine, W, H, noise=blue_noise, kernel=abi.RT_KERNEL_PATHS, spp=2, flags=flags) as ctx:
            for k in range(K):
                u.seed = 100 + 2 * k
                ctx.draw_frame(u)
                if interleave:
                    ctx.trace_rays(o, d)
                    ctx.pick_pixels(u, [(1, 2), (30, 20)])
            ctx.sync()
            t = ctx.timing()
            runs.append((ctx.readback_all(), ctx.accumulation(), ctx.counters().as_dict(), (t.trace_launches, t.other_launches)))
    (p0, a0, c0, t0), (p1, a1, c1, t1) = runs
    for name in p0:
        assert p0[name].tobytes() == p1[name].tobytes(), name
    assert a0 == a1 and a0[0] == K
    assert c0 == c1 and t0 == t1


# ---- rejections ------------------------------------------------------------------------------------------------------------------
def test_rejections(procedural_region, blue_noise):
    mats, mine = procedural_region
    lib = render._lib.amd()
    u = po.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 9)
    W, H = 64, 40
    lr = (C.c_int32 * 3)(0, 0, 0)
    ray = np.zeros((1, 8), np.float32)
    ray[0, 6] = 1.0
    hit = np.zeros(1, render.HIT_DTYPE)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    with render.Context(render.make_config(W, H)) as ctx:
        assert lib.rt_trace_rays(ctx.handle, P(ray), 1, lr, P(hit)) == abi.RT_ERR_NOT_READY
        assert lib.rt_pick_pixels(ctx.handle, C.byref(u), P(np.zeros(2, np.int32)), 1, P(hit)) == abi.RT_ERR_NOT_READY
        assert lib.rt_trace_rays(ctx.handle, None, 0, lr, None) == abi.RT_OK
    with _ctx(mats, mine, W, H, noise=blue_noise) as ctx:
        ctx.draw_frame(u)
        before = ctx.readback_all()
        h = ctx.handle
        assert lib.rt_trace_rays(h, None, 1, lr, P(hit)) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_trace_rays(h, P(ray), 1, None, P(hit)) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_trace_rays(h, P(ray), 1, lr, None) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_trace_rays(h, P(ray), (1 << 26) + 1, lr, P(hit)) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_trace_rays_async(h, None, 1, lr, None) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_trace_rays_async(h, None, 0, lr, None) == abi.RT_OK
        for bad in ((-1, 0), (W, 0), (0, H), (0, -1)):
            xy = np.array(bad, np.int32)
            assert lib.rt_pick_pixels(h, C.byref(u), P(xy), 1, P(hit)) == abi.RT_ERR_INVALID_ARG, bad
        assert lib.rt_pick_pixels(h, None, P(np.zeros(2, np.int32)), 1, P(hit)) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_pick_pixels(h, C.byref(u), None, 0, None) == abi.RT_OK
        assert hit.tobytes() == np.zeros(1, render.HIT_DTYPE).tobytes()
        ctx.draw_frame(u)
        after = ctx.readback_all()
    for name in before:
        assert before[name].tobytes() == after[name].tobytes(), name
