"""Ray queries on the GPU, second part: the texel and every other field at region 512 (a scrolled window) against the restatement
generalised in R; an edit enqueued right behind an asynchronous query that is still running; asynchronous queries between
accumulating frames in flight; the refusal of misaligned device pointers."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from raytrace_amd import abi, render, world
from tests import ray_query_ref as rq
from tests.test_gpu_ray_queries import _ctx, _primary
from tests.test_ray_query_contract import assert_float_bits, oracle_kind, seeded_rays

pytestmark = pytest.mark.gpu


def _same(g, r):
    """A GPU hit record against a ray_query_ref result, every field."""
    assert_float_bits(g["position"], r["position"])
    assert_float_bits(g["distance"], r["distance"])
    assert tuple(int(v) for v in g["texel"]) == r["texel"]
    assert (int(g["material"]), int(g["normal"]), int(g["kind"]), int(g["iterations"]), int(g["border_fetches"])) == (
        r["material"], r["normal"], r["kind"], r["iterations"], r["border_fetches"])


@pytest.fixture(scope="module")
def region512_a(native_built):
    return world.generate_region(world.DEFAULT_SEED, region=512)


def test_region_512_rays_and_picks_match_the_restatement(region512_a, blue_noise):
    """R = 512 (swizzle with 128 bricks per axis) through a scrolled window: rays and picks, every field including the texel,
    against tests/ray_query_ref.py at R = 512."""
    R, lr = 512, (32, -64, 32)
    mats, mine = region512_a
    m3, f3 = mats.reshape(R, R, R), mine.reshape(R, R, R)
    rng = np.random.default_rng(29)
    o, d = seeded_rays(rng, 120, R)
    o += np.float32(lr)
    u = po.camera_uniforms((120.0, -40.0, 80.0), 2.2, -0.3, 0.5, 9, lr)
    W, H = 64, 40
    xy = [(x, y) for x in range(0, W, 9) for y in range(0, H, 7)]
    with _ctx(mats, mine, W, H, R, noise=blue_noise) as ctx:
        hits = ctx.trace_rays(o, d, lr)
        picks = ctx.pick_pixels(u, xy)
    solid = 0
    for i in range(len(o)):
        r = rq.trace_ray(m3, f3, o[i], d[i], lr, R)
        _same(hits[i], r)
        solid += r["kind"] == abi.RT_HIT_SOLID and r["texel"] != (-1, -1, -1)
    for (x, y), g in zip(xy, picks):
        r = rq.trace_ray(m3, f3, *_primary(u, x, y, W, H, R), lr, R)
        _same(g, r)
        solid += r["kind"] == abi.RT_HIT_SOLID
    assert solid > 20


def test_edit_behind_a_pending_async_query(procedural_region, blue_noise):
    """An edit enqueued while an asynchronous query still reads the region waits for it: 2^24 copies of one ray all report the
    surface before the edit, a query enqueued after the edit reports the one behind it."""
    from tests.test_gpu_ray_queries import _edited_oracle
    mats, mine = procedural_region
    u = po.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 9)
    start, direction = _primary(u, 32, 20, 64, 40, 256)
    ray = np.concatenate([start, [0], direction, [0]]).astype(np.float32)
    before = po.trace_ray(mats, mine, start, direction)
    assert not before.air
    with _ctx(mats, mine, noise=blue_noise) as ctx:
        texel = tuple(int(v) for v in ctx.trace_rays([start], [direction])[0]["texel"])
        n = 1 << 24
        rays = torch.from_numpy(ray).cuda().expand(n, 8).contiguous()
        hits_a = torch.zeros((n, 48), dtype=torch.uint8, device="cuda")
        one = rays[:1].clone()
        hits_b = torch.zeros((1, 48), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.trace_rays_async(rays, hits_a)
        ctx.edit_voxels([texel], [0], [0])           # no host wait between the query and the edit
        ctx.trace_rays_async(one, hits_b)
        ctx.sync()
        a = hits_a.cpu().numpy()
        b = hits_b.cpu().numpy().view(render.HIT_DTYPE).reshape(-1)[0]
    assert (a == a[0]).all(), "some copies of the ray saw the edited region"
    a0 = a[:1].view(render.HIT_DTYPE).reshape(-1)[0]
    assert_float_bits(a0["position"], before.position[:])
    assert int(a0["kind"]) == oracle_kind(before) and tuple(int(v) for v in a0["texel"]) == texel
    em, ef = _edited_oracle(mats, mine, texel, 0, 0)
    after = po.trace_ray(em, ef, start, direction)
    assert_float_bits(b["position"], after.position[:])
    assert int(b["kind"]) == oracle_kind(after) and tuple(int(v) for v in b["texel"]) != texel


def test_async_queries_between_accumulating_frames(procedural_region, blue_noise):
    """Asynchronous queries between frames in flight (two frame slots, accumulation): the frames are bit-identical to frames drawn
    without them, the accumulation, counters and launch counts too; the queries' hits equal the synchronous call's."""
    mats, mine = procedural_region
    u = po.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 9)
    W, H, K = 64, 40, 4
    flags = abi.RT_FLAG_FRAMES_IN_FLIGHT_2 | abi.RT_FLAG_ACCUMULATE | abi.RT_FLAG_COUNTERS | abi.RT_FLAG_TIMING
    o, d = seeded_rays(np.random.default_rng(4), 1 << 20)
    rays_np = np.zeros((len(o), 8), np.float32)
    rays_np[:, 0:3], rays_np[:, 4:7] = o, d
    rays = torch.from_numpy(rays_np).cuda()
    hits = [torch.zeros((len(o), 48), dtype=torch.uint8, device="cuda") for _ in range(K)]
    torch.cuda.synchronize()
    runs = []
    for interleave in (False, True):
        with _ctx(mats, mine, W, H, noise=blue_noise, kernel=abi.RT_KERNEL_PATHS, spp=2, flags=flags) as ctx:
            for k in range(K):
                u.seed = 100 + 2 * k
                ctx.draw_frame(u)
                if interleave:
                    ctx.trace_rays_async(rays, hits[k])   # no host wait anywhere until the end
            ctx.sync()
            t = ctx.timing()
            runs.append((ctx.readback_all(), ctx.accumulation(), ctx.counters().as_dict(), (t.trace_launches, t.other_launches)))
            if interleave:
                want = ctx.trace_rays(o, d)
    (p0, a0, c0, t0), (p1, a1, c1, t1) = runs
    for name in p0:
        assert p0[name].tobytes() == p1[name].tobytes(), name
    assert a0 == a1 and a0[0] == K
    assert c0 == c1 and t0 == t1
    for h in hits:
        assert h.cpu().numpy().tobytes() == want.tobytes()


def test_misaligned_device_pointers_are_refused(procedural_region):
    mats, mine = procedural_region
    lib = render._lib.amd()
    lr = (C.c_int32 * 3)(0, 0, 0)
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    with _ctx(mats, mine) as ctx:
        assert lib.rt_trace_rays_async(ctx.handle, C.c_void_p(base + 4), 1, lr, C.c_void_p(base + 1024)) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_trace_rays_async(ctx.handle, C.c_void_p(base), 1, lr, C.c_void_p(base + 1028)) == abi.RT_ERR_INVALID_ARG
        ctx.sync()
    assert not buf.any().item()
