"""The primary prepass (k_primary2) hands out its tiles dynamically: a workgroup takes chunks of 16 consecutive tiles from a cursor
in global memory until none are left, and the slot's two cursors are cleared in turn by the prepass before.  None of it may change a
bit of any frame: every case here compares all planes (and, where counted, the exact counters) with the oracle.  The frame sizes make a
chunk partly empty (8x8: one tile; 136x72: 153 tiles, nine full chunks and one of nine), the grid smaller than the CU count, and
some workgroups take several chunks (576x464: 261 chunks, more than there are workgroups)."""
import numpy as np
import pytest

from raytrace_amd import abi, render, tiles, world
from oracle import pyoracle as po
from tests.test_gpu_parity import _cached_counters, _compare

pytestmark = pytest.mark.gpu

SPP, DEPTH = 2, 2
CACHE = abi.RT_FLAG_CACHE_PRIMARY
POSE = dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.1, sun=0.3, seed=7, lr=(0, 0, 0))


def _u(**kw):
    p = dict(POSE)
    p.update(kw)
    return po.camera_uniforms(p["origin"], p["heading"], p["pitch"], p["sun"], p["seed"], p["lr"])


def _draw(scene, noise, u, W, H, spp=SPP, depth=DEPTH, flags=CACHE, **cfg):
    with render.Context(render.make_config(W, H, spp=spp, depth=depth, kernel=abi.RT_KERNEL_PATHS, flags=flags, **cfg)) as ctx:
        ctx.upload_world(*scene)
        ctx.upload_noise(noise)
        ctx.draw_frame(u)
        ctx.sync()
        assert ctx.kernel_in_use() == abi.RT_KERNEL_PATHS   # (RT_KERNEL_DEFAULT would draw frames this small on k_frame: no prepass)
        return ctx.readback_all(), ctx.counters() if flags & abi.RT_FLAG_COUNTERS else None


@pytest.fixture(scope="module")
def region512(native_built):
    return world.generate_region(world.DEFAULT_SEED, region=512)


@pytest.mark.parametrize("W,H", [(8, 8), (136, 72), (576, 464)])
def test_frame_sizes(procedural_region, blue_noise, W, H):
    assert ((W + 7) // 8) * ((H + 7) // 8) == {8: 1, 136: 153, 576: 4176}[W]
    u = _u()
    cpu, _ = po.render(*procedural_region, blue_noise, u, W, H, SPP, DEPTH)
    gpu, _ = _draw(procedural_region, blue_noise, u, W, H)
    _compare(gpu, cpu)


def test_tile_share(procedural_region, blue_noise):
    """Rank 1 of 3: 51 of the 153 tiles, every third one."""
    W, H, rank, nranks = 136, 72, 1, 3
    u = _u()
    cpu, _ = po.render(*procedural_region, blue_noise, u, W, H, SPP, DEPTH)
    gpu, _ = _draw(procedural_region, blue_noise, u, W, H, tile_rank=rank, tile_world=nranks)
    n = tiles.tile_count(W, H, rank, nranks) * 64
    assert n == 51 * 64
    inside = tiles.tile_major_from_frame(np.ones((H, W), dtype=np.uint8), rank, nranks)[:n].astype(bool)
    for name in cpu:
        exp = tiles.tile_major_from_frame(cpu[name], rank, nranks)
        px = gpu[name].reshape((-1,) + exp.shape[1:])[:n]
        assert np.array_equal(px[inside], exp[:n][inside], equal_nan=True), name


def test_scrolled_region(blue_noise, native_built):
    lr = (48, 0, 32)
    scene = world.toroidal_region(lr)
    u = _u(origin=(18.0, -128.0, 132.0), pitch=0.0, lr=lr)
    cpu, _ = po.render(*scene, blue_noise, u, 136, 72, SPP, DEPTH)
    gpu, _ = _draw(scene, blue_noise, u, 136, 72)
    _compare(gpu, cpu)


def test_depth_zero_is_the_prepass_alone(procedural_region, blue_noise):
    u = _u()
    cpu, _ = po.render(*procedural_region, blue_noise, u, 136, 72, SPP, 0)
    gpu, _ = _draw(procedural_region, blue_noise, u, 136, 72, depth=0)
    _compare(gpu, cpu)


@pytest.mark.parametrize("what,origin,heading,pitch", [("sky", (-30.0, -128.0, 120.0), np.pi / 2, 1.3), ("terrain", (0.0, 0.0, 120.0), 0.3, -1.2)])
def test_empty_and_full_worklists(procedural_region, blue_noise, what, origin, heading, pitch):
    u = _u(origin=origin, heading=heading, pitch=pitch)
    cpu, _ = po.render(*procedural_region, blue_noise, u, 136, 72, SPP, DEPTH)
    air = cpu["normal_r8"] == 16   # RT_NORMAL_AIR
    assert air.all() if what == "sky" else not air.any()
    gpu, _ = _draw(procedural_region, blue_noise, u, 136, 72)
    _compare(gpu, cpu)


def test_region_512(region512, blue_noise):
    u = _u(origin=(-60.0, -256.0, 110.0), pitch=-0.05)
    cpu, _ = po.render(*region512, blue_noise, u, 136, 72, SPP, DEPTH, region=512)
    gpu, _ = _draw(region512, blue_noise, u, 136, 72, region=512)
    _compare(gpu, cpu)


def _peek(ptrs, W, H):
    """Planes behind device pointers captured earlier (the slot of a frame that is no longer the context's current one)."""
    import torch
    import bench
    out = {}
    for b, ptr in ptrs.items():
        dt, ch = abi.BUFFER_FORMATS[b]
        n = W * H * ch * np.dtype(dt).itemsize
        raw = torch.as_tensor(bench._DevArray(ptr, n), device=torch.device("cuda", 0)).cpu().numpy()
        out[abi.BUFFER_NAMES[b]] = raw.view(dt).reshape((H, W, ch) if ch > 1 else (H, W))
    return out


def test_two_frame_slots_use_both_cursor_parities(procedural_region, blue_noise):
    """Six frames with six cameras enqueued back to back on two frame slots: every slot runs three prepasses, so both of its tile
    cursors are used, each cleared by the prepass before.  After one wait the context's planes are the last frame and the other
    slot still holds the frame before it."""
    W, H = 136, 72
    us = [_u(origin=(-30.0 + 3 * i, -128.0, 100.0 - 2 * i), heading=np.pi / 2 + 0.05 * i, pitch=-0.02 * i, seed=11 + 5 * i) for i in range(6)]
    cfg = render.make_config(W, H, spp=SPP, depth=DEPTH, kernel=abi.RT_KERNEL_PATHS, flags=CACHE | abi.RT_FLAG_FRAMES_IN_FLIGHT_2)
    with render.Context(cfg) as ctx:
        ctx.upload_world(*procedural_region)
        ctx.upload_noise(blue_noise)
        seen = []
        for u in us:
            ctx.draw_frame(u)
            seen.append({b: ctx.device_ptr(b) for b in range(abi.RT_BUF_FINAL_BGRA8)})
        ctx.sync()
        assert seen[0] == seen[2] == seen[4] and seen[1] == seen[3] == seen[5] and seen[0] != seen[1]
        last = ctx.readback_all()
        before = _peek(seen[4], W, H)
    _compare(last, po.render(*procedural_region, blue_noise, us[5], W, H, SPP, DEPTH)[0])
    _compare(before, po.render(*procedural_region, blue_noise, us[4], W, H, SPP, DEPTH)[0])


def test_counters_of_the_153_tile_frame(procedural_region, blue_noise):
    W, H = 136, 72
    u = _u()
    cpu, ccn = po.render(*procedural_region, blue_noise, u, W, H, SPP, DEPTH)
    gpu, gcn = _draw(procedural_region, blue_noise, u, W, H, flags=CACHE | abi.RT_FLAG_COUNTERS)
    _compare(gpu, cpu)
    assert gcn.rays_primary == W * H
    assert gcn.as_dict() == _cached_counters(*procedural_region, blue_noise, u, W, H, SPP, DEPTH, ccn)
