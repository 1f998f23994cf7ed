"""GPU parity on inputs outside the palette worlds (tests/adversarial_worlds.py, tests/synthetic_planes.py): every kernel against
the oracle, every plane bit for bit and the counters exact, on a region-wide pyramid minefield (values up to 9) and on an
arbitrary one (every value 0..30 in uniform, mixed and one-odd-voxel coarse cubes, random 32-bit material words); slabs that move
coarse cubes across the nibble map's boundaries; the post passes on synthetic planes.  tests/test_adversarial_worlds.py checks on
the CPU that these frames do reach every value and albedo code and that the oracle agrees with the second restatements there."""
import numpy as np
import pytest

from raytrace_amd import abi, render
from oracle import pyoracle as po
from tests import adversarial_worlds as aw
from tests import synthetic_planes as sp_planes
from tests.test_adversarial_worlds import FRAMES_256
from tests.test_gpu_parity import _cached_counters, _compare

pytestmark = pytest.mark.gpu

C, CACHE = abi.RT_FLAG_COUNTERS, abi.RT_FLAG_CACHE_PRIMARY
RUNS = [(abi.RT_KERNEL_MEGA, C), (abi.RT_KERNEL_PERSISTENT, C), (abi.RT_KERNEL_PERSISTENT, CACHE), (abi.RT_KERNEL_PATHS, CACHE),
        (abi.RT_KERNEL_FRAME, CACHE), (abi.RT_KERNEL_PATHS, CACHE | C), (abi.RT_KERNEL_DEFAULT, 0)]
RUNS_256 = RUNS + [(abi.RT_KERNEL_WAVEFRONT, C)]          # the split wavefront baseline takes region 256 only

_WORLDS = {}


def _world(name, R):
    """(materials, minefield), built once per module; one region above 256 is held at a time (5 GiB at 1024)."""
    if (name, R) not in _WORLDS:
        for k in [k for k in _WORLDS if k[1] > 256]:
            del _WORLDS[k]
        w = aw.arbitrary_world(R) if name == "arbitrary" else aw.pyramid_world(R)
        _WORLDS[(name, R)] = (w[0], w[1])
    return _WORLDS[(name, R)]


def _poses(name):
    return aw.POSES if name == "arbitrary" else aw.PYRAMID_POSES


def _want_kernel(kernel, flags, depth):
    """What kernel_in_use() must report after the frame (None: the library chooses)."""
    if kernel in (abi.RT_KERNEL_MEGA, abi.RT_KERNEL_WAVEFRONT):
        return kernel
    if kernel == abi.RT_KERNEL_PERSISTENT and not flags & CACHE:
        return kernel
    if kernel == abi.RT_KERNEL_PATHS and depth >= 1:
        return kernel
    if kernel == abi.RT_KERNEL_FRAME and depth <= 8:
        return kernel
    return None


def _check_runs(mats, mine, noise, u, W, H, spp, depth, R, runs):
    cpu, ccn = po.render(mats, mine, noise, u, W, H, spp, depth, region=R)
    cached = _cached_counters(mats, mine, noise, u, W, H, spp, depth, ccn, region=R)
    for kernel, flags in runs:
        cfg = render.make_config(W, H, spp=spp, depth=depth, kernel=kernel, flags=flags, region=R)
        with render.Context(cfg) as ctx:
            ctx.upload_world(mats, mine)
            ctx.upload_noise(noise)
            ctx.draw_frame(u)
            ctx.sync()
            gpu, gcn, ran = ctx.readback_all(), ctx.counters(), ctx.kernel_in_use()
        what = (kernel, flags, W, H, spp, depth, R)
        want = _want_kernel(kernel, flags, depth)
        assert want is None or ran == want, (what, ran)
        try:
            _compare(gpu, cpu)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (what, e))
        if flags & C:
            gd, cd = gcn.as_dict(), (cached if flags & CACHE else ccn.as_dict())
            assert gd == cd, (what, {k: (gd[k], cd[k]) for k in gd if gd[k] != cd[k]})
    return cpu


@pytest.mark.parametrize("name", ["arbitrary", "pyramid"])
@pytest.mark.parametrize("pose,W,H,spp,depth", FRAMES_256)
def test_kernels_match_oracle_at_256(name, pose, W, H, spp, depth, blue_noise, native_built):
    """Depth 0 (primary only), 2, 4 (STK 0), 5 and 8 (STK 2: levels 4-7 in global memory), 9 (k_frame's limit: k_persist);
    lr = 0 and lr != 0 (pose 4); one and several samples; frame sides that are not multiples of 8."""
    mats, mine = _world(name, 256)
    u = aw.pose_uniforms(po, _poses(name)[pose], 256, seed=pose * 97 + depth)
    cpu = _check_runs(mats, mine, blue_noise, u, W, H, spp, depth, 256, RUNS_256)
    assert (cpu["normal_r8"] != 16).mean() > 0.3       # the frame hits geometry


@pytest.mark.parametrize("R,pose,W,H,spp,depth", [(512, 4, 36, 21, 2, 5), (512, 0, 40, 27, 1, 2), (1024, 0, 40, 27, 2, 3),
                                                  (1024, 4, 28, 17, 1, 9)])
@pytest.mark.parametrize("name", ["arbitrary", "pyramid"])
def test_kernels_match_oracle_on_the_larger_regions(name, R, pose, W, H, spp, depth, blue_noise, native_built):
    mats, mine = _world(name, R)
    u = aw.pose_uniforms(po, _poses(name)[pose], R, seed=5 + depth)
    cpu = _check_runs(mats, mine, blue_noise, u, W, H, spp, depth, R, RUNS)
    assert (cpu["normal_r8"] != 16).mean() > 0.1


def _edit_slab(mine, mats, rng, e):
    """New content for a slab (shape a multiple of the coarse cube edge e on every axis): a uniform cube becomes mixed, an odd-voxel
    cube or another uniform value across the 6/7 or 14/15 boundary; a mixed cube becomes uniform.  New material words."""
    sz, sy, sx = mine.shape
    c = mine.reshape(sz // e, e, sy // e, e, sx // e, e)
    uni = c.min(axis=(1, 3, 5)) == c.max(axis=(1, 3, 5))
    v = c.min(axis=(1, 3, 5))
    across = np.array([7, 7, 7, 7, 7, 7, 7, 6, 6, 6, 15, 15, 15, 15, 15, 14, 14] + [14] * 14, dtype=np.uint8)   # v -> its boundary partner
    pick = rng.integers(0, 3, size=uni.shape)
    newv = np.where(uni, across[v], rng.choice(np.array([1, 2, 6, 7, 14, 15], dtype=np.uint8), size=uni.shape)).astype(np.uint8)
    to_mixed = uni & (pick == 0)
    to_odd = uni & (pick == 1)
    newv[to_odd] = 1
    b = lambda a: np.broadcast_to(a[:, None, :, None, :, None], c.shape).reshape(mine.shape)
    out = b(newv).copy()
    m = b(to_mixed)
    out[m] = rng.integers(0, 31, size=int(m.sum()), dtype=np.uint8)
    oz, oy, ox = np.nonzero(to_odd)
    k = rng.integers(0, e, size=(len(oz), 3))
    out[oz * e + k[:, 0], oy * e + k[:, 1], ox * e + k[:, 2]] = 0
    return out, rng.integers(0, 1 << 32, size=mats.shape, dtype=np.uint32)


@pytest.mark.parametrize("R", [256, 512, 1024])
def test_slabs_across_the_nibble_boundaries(R, blue_noise, native_built):
    """rt_upload_slice on the arbitrary world: slabs at offset 0, R - 16 and next to the camera on each axis that flip cubes between
    uniform and mixed and move uniform values across 6/7 and 14/15; through the direct and the staging path, with and without
    RT_FLAG_TRUSTED_WORLD; then a frame whose rays cross the slabs against the oracle on the edited world."""
    for k in [k for k in _WORLDS if k[1] > 256]:
        del _WORLDS[k]
    mats, mine, _, _ = aw.arbitrary_world(R)      # edited in place below: not the module's shared copy
    e = R // 64
    pose = aw.POSES[0]
    cam = [int(c + R // 2) for c in aw.pose_origin(pose, R)]
    u = aw.pose_uniforms(po, pose, R, seed=12)
    W, H, spp, depth = 48, 40, 1, 2
    edits = []
    for axis in range(3):
        near = (cam[axis] // 16 + 1) * 16
        for off in (0, R - 16, near):
            edits.append((axis, off))
    runs = [(abi.RT_KERNEL_DEFAULT, CACHE), (abi.RT_KERNEL_PATHS, CACHE | abi.RT_FLAG_TRUSTED_WORLD)]
    ctxs = []
    try:
        for kernel, flags in runs:
            ctx = render.Context(render.make_config(W, H, spp=spp, depth=depth, kernel=kernel, flags=flags, region=R))
            ctxs.append(ctx)
            ctx.upload_world(mats, mine)
            ctx.upload_noise(blue_noise)
            assert ctx.selftest(abi.RT_SELFTEST_SCENE_MAPS) == 0      # every nibble value, uniform 15..30 included (mixed)
        rng = np.random.default_rng(R)
        slab_bricks = np.zeros((64, 64, 64), dtype=np.uint8) if R == 256 else None
        for k, (axis, off) in enumerate(edits):
            sl = [slice(None)] * 3
            sl[2 - axis] = slice(off, off + 16)      # arrays are [z, y, x]
            sl = tuple(sl)
            nm, nt = _edit_slab(mine[sl], mats[sl], rng, e)
            mine[sl] = nm
            mats[sl] = nt
            if slab_bricks is not None:
                bs = [slice(None)] * 3
                bs[2 - axis] = slice(off // 4, off // 4 + 4)
                slab_bricks[tuple(bs)] = 1
            for j, ctx in enumerate(ctxs):
                if (k + j) % 2 == 0:
                    ctx.upload_slice(axis, off, np.ascontiguousarray(nt), np.ascontiguousarray(nm))
                else:
                    sm, sf = ctx.slice_staging()
                    sm[:] = nt.reshape(-1)
                    sf[:] = nm.reshape(-1)
                    ctx.upload_slice(axis, off, sm, sf)
        for ctx in ctxs:
            assert ctx.selftest(abi.RT_SELFTEST_SCENE_MAPS) == 0      # ... and after the slabs' partial rebuilds
        cpu, _ = po.render(mats, mine, blue_noise, u, W, H, spp, depth, region=R)
        for ctx, (kernel, flags) in zip(ctxs, runs):
            ctx.draw_frame(u)
            ctx.sync()
            try:
                _compare(ctx.readback_all(), cpu)
            except AssertionError as err:
                raise AssertionError("%s: %s" % ((kernel, flags, R), err))
    finally:
        for ctx in ctxs:
            ctx.destroy()
    assert (cpu["normal_r8"] != 16).mean() > 0.05
    if slab_bricks is not None:
        # the rays cross the slabs: the oracle's fetch statistics with the slabs' bricks as the "uniform" set count the fetches there
        _, _, hist = po.fetch_histogram(mats, mine, blue_noise, u, W, H, spp, depth, bricks=slab_bricks)
        assert hist[1].sum() > 1000 and hist[1][7] + hist[1][15] + hist[1][6] + hist[1][14] > 0, hist[1]


def test_brick_map_words_of_every_builder(monkeypatch, native_built):
    """RT_BRICK_MAP makes the library keep the per-brick nibble map above R = 256 (no shipped kernel consults it, so nothing else
    runs its builders): on the arbitrary world, the brick words of the upload, of uploaded slabs on each axis, of an edit batch, of
    a generated slab and of a generated region against the voxel-by-voxel self-test."""
    R = 512
    monkeypatch.setenv("RT_BRICK_MAP", "1")
    for k in [k for k in _WORLDS if k[1] > 256]:
        del _WORLDS[k]
    mats, mine, _, _ = aw.arbitrary_world(R)
    rng = np.random.default_rng(7)
    with render.Context(render.make_config(64, 64, region=R)) as ctx:
        ctx.upload_world(mats, mine)
        assert ctx.selftest(abi.RT_SELFTEST_SCENE_MAPS) == 0
        for axis, off in ((0, 16), (0, 208), (1, 0), (2, R - 16)):       # x slabs inside one brick word and across two
            sl = [slice(None)] * 3
            sl[2 - axis] = slice(off, off + 16)
            nm, nt = _edit_slab(mine[tuple(sl)], mats[tuple(sl)], rng, R // 64)
            ctx.upload_slice(axis, off, np.ascontiguousarray(nt), np.ascontiguousarray(nm))
            assert ctx.selftest(abi.RT_SELFTEST_SCENE_MAPS) == 0, (axis, off)
        n = 3000
        ctx.edit_voxels(rng.integers(0, R, size=(n, 3)), rng.integers(0, 1 << 32, size=n, dtype=np.uint32), rng.random(n) < 0.5)
        assert ctx.selftest(abi.RT_SELFTEST_SCENE_MAPS) == 0
        ctx.generate_slice(0x5EED, 0, (R // 2 + 32, -R // 2, -R // 2))
        assert ctx.selftest(abi.RT_SELFTEST_SCENE_MAPS) == 0
        ctx.generate_world(0x5EED)
        assert ctx.selftest(abi.RT_SELFTEST_SCENE_MAPS) == 0


@pytest.mark.parametrize("W,H", [(1, 1), (3, 50), (333, 77), (1920, 1080)])
def test_post_passes_on_synthetic_planes(W, H, blue_noise, native_built, monkeypatch):
    """rt_denoise_planes / rt_finalize_planes on caller planes (torch device tensors) that a rendered frame never holds: depths below
    16 in clusters, alone at tile corners and frame edges, or absent from a tile; full fog; every normal byte; full-range lighting
    with alpha != 4096; non-zero emission.  Both descriptor-set modes, the LDS-tiled and the direct dispatches: bit for bit against
    po.denoise and po.finalize.  (That the pong dispatches do filter the near pixels here is asserted in the oracle on the CPU.)"""
    import torch
    p = sp_planes.post_planes(W, H, seed=W * 7 + H)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(dev)
    depth, normal, albedo, emission, fog = t(p["depth"]), t(p["normal"]), t(p["albedo"]), t(p["emission"]), t(p["fog"])
    out = torch.zeros(W * H * 4, dtype=torch.uint8, device=dev)
    with render.Context(render.make_config(W, H)) as ctx:
        ctx.upload_noise(blue_noise)
        for faithful in (True, False):
            exp_den = po.denoise(p["lighting"], p["depth"], p["normal"], faithful=faithful)
            exp_fin = po.finalize(p["albedo"], p["emission"], p["fog"], exp_den, p["depth"], blue_noise)
            for untiled in (False, True):
                if untiled:
                    monkeypatch.setenv("RT_DENOISE_UNTILED", "1")
                else:
                    monkeypatch.delenv("RT_DENOISE_UNTILED", raising=False)
                lighting = t(p["lighting"])
                out.zero_()
                torch.cuda.synchronize()
                ctx.denoise_planes(lighting.data_ptr(), depth.data_ptr(), normal.data_ptr(), faithful=faithful)
                ctx.finalize_planes(albedo.data_ptr(), emission.data_ptr(), fog.data_ptr(), lighting.data_ptr(), depth.data_ptr(),
                                    out.data_ptr())
                ctx.sync()
                den = lighting.cpu().numpy().view(np.uint16).reshape(H, W, 4)
                fin = out.cpu().numpy().reshape(H, W, 4)
                assert np.array_equal(den, exp_den), ("denoise", faithful, untiled, int(np.count_nonzero(den != exp_den)))
                assert np.array_equal(fin, exp_fin), ("finalize", faithful, untiled, int(np.count_nonzero(fin != exp_fin)))
