"""Light probes on the GPU (rt_probe_light, rt_probe_light_async), everything bit for bit, sun_samples included: the identity
against the lighting planes of frames drawn by several kernels (regions 256 and 512, a scrolled window, depth 8), reference cases
against tests/light_probe_ref.py, the sample and batch sizes at which the reduction and the launch split change, the asynchronous
call and its ordering against an edit, every rejection, and the absence of side effects on accumulating, reprojecting frames."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from raytrace_amd import abi, render, world
from tests import light_probe_ref as lp
from tests import scenes
from tests.test_gpu_ray_queries import _ctx

pytestmark = pytest.mark.gpu

TERRAIN_POSE = dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.2, sun=0.3, lr=(0, 0, 0))
BLOCKS_POSE = dict(origin=(-60.0, -90.0, -60.0), heading=0.9, pitch=-0.35, sun=0.6, lr=(0, 0, 0))
POSE_512 = dict(origin=(120.0, -40.0, 80.0), heading=2.2, pitch=-0.3, sun=0.5, lr=(32, -64, 32))
W, H = 72, 44


def _u(pose, seed):
    return po.camera_uniforms(pose["origin"], pose["heading"], pose["pitch"], pose["sun"], seed, pose["lr"])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def blocks_region(native_built):
    return world.region_from_ids(scenes.random_blocks_ids())


@pytest.fixture(scope="module")
def stairs_region(native_built):
    return world.region_from_ids(scenes.staircase_ids())


@pytest.fixture(scope="module")
def region512_p(native_built):
    return world.generate_region(world.DEFAULT_SEED, region=512)


def _pixel_probes(ctx, u, width, height):
    """(xy int[N, 2], RtLightProbe records) of the pixels whose primary ray hits: position and normal as rt_pick_pixels returns them,
    the pixel's workgroup as the noise cell."""
    xy = np.stack(np.meshgrid(np.arange(width), np.arange(height)), axis=-1).reshape(-1, 2)
    hits = ctx.pick_pixels(u, xy)
    keep = hits["kind"] != abi.RT_HIT_AIR
    xy, hits = xy[keep], hits[keep]
    cells = np.stack([render.workgroup_of(xy[:, 0]), render.workgroup_of(xy[:, 1])], axis=-1)
    return xy, render.make_probes(hits["position"], hits["normal"], cells)


@pytest.fixture(scope="module")
def terrain_probes(procedural_region, blue_noise):
    """The probes of the terrain frame's non-sky pixels: shared input of the shape, async and side-effect tests."""
    mats, mine = procedural_region
    with _ctx(mats, mine, W, H, noise=blue_noise) as ctx:
        _, probes = _pixel_probes(ctx, _u(TERRAIN_POSE, 21), W, H)
    assert len(probes) > 1500
    return probes


def _check_ref(mats, mine, noise, pose, seed, probes, got, samples, depth, idx):
    for i in idx:
        p = probes[i]
        light, sun = lp.probe_light(mats, mine, noise, pose["sun"], seed, pose["lr"], p["position"], int(p["normal"]),
                                    (int(p["cell"][0]), int(p["cell"][1])), samples, depth)
        g = got[i]
        nan = np.isnan(light)
        assert np.array_equal(nan, np.isnan(g["light"])), (i, light, g)
        assert bits(g["light"])[~nan].tolist() == bits(light)[~nan].tolist(), (i, light, g)
        assert int(g["sun_samples"]) == sun, (i, sun, g)


# ---- identity against frames ----------------------------------------------------------------------------------------------------
IDENTITY = [
    ("terrain spp 4", "terrain", TERRAIN_POSE, 256, 4, 2, (abi.RT_KERNEL_DEFAULT, abi.RT_KERNEL_PATHS)),
    ("terrain spp 1", "terrain", TERRAIN_POSE, 256, 1, 2, (abi.RT_KERNEL_DEFAULT, abi.RT_KERNEL_MEGA)),
    ("512 scrolled", "512", POSE_512, 512, 4, 2, (abi.RT_KERNEL_DEFAULT, abi.RT_KERNEL_PERSISTENT)),
    ("blocks depth 8", "blocks", BLOCKS_POSE, 256, 4, 8, (abi.RT_KERNEL_FRAME, abi.RT_KERNEL_PERSISTENT)),
]


@pytest.mark.parametrize("case", IDENTITY, ids=[c[0] for c in IDENTITY])
def test_probes_equal_the_lighting_of_frames(case, procedural_region, blocks_region, region512_p, blue_noise):
    _, scene, pose, R, spp, depth, kernels = case
    mats, mine = {"terrain": procedural_region, "blocks": blocks_region, "512": region512_p}[scene]
    seed = 21
    u, u_next = _u(pose, seed), _u(pose, seed + 1)
    frames, used = [], set()
    for kernel in kernels:
        with _ctx(mats, mine, W, H, R, noise=blue_noise, kernel=kernel, spp=spp, depth=depth, flags=abi.RT_FLAG_CACHE_PRIMARY) as ctx:
            ctx.draw_frame(u)
            frames.append(ctx.readback(abi.RT_BUF_LIGHTING_F32))
            used.add(ctx.kernel_in_use())
            if kernel != kernels[0]:
                continue
            ctx.draw_frame(u_next)
            frame_next = ctx.readback(abi.RT_BUF_LIGHTING_F32)
            xy, probes = _pixel_probes(ctx, u, W, H)
            got = ctx.probe_records(u, probes, spp, depth)
            shallow = ctx.probe_records(u, probes, spp, 1)
    assert len(used) >= 2                                        # two routes drew the frame ...
    assert frames[0].tobytes() == frames[1].tobytes()            # ... and the lighting does not depend on the route
    if R == 512:   # the yardstick at this region is the oracle's own frame
        cpu, _ = po.render(mats, mine, blue_noise, u, W, H, spp, depth, region=R)
        assert cpu["lighting_f32"].tobytes() == frames[0].tobytes()
    want = frames[0][xy[:, 1], xy[:, 0], :3]
    assert bits(got["light"] / np.float32(16.0)).tolist() == bits(want).tolist()
    # the conditions on the input: mostly surfaces, light that depends on the seed, paths that go deeper than one level
    assert len(probes) >= 0.6 * W * H
    changed = np.any(bits(frames[0]) != bits(frame_next), axis=-1)[xy[:, 1], xy[:, 0]]
    assert np.count_nonzero(changed) >= 0.5 * len(probes)
    deeper = np.any(bits(got["light"]) != bits(shallow["light"]), axis=-1)   # (a lower bound: a level 2 in the dark adds nothing)
    assert np.count_nonzero(deeper) >= 0.1 * len(probes)
    assert got["sun_samples"].max() <= spp and got["sun_samples"].max() > 0


# ---- reference cases at R = 256 -------------------------------------------------------------------------------------------------
def test_sphere_probes_and_illegal_positions(procedural_region, blue_noise):
    """RT_PROBE_SPHERE in the open air and near the ground; a probe inside a solid voxel, one outside the window, NaN coordinates."""
    mats, mine = procedural_region
    solid = np.argwhere(mine.reshape(256, 256, 256) == 0)[::50000][:3, ::-1] - 128 + np.float32(0.4)
    pos = [(-30.0, -100.0, 110.0), (10.5, 20.25, 60.0), (-30.0, -128.0, 20.0), (0.0, 0.0, 127.5)] + [tuple(v) for v in solid] + [
        (300.0, 0.0, 0.0), (0.0, -500.0, 10.0), (np.nan, 0.0, 0.0), (1.0, 2.0, np.nan)]
    nrm = [abi.RT_PROBE_SPHERE] * 4 + [4, abi.RT_PROBE_SPHERE, 0] + [4, abi.RT_PROBE_SPHERE, 2, abi.RT_PROBE_SPHERE]
    probes = render.make_probes(pos, nrm, [(3 * i, 5 * i + 1) for i in range(len(pos))])
    u = _u(TERRAIN_POSE, 77)
    with _ctx(mats, mine, noise=blue_noise) as ctx:
        got = ctx.probe_records(u, probes, 3, 3)
    _check_ref(mats, mine, blue_noise, TERRAIN_POSE, 77, probes, got, 3, 3, range(len(probes)))
    assert np.count_nonzero(got["sun_samples"][:4]) > 0


def test_six_faces_of_a_free_standing_block(stairs_region, blue_noise):
    """The floating block of the staircase scene (world x, y in [-28, -18), z in [52, 62)): a probe just off the middle of each face
    with that face's code, and the wrong way round (the hemisphere points into the block)."""
    mats, mine = stairs_region
    lo, hi, mid, off = (-28.0, -28.0, 52.0), (-18.0, -18.0, 62.0), (-23.5, -23.5, 57.5), 0.001
    pos, nrm = [], []
    for code in range(6):
        axis, p = code // 2, list(mid)
        p[axis] = hi[axis] + off if code % 2 == 0 else lo[axis] - off
        pos += [tuple(p), tuple(p)]
        nrm += [code, code ^ 1]
    probes = render.make_probes(pos, nrm, [(i, 2 * i) for i in range(len(pos))])
    pose = dict(TERRAIN_POSE, sun=0.8)
    u = _u(pose, 5)
    with _ctx(mats, mine, noise=blue_noise) as ctx:
        got = ctx.probe_records(u, probes, 4, 2)
    _check_ref(mats, mine, blue_noise, pose, 5, probes, got, 4, 2, range(len(probes)))
    assert len({g.tobytes() for g in got}) > 6


UNIFORM_CASES = [("sun_angle 0", 0.0, 9, (4, 7)), ("seed wraps", 0.3, abi.NOISE_BYTES - 2, (4, 7)), ("cell 65535", 0.3, 9, (65535, 65535))]


@pytest.mark.parametrize("case", UNIFORM_CASES, ids=[c[0] for c in UNIFORM_CASES])
def test_uniform_and_cell_edges(case, procedural_region, terrain_probes, blue_noise):
    _, sun, seed, cell = case
    mats, mine = procedural_region
    probes = terrain_probes[::331].copy()
    probes["cell"] = cell
    pose = dict(TERRAIN_POSE, sun=sun)
    u = _u(pose, seed)
    with _ctx(mats, mine, noise=blue_noise) as ctx:
        got = ctx.probe_records(u, probes, 4, 2)
    _check_ref(mats, mine, blue_noise, pose, seed, probes, got, 4, 2, range(len(probes)))


# ---- shapes that break reductions and launch splits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [1, 3, 64, 65, 256, 257, 4096])
def test_sample_counts_of_one_probe(samples, procedural_region, terrain_probes, blue_noise):
    """One probe at every sample count where the sum changes hands: inside the workgroup (1, 64, 256), through the scratch (3, 65,
    257, 4096).  (4096 samples at depth 1: the reference walks every path on the CPU.)"""
    mats, mine = procedural_region
    depth = 1 if samples == 4096 else 2
    probes = terrain_probes[700:701]
    u = _u(TERRAIN_POSE, 33)
    with _ctx(mats, mine, noise=blue_noise) as ctx:
        got = ctx.probe_records(u, probes, samples, depth)
    _check_ref(mats, mine, blue_noise, TERRAIN_POSE, 33, probes, got, samples, depth, [0])


def test_probe_counts_and_the_scratch_bound(procedural_region, terrain_probes, blue_noise):
    """count 1, 63, 65 and 1000 at 5 samples (the scratch path), then one call whose path records pass the 64 MiB scratch by one
    probe (two launches): every result equals that of the same probe in the 1000-probe call."""
    mats, mine = procedural_region
    samples, depth = 5, 2
    base = terrain_probes[:1000]
    u = _u(TERRAIN_POSE, 33)
    with _ctx(mats, mine, noise=blue_noise) as ctx:
        before = ctx.info().device_bytes
        full = ctx.probe_records(u, base, samples, depth)
        for n in (1, 63, 65):
            assert ctx.probe_records(u, base[:n], samples, depth).tobytes() == full[:n].tobytes(), n
        per_launch = (64 << 20) // 16 // samples
        n_big = per_launch + 1
        big = ctx.probe_records(u, np.resize(base, n_big), samples, depth)
        grown = ctx.info().device_bytes - before
    assert np.array_equal(big.view(np.uint32).reshape(-1, 4), np.resize(full, n_big).view(np.uint32).reshape(-1, 4))
    assert grown >= per_launch * samples * 16     # the scratch (and the staging) are counted ...
    assert grown <= (64 << 20) + 2 * n_big * 48   # ... and the scratch stays within its bound
    _check_ref(mats, mine, blue_noise, TERRAIN_POSE, 33, base, full, samples, depth, [0, 1, 62, 63, 64, 998, 999])


@pytest.mark.parametrize("samples", [4, 7])
def test_a_repeated_probe_gives_one_answer(samples, procedural_region, terrain_probes, blue_noise):
    mats, mine = procedural_region
    probes = np.resize(terrain_probes[900:901], 300)
    with _ctx(mats, mine, noise=blue_noise) as ctx:
        got = ctx.probe_records(_u(TERRAIN_POSE, 12), probes, samples, 3)
    assert len({g.tobytes() for g in got}) == 1


def test_every_kernel_and_a_tile_context_answer_the_same(procedural_region, terrain_probes, blue_noise):
    mats, mine = procedural_region
    probes = terrain_probes[::7]
    u = _u(TERRAIN_POSE, 21)
    answers = set()
    for kw in (dict(), dict(kernel=abi.RT_KERNEL_MEGA), dict(kernel=abi.RT_KERNEL_WAVEFRONT), dict(kernel=abi.RT_KERNEL_PATHS),
               dict(tile_world=2, tile_rank=1), dict(spp=8, depth=0)):
        with _ctx(mats, mine, noise=blue_noise, **kw) as ctx:
            answers.add(ctx.probe_records(u, probes, 6, 3).tobytes())
    assert len(answers) == 1


# ---- async ---------------------------------------------------------------------------------------------------------------------
def _dev(probes):
    return torch.from_numpy(probes.view(np.uint8).reshape(-1, 32).copy()).cuda()


def _host(out_t):
    return out_t.cpu().numpy().view(render.PROBE_LIGHT_DTYPE).reshape(-1)


@pytest.mark.parametrize("samples", [4, 5])
def test_async_on_the_query_stream_and_on_a_callers_stream(samples, procedural_region, terrain_probes, blue_noise):
    mats, mine = procedural_region
    u = _u(TERRAIN_POSE, 21)
    probes_t = _dev(terrain_probes)
    out_a = torch.zeros((len(terrain_probes), 4), dtype=torch.float32, device="cuda")
    out_b = torch.zeros_like(out_a)
    torch.cuda.synchronize()
    with _ctx(mats, mine, noise=blue_noise) as ctx:
        want = ctx.probe_records(u, terrain_probes, samples, 2)
        ctx.probe_light_async(u, probes_t, out_a, samples, 2)
        ctx.sync()
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        ctx.probe_light_async(u, probes_t, out_b, samples, 2)
        stream.synchronize()
        on_stream = ctx.probe_records(u, terrain_probes, samples, 2)
        ctx.set_stream(None)
    assert _host(out_a).tobytes() == want.tobytes()
    assert _host(out_b).tobytes() == want.tobytes()
    assert on_stream.tobytes() == want.tobytes()


def test_async_pointers_are_checked(procedural_region, blue_noise):
    mats, mine = procedural_region
    lib = render._lib.amd()
    u = _u(TERRAIN_POSE, 21)
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    host = np.zeros(64, np.uint8)
    hp = host.ctypes.data_as(C.c_void_p)
    with _ctx(mats, mine, noise=blue_noise) as ctx:
        h = ctx.handle
        call = lambda p, o: lib.rt_probe_light_async(h, C.byref(u), p, 1, 2, 2, o)  # noqa: E731
        assert call(C.c_void_p(base + 4), C.c_void_p(base + 1024)) == abi.RT_ERR_INVALID_ARG
        assert call(C.c_void_p(base), C.c_void_p(base + 1028)) == abi.RT_ERR_INVALID_ARG
        assert call(hp, C.c_void_p(base + 1024)) == abi.RT_ERR_INVALID_ARG
        assert call(C.c_void_p(base), hp) == abi.RT_ERR_INVALID_ARG
        assert call(None, C.c_void_p(base + 1024)) == abi.RT_ERR_INVALID_ARG
        assert call(C.c_void_p(base), None) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_probe_light_async(h, None, C.c_void_p(base), 1, 2, 2, C.c_void_p(base + 1024)) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_probe_light_async(h, C.byref(u), None, 0, 2, 2, None) == abi.RT_OK
        ctx.sync()
    assert not buf.any().item() and not host.any()


def test_an_edit_between_two_async_calls_shades_only_the_second(procedural_region, terrain_probes, blue_noise):
    """A probe in full sun; 27 voxels placed three voxels up its sun ray between two asynchronous calls, with no host wait: the
    first call (2^16 copies of the probe, still running when the edit is enqueued) answers for the world before the edit, the
    second for the world after it."""
    mats, mine = procedural_region
    samples, depth = 16, 2
    u = _u(TERRAIN_POSE, 21)
    sunangle, _ = po.sun(TERRAIN_POSE["sun"])
    with _ctx(mats, mine, noise=blue_noise) as ctx:
        lit = ctx.probe_records(u, terrain_probes, samples, depth)
        i = int(np.flatnonzero((lit["sun_samples"] == samples) & (terrain_probes["normal"] == 4))[0])
        probe = terrain_probes[i:i + 1]
        q = np.floor(probe["position"][0] + np.float32(3.0) * sunangle + np.float32(128.0)).astype(np.int64)
        xyz = [(q[0] + dx, q[1] + dy, q[2] + dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]
        assert min(min(t) for t in xyz) >= 0 and max(max(t) for t in xyz) < 256
        n = 1 << 16
        many = _dev(np.resize(probe, n))
        out_a = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        one = _dev(probe)
        out_b = torch.zeros((1, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.probe_light_async(u, many, out_a, samples, depth)
        ctx.edit_voxels(xyz, [0x1234] * 27, [1] * 27)       # no host wait between the probes and the edit
        ctx.probe_light_async(u, one, out_b, samples, depth)
        ctx.sync()
        after = ctx.probe_records(u, probe, samples, depth)
    a, b = _host(out_a), _host(out_b)
    assert len({g.tobytes() for g in a}) == 1, "some copies of the probe saw the edited region"
    assert a[0].tobytes() == lit[i].tobytes() and int(a[0]["sun_samples"]) == samples
    assert b[0].tobytes() == after[0].tobytes() and int(b[0]["sun_samples"]) == 0
    assert b[0].tobytes() != a[0].tobytes()


# ---- arguments -----------------------------------------------------------------------------------------------------------------
def _rejections(ctx, u, probes):
    """Every rejected form of the two calls on a ready context; returns how many were made."""
    lib = render._lib.amd()
    h = ctx.handle
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.zeros(len(probes), render.PROBE_LIGHT_DTYPE)
    dev_in = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    dev_out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    n = len(probes)
    calls = 0
    for fn, pi, po_ in ((lib.rt_probe_light, P(probes), P(out)), (lib.rt_probe_light_async, C.c_void_p(dev_in.data_ptr()), C.c_void_p(dev_out.data_ptr()))):
        for samples, depth, count in ((0, 2, n), (4097, 2, n), (4, 0, n), (4, 17, n), (4, -1, n), (4, 2, (1 << 24) + 1), (4096, 2, (1 << 14) + 1)):
            assert fn(h, C.byref(u), pi, count, samples, depth, po_) == abi.RT_ERR_INVALID_ARG, (samples, depth, count)
            calls += 1
        assert fn(h, None, pi, n, 4, 2, po_) == abi.RT_ERR_INVALID_ARG
        assert fn(h, C.byref(u), None, n, 4, 2, po_) == abi.RT_ERR_INVALID_ARG
        assert fn(h, C.byref(u), pi, n, 4, 2, None) == abi.RT_ERR_INVALID_ARG
        assert fn(h, C.byref(u), None, 0, 4, 2, None) == abi.RT_OK            # count == 0: nothing to do
        calls += 4
    bad = probes.copy()
    bad["normal"][-1] = 7
    assert lib.rt_probe_light(h, C.byref(u), P(bad), n, 4, 2, P(out)) == abi.RT_ERR_INVALID_ARG
    for k in range(3):
        bad = probes.copy()
        bad["reserved"][n // 2, k] = 1
        assert lib.rt_probe_light(h, C.byref(u), P(bad), n, 4, 2, P(out)) == abi.RT_ERR_INVALID_ARG
    assert not out.view(np.uint8).any() and not dev_out.any().item()
    return calls + 4


def test_rejections_change_nothing(procedural_region, terrain_probes, blue_noise):
    """Each rejection of the header's list; frames of an accumulating context drawn round them, and rt_get_accumulation, are those
    of a run without them."""
    mats, mine = procedural_region
    probes = terrain_probes[:40]
    runs = []
    for reject in (False, True):
        with _ctx(mats, mine, W, H, noise=blue_noise, spp=2, flags=abi.RT_FLAG_ACCUMULATE | abi.RT_FLAG_CACHE_PRIMARY) as ctx:
            seen = []
            for k in range(3):
                u = _u(TERRAIN_POSE, 100 + 2 * k)
                ctx.draw_frame(u)
                if reject:
                    assert _rejections(ctx, u, probes) > 20
                    seen.append(ctx.accumulation())
                else:
                    seen.append(ctx.accumulation())
            runs.append((ctx.readback_all(), seen))
    (p0, a0), (p1, a1) = runs
    assert a0 == a1 and a0[-1][0] == 3
    for name in p0:
        assert p0[name].tobytes() == p1[name].tobytes(), name


def test_not_ready_without_a_world_or_noise(procedural_region, blue_noise):
    mats, mine = procedural_region
    lib = render._lib.amd()
    u = _u(TERRAIN_POSE, 1)
    probes = render.make_probes([(0.0, 0.0, 100.0)], [abi.RT_PROBE_SPHERE], [(0, 0)])
    out = np.zeros(1, render.PROBE_LIGHT_DTYPE)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    dev = torch.zeros(64, dtype=torch.uint8, device="cuda")
    d0, d1 = C.c_void_p(dev.data_ptr()), C.c_void_p(dev.data_ptr() + 32)
    with render.Context(render.make_config(64, 40)) as ctx:
        ctx.upload_noise(blue_noise)                                    # noise, no world
        assert lib.rt_probe_light(ctx.handle, C.byref(u), P(probes), 1, 2, 2, P(out)) == abi.RT_ERR_NOT_READY
        assert lib.rt_probe_light_async(ctx.handle, C.byref(u), d0, 1, 2, 2, d1) == abi.RT_ERR_NOT_READY
        assert lib.rt_probe_light(ctx.handle, C.byref(u), None, 0, 2, 2, None) == abi.RT_OK
    with _ctx(mats, mine) as ctx:                                       # a world, no noise
        assert lib.rt_probe_light(ctx.handle, C.byref(u), P(probes), 1, 2, 2, P(out)) == abi.RT_ERR_NOT_READY
        assert lib.rt_probe_light_async(ctx.handle, C.byref(u), d0, 1, 2, 2, d1) == abi.RT_ERR_NOT_READY
        ctx.upload_noise(blue_noise)
        assert lib.rt_probe_light(ctx.handle, C.byref(u), P(probes), 1, 2, 2, P(out)) == abi.RT_OK
    assert out["light"].any() and not dev.any().item()


# ---- no side effects -----------------------------------------------------------------------------------------------------------
def test_probes_do_not_disturb_accumulating_reprojecting_frames(procedural_region, terrain_probes, blue_noise):
    """An RT_FLAG_ACCUMULATE | RT_FLAG_REPROJECT context with counters: probes between its frames (synchronous, asynchronous, both
    reduction paths) leave the planes, the history counts, the counters and rt_kernel_in_use as in a run without them."""
    mats, mine = procedural_region
    flags = abi.RT_FLAG_ACCUMULATE | abi.RT_FLAG_REPROJECT | abi.RT_FLAG_COUNTERS
    probes_t = _dev(terrain_probes)
    outs = [torch.zeros((len(terrain_probes), 4), dtype=torch.float32, device="cuda") for _ in range(5)]
    torch.cuda.synchronize()
    runs = []
    for interleave in (False, True):
        with _ctx(mats, mine, W, H, noise=blue_noise, spp=1, flags=flags) as ctx:
            for k in range(5):
                pose = dict(TERRAIN_POSE, heading=TERRAIN_POSE["heading"] + (0.01 if k >= 3 else 0.0))   # still, then moved
                u = _u(pose, 50 + k)
                ctx.draw_frame(u)
                if interleave:
                    ctx.probe_light_async(u, probes_t, outs[k], 4 + (k & 1), 3)      # no host wait
                    if k == 2:
                        ctx.probe_records(u, terrain_probes[:100], 3, 2)
            ctx.sync()
            runs.append((ctx.readback_all(), ctx.read_history(), ctx.accumulation(), ctx.counters().as_dict(), ctx.kernel_in_use()))
            if interleave:
                want = [ctx.probe_records(_u(TERRAIN_POSE, 50 + k), terrain_probes, 4 + (k & 1), 3) for k in range(3)]
    (p0, h0, a0, c0, k0), (p1, h1, a1, c1, k1) = runs
    for name in p0:
        assert p0[name].tobytes() == p1[name].tobytes(), name
    assert h0.tobytes() == h1.tobytes() and h0.max() > 1
    assert a0 == a1 and c0 == c1 and k0 == k1
    for k in range(3):
        assert _host(outs[k]).tobytes() == want[k].tobytes()
