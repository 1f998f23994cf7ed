"""GPU parity on noise textures other than the blue-noise fixture (tests/adversarial_noise.py), everything bit for bit against the
oracle with coinciding NaN patterns: frames that read every (r, g) byte pair — every entry of sphere_lut, dif_lut and sun_lut, the
256 NaN entries of face 5 and the 1 / |d.z| = inf entries of face 4 included — exactly once, on every route; sun changes on one
context; the reference's one-sample route frame by frame; light probes (k_probe computes its directions itself) over all entries;
constant, extreme and random textures on ordinary scenes; a second upload that differs from the first; finalize's dither.
tests/test_adversarial_noise.py checks on the CPU that these inputs are what they are meant to be."""
import numpy as np
import pytest

from oracle import pyoracle as po
from raytrace_amd import abi, render, world
from tests import adversarial_noise as an
from tests import adversarial_worlds as aw
from tests import scenes
from tests import synthetic_planes as sp_planes
from tests.test_gpu_parity import _cached_counters, _compare

pytestmark = pytest.mark.gpu

C, CACHE, FIF2 = abi.RT_FLAG_COUNTERS, abi.RT_FLAG_CACHE_PRIMARY, abi.RT_FLAG_FRAMES_IN_FLIGHT_2
# the routes of tests/test_gpu_fuzz.py, plus the split wavefront baseline
ROUTES = [(abi.RT_KERNEL_PERSISTENT, C), (abi.RT_KERNEL_PERSISTENT, CACHE), (abi.RT_KERNEL_PATHS, CACHE), (abi.RT_KERNEL_FRAME, CACHE),
          (abi.RT_KERNEL_MEGA, C), (abi.RT_KERNEL_WAVEFRONT, C)]
TABLE_KERNELS = {abi.RT_KERNEL_PERSISTENT, abi.RT_KERNEL_PATHS, abi.RT_KERNEL_FRAME}
W, H, SPP = an.LATTICE_FRAME
SEED0 = an.LATTICE_SEED0
WORLD_DEPTH = {"plain": 2, "shell": 4}

_FRAMES = {}


@pytest.fixture(scope="module")
def lattice(native_built):
    T = an.lattice_noise()
    T.setflags(write=False)
    return T


def _view(face):
    return [v for v in an.FACE_VIEWS if v[0] == face][0]


def _lattice_frame(face, world_name, lattice):
    """(uniforms, oracle planes, oracle counters) of the lattice frame of a face view under the face's sun: computed once, shared."""
    key = (face, world_name)
    if key not in _FRAMES:
        mats, mine = an.cube_world(world_name == "shell")
        u = an.view_uniforms(po, _view(face), an.FACE_SUN[face])
        _FRAMES[key] = (u,) + po.render(mats, mine, lattice, u, W, H, SPP, WORLD_DEPTH[world_name])
    return _FRAMES[key]


def _draw_routes(mats, mine, noise, frames, width, height, spp, depth, routes=ROUTES):
    """Every route draws every frame of `frames` ((uniforms, oracle planes, oracle counters) each) on one context per route: planes
    bit for bit, counters exact on the counting routes.  Returns the set of kernels that ran."""
    used = set()
    for kernel, flags in routes:
        with render.Context(render.make_config(width, height, spp=spp, depth=depth, kernel=kernel, flags=flags)) as ctx:
            ctx.upload_world(mats, mine)
            ctx.upload_noise(noise)
            for i, (u, cpu, ccn) in enumerate(frames):
                ctx.reset_counters()
                ctx.draw_frame(u)
                ctx.sync()
                gpu, gcn = ctx.readback_all(), ctx.counters()
                try:
                    _compare(gpu, cpu)
                except AssertionError as e:
                    raise AssertionError("frame %d, kernel %d, flags %#x: %s" % (i, kernel, flags, e))
                if flags & C:
                    want = _cached_counters(mats, mine, noise, u, width, height, spp, depth, ccn) if flags & CACHE else ccn.as_dict()
                    got = gcn.as_dict()
                    assert got == want, (i, kernel, flags, {k: (got[k], want[k]) for k in got if got[k] != want[k]})
            used.add(ctx.kernel_in_use())
    return used


@pytest.mark.parametrize("world_name", ["plain", "shell"])
@pytest.mark.parametrize("face", [4, 5, 1, 0, 3, 2])
def test_every_table_entry_on_every_route(face, world_name, lattice):
    """A 16 x 16 frame of 256 samples on the lattice texture: each of the 65 536 (r, g) pairs indexes the tables of the view's face
    exactly once at level 1 (the shell world's deeper levels stand on the other faces as well)."""
    mats, mine = an.cube_world(world_name == "shell")
    u, cpu, ccn = _lattice_frame(face, world_name, lattice)
    assert (cpu["normal_r8"] == face).all()
    used = _draw_routes(mats, mine, lattice, [(u, cpu, ccn)], W, H, SPP, WORLD_DEPTH[world_name])
    assert TABLE_KERNELS <= used, used
    if face == 5:     # the NaN entries were taken: each of the 256 starts a level at a NaN position (border fetches, lr = 0)
        assert ccn.border_fetches >= 5 * 256


def test_sun_changes_on_one_context(lattice):
    """The per-frame tables (sun_lut, the sky slot of dif_lut) follow the sun: the shell world's face-4 view at sun 0.6, -2.2, 0.6 and
    -0.6 (the last differs from the one before by sign alone: a rebuild keyed on the angle's magnitude would keep the sky slot) on
    one context."""
    mats, mine = an.cube_world(True)
    frames = []
    for sun in (0.6, -2.2, 0.6, -0.6):
        u = an.view_uniforms(po, _view(4), sun)
        frames.append((u,) + po.render(mats, mine, lattice, u, W, H, SPP, 4))
    lit = [f[2].sky_exits for f in frames]
    assert lit[0] == lit[2] and len({lit[0], lit[1], lit[3]}) == 3
    assert not np.array_equal(frames[0][1]["lighting_f32"], frames[3][1]["lighting_f32"])
    used = _draw_routes(mats, mine, lattice, frames, W, H, SPP, 4, routes=[(abi.RT_KERNEL_PATHS, CACHE), (abi.RT_KERNEL_FRAME, CACHE)])
    assert used == {abi.RT_KERNEL_PATHS, abi.RT_KERNEL_FRAME}


@pytest.mark.parametrize("face", [4, 5])
def test_reference_route_frame_by_frame(face, lattice):
    """One sample per frame, depth 2 — the reference's own frames — with seeds seed0 .. seed0 + 255: together the 256 frames read
    every pair once.  RT_KERNEL_DEFAULT and RT_KERNEL_FRAME contexts, every frame compared; then the same frames on a context with two
    frames in flight, drawn without a sync between them and read back after each."""
    mats, mine = an.cube_world(True)
    us = [an.view_uniforms(po, _view(face), an.FACE_SUN[face], seed=SEED0 + s) for s in range(SPP)]
    cpus = [po.render(mats, mine, lattice, u, W, H, 1, 2)[0] for u in us]
    assert len({c["lighting_f32"].tobytes() for c in cpus}) > 200          # the frames do differ with the seed
    for kernel, flags, sync in ((abi.RT_KERNEL_DEFAULT, 0, True), (abi.RT_KERNEL_FRAME, CACHE, True), (abi.RT_KERNEL_DEFAULT, FIF2, False)):
        with render.Context(render.make_config(W, H, spp=1, depth=2, kernel=kernel, flags=flags)) as ctx:
            ctx.upload_world(mats, mine)
            ctx.upload_noise(lattice)
            for s, (u, cpu) in enumerate(zip(us, cpus)):
                ctx.draw_frame(u)
                if sync:
                    ctx.sync()
                try:
                    _compare(ctx.readback_all(), cpu)
                except AssertionError as e:
                    raise AssertionError("seed0 + %d, kernel %d, flags %#x: %s" % (s, kernel, flags, e))
            assert ctx.kernel_in_use() == abi.RT_KERNEL_FRAME


@pytest.mark.parametrize("world_name", ["plain", "shell"])
@pytest.mark.parametrize("face", [4, 5, 1, 0, 3, 2])
def test_probes_over_every_entry(face, world_name, lattice):
    """rt_probe_light at the 256 pixels' surfaces with the pixels' workgroups as cells and 256 samples: light / 16 is the lighting of
    the oracle's frame.  k_probe evaluates diffuse_direction on the device: this holds that build to all entries as well."""
    mats, mine = an.cube_world(world_name == "shell")
    depth = WORLD_DEPTH[world_name]
    u, cpu, _ = _lattice_frame(face, world_name, lattice)
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2)
    with render.Context(render.make_config(W, H)) as ctx:
        ctx.upload_world(mats, mine)
        ctx.upload_noise(lattice)
        hits = ctx.pick_pixels(u, xy)
        assert (hits["kind"] != abi.RT_HIT_AIR).all() and (hits["normal"] == face).all()
        cells = np.stack([render.workgroup_of(xy[:, 0]), render.workgroup_of(xy[:, 1])], axis=-1)
        got = ctx.probe_records(u, render.make_probes(hits["position"], hits["normal"], cells), SPP, depth)
    want = cpu["lighting_f32"][xy[:, 1], xy[:, 0], :3]
    light = got["light"] / np.float32(16.0)
    assert np.array_equal(np.isnan(light), np.isnan(want))
    assert np.array_equal(light, want, equal_nan=True), int(np.count_nonzero(light.view(np.uint32) != want.view(np.uint32)))


TEXTURES = {"zero": lambda: an.constant_noise(0, 0), "ones": lambda: an.constant_noise(255, 255), "r0_g255": lambda: an.constant_noise(0, 255),
            "extreme": lambda: an.extreme_noise(3), "random": lambda: an.random_noise(4)}
BLOCKS_POSES = [dict(origin=(-60.0, -90.0, -60.0), heading=0.9, pitch=-0.35, sun=0.6, lr=(0, 0, 0)),
                dict(origin=(-40.0, -100.0, 90.0), heading=1.1, pitch=-0.5, sun=0.3, lr=(0, 0, 0))]
_SCENES = {}


def _scene(name):
    if name not in _SCENES:
        _SCENES[name] = world.region_from_ids(scenes.random_blocks_ids()) if name == "blocks" else aw.arbitrary_world(256)[:2]
    return _SCENES[name]


@pytest.mark.parametrize("scene", ["blocks", "arbitrary"])
@pytest.mark.parametrize("texture", list(TEXTURES))
def test_degenerate_and_random_textures_on_ordinary_scenes(texture, scene, native_built):
    """Constant (0, 0) — every diffuse ray off a face-5 surface NaN —, (255, 255) — every one off face 4 along the surface —,
    (0, 255), bytes from {0, 1, 127, 128, 254, 255} and uniform bytes, on the blocks scene (it has ceilings) and the arbitrary
    world; the second pose of the arbitrary world has lr != 0 (k_persist's scrolled build)."""
    mats, mine = _scene(scene)
    noise = TEXTURES[texture]()
    width, height, spp, depth = 73, 40, 4, 3
    poses = BLOCKS_POSES if scene == "blocks" else [aw.POSES[0], aw.POSES[4]]
    frames = []
    for i, pose in enumerate(poses):
        u = po.camera_uniforms(pose["origin"], pose["heading"], pose["pitch"], pose["sun"], 1000 * i + 77, pose["lr"])
        frames.append((u,) + po.render(mats, mine, noise, u, width, height, spp, depth))
        assert (frames[-1][1]["normal_r8"] != 16).mean() > 0.3            # the frame hits geometry
    if texture == "zero":   # diffuse rays go straight up off face 4 and are NaN off the ceilings they reach: thousands of levels start
        assert frames[0][2].border_fetches > 5000                         # at a NaN position (the other textures' frames: a few hundred)
    used = _draw_routes(mats, mine, noise, frames, width, height, spp, depth)
    assert TABLE_KERNELS <= used, used


@pytest.mark.parametrize("kernel", [abi.RT_KERNEL_PATHS, abi.RT_KERNEL_FRAME, abi.RT_KERNEL_DEFAULT])
def test_new_noise_replaces_old(kernel, native_built):
    """Two random textures on a context with two frames in flight: upload A, draw, upload B without waiting for the frame, draw.  The
    first frame is the oracle's with A (the upload did not overtake it), the second the oracle's with B; A again gives the first."""
    mats, mine = _scene("blocks")
    A, B = an.random_noise(11), an.random_noise(12)
    width, height, spp, depth = 73, 40, 4, 3
    pose = BLOCKS_POSES[0]
    u = po.camera_uniforms(pose["origin"], pose["heading"], pose["pitch"], pose["sun"], 5, pose["lr"])
    cpu_a, cpu_b = (po.render(mats, mine, n, u, width, height, spp, depth)[0] for n in (A, B))
    assert not np.array_equal(cpu_a["lighting_f32"], cpu_b["lighting_f32"], equal_nan=True)
    with render.Context(render.make_config(width, height, spp=spp, depth=depth, kernel=kernel, flags=CACHE | FIF2)) as ctx:
        ctx.upload_world(mats, mine)
        ctx.upload_noise(A)
        ctx.draw_frame(u)
        ctx.upload_noise(B)
        _compare(ctx.readback_all(), cpu_a)
        ctx.draw_frame(u)
        _compare(ctx.readback_all(), cpu_b)
        ctx.upload_noise(A)
        ctx.draw_frame(u)
        ctx.sync()
        _compare(ctx.readback_all(), cpu_a)


@pytest.mark.parametrize("texture", ["random", "extreme"])
def test_finalize_dither_with_other_textures(texture, blue_noise, native_built):
    """The method of test_gpu_adversarial_worlds.test_post_passes_on_synthetic_planes at 333 x 77: k_finalize's dither reads the
    uploaded texture (all four channels' worth of texels, the frame's own addressing), against po.finalize with the same one."""
    import torch
    width, height = 333, 77
    noise = TEXTURES[texture]()
    p = sp_planes.post_planes(width, height, seed=width * 7 + height)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(dev)
    depth, normal, albedo, emission, fog = t(p["depth"]), t(p["normal"]), t(p["albedo"]), t(p["emission"]), t(p["fog"])
    out = torch.zeros(width * height * 4, dtype=torch.uint8, device=dev)
    with render.Context(render.make_config(width, height)) as ctx:
        ctx.upload_noise(blue_noise)    # the texture that must not be used
        ctx.upload_noise(noise)
        for faithful in (True, False):
            exp_den = po.denoise(p["lighting"], p["depth"], p["normal"], faithful=faithful)
            exp_fin = po.finalize(p["albedo"], p["emission"], p["fog"], exp_den, p["depth"], noise)
            assert not np.array_equal(exp_fin, po.finalize(p["albedo"], p["emission"], p["fog"], exp_den, p["depth"], blue_noise))
            lighting = t(p["lighting"])
            out.zero_()
            torch.cuda.synchronize()
            ctx.denoise_planes(lighting.data_ptr(), depth.data_ptr(), normal.data_ptr(), faithful=faithful)
            ctx.finalize_planes(albedo.data_ptr(), emission.data_ptr(), fog.data_ptr(), lighting.data_ptr(), depth.data_ptr(), out.data_ptr())
            ctx.sync()
            den = lighting.cpu().numpy().view(np.uint16).reshape(height, width, 4)
            fin = out.cpu().numpy().reshape(height, width, 4)
            assert np.array_equal(den, exp_den), ("denoise", faithful, int(np.count_nonzero(den != exp_den)))
            assert np.array_equal(fin, exp_fin), ("finalize", faithful, int(np.count_nonzero(fin != exp_fin)))
