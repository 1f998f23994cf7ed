"""The history-aware denoise on the GPU (rt_denoise_history, rt_denoise_planes_counted, Pipeline.enable_history_denoise): bit for bit
against tests/denoise_history_ref.py, which tests/test_denoise_history_contract.py anchors to the oracle on the CPU."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from raytrace_amd import _lib, abi, render
from tests import denoise_history_ref as ref

pytestmark = pytest.mark.gpu

ACC, REP, CACHE, FIF2 = abi.RT_FLAG_ACCUMULATE, abi.RT_FLAG_REPROJECT, abi.RT_FLAG_CACHE_PRIMARY, abi.RT_FLAG_FRAMES_IN_FLIGHT_2
PRESET = (0, 16, 8, 4, 4, 2)
ODD = (0, 0, 127, 1, 0, 5)
SETTLES = (ref.NEUTRAL, PRESET, ODD)
# every (weight, settle, faithful)
COMBOS = tuple((w, s, f) for w in (False, True) for s in SETTLES for f in (True, False))

_rendered = {}


def _rendered_planes(W, H, region, noise):
    """The small terrain pose of tests/test_post_passes.py (sky, terrain, silhouettes), from the oracle."""
    if (W, H) not in _rendered:
        u = po.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.25, 0.3, 9)
        p = po.render(region[0], region[1], noise, u, W, H, 1, 2)[0]
        _rendered[(W, H)] = (p["lighting_rgba16"], p["depth_r16"], p["normal_r8"])
    return _rendered[(W, H)]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(torch.device("cuda", 0))


def _run_counted(ctx, lighting, depth_t, normal_t, counts_t, params):
    import torch
    light_t = _dev(lighting)
    torch.cuda.synchronize()
    ctx.denoise_planes_counted(light_t.data_ptr(), depth_t.data_ptr(), normal_t.data_ptr(), counts_t.data_ptr(), params)
    ctx.sync()
    return light_t.cpu().numpy().view(np.uint16).reshape(lighting.shape)


# ---- 5. planes against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", ["edge", "random"])
@pytest.mark.parametrize("planes", ["rendered", "random"])
@pytest.mark.parametrize("W,H", [(333, 77), (40, 30)])
def test_counted_planes_match_the_reference(procedural_region, blue_noise, monkeypatch, W, H, planes, counts):
    """333x77 is no multiple of the 32x8 tile, 40x30 is smaller than the halos of sizes 8 and 16; synthetic counts sit on every clamp
    and threshold (0, 1, 2, 7, 8, 126, 127, 128, 2^24, 2^27 - 1) or are random in 0..200; the LDS-tiled dispatches and the direct
    ones (RT_DENOISE_UNTILED) must both give the reference's bits."""
    lighting, depth, normal = _rendered_planes(W, H, procedural_region, blue_noise) if planes == "rendered" else ref.random_planes(H, W)
    cnt = ref.edge_counts(H, W) if counts == "edge" else ref.random_counts(H, W)
    depth_t, normal_t, counts_t = _dev(depth), _dev(normal), _dev(cnt)
    changed = 0
    with render.Context(render.make_config(W, H)) as ctx:
        for weight, settle, faithful in COMBOS:
            want = ref.denoise(lighting, depth, normal, faithful, cnt, weight, settle)
            changed += int(not np.array_equal(want, po.denoise(lighting, depth, normal, faithful)))
            params = render.denoise_params(faithful, weight, settle)
            for untiled in (False, True):
                if untiled:
                    monkeypatch.setenv("RT_DENOISE_UNTILED", "1")
                else:
                    monkeypatch.delenv("RT_DENOISE_UNTILED", raising=False)
                got = _run_counted(ctx, lighting, depth_t, normal_t, counts_t, params)
                assert np.array_equal(got, want), (weight, settle, faithful, untiled, int(np.count_nonzero(got != want)))
    assert changed == len(COMBOS) - 2   # the counts matter: only the neutral parameters (either binding) give plain denoise


# ---- 6. neutral parameters, all settled --------------------------------------------------------------------------------------------
def _ctx(region, noise, W=96, H=64, flags=ACC | REP | CACHE, **kw):
    ctx = render.Context(render.make_config(W, H, spp=1, depth=2, flags=flags, **kw))
    ctx.upload_world(*region)
    ctx.upload_noise(noise)
    return ctx


def _pose(k, step):
    return po.camera_uniforms((-30.0 + 0.25 * step, -128.0, 100.0), np.pi / 2 + 0.002 * step, -0.1, 0.3, 5 + k)


@pytest.mark.parametrize("faithful", [True, False])
def test_neutral_parameters_are_rt_denoise_and_all_settled_is_the_identity(procedural_region, blue_noise, faithful):
    import torch
    W, H = 96, 64
    with _ctx(procedural_region, blue_noise) as ctx:
        ctx.draw_frame(_pose(0, 0))
        g = ctx.readback_all()
        assert (ctx.read_history() == 1).all()
        depth_t, normal_t = _dev(g["depth_r16"]), _dev(g["normal_r8"])
        plain_t = _dev(g["lighting_rgba16"])
        torch.cuda.synchronize()
        ctx.denoise_planes(plain_t.data_ptr(), depth_t.data_ptr(), normal_t.data_ptr(), faithful=faithful)
        ctx.sync()
        plain = plain_t.cpu().numpy().view(np.uint16).reshape(H, W, 4)
        assert np.array_equal(plain, po.denoise(g["lighting_rgba16"], g["depth_r16"], g["normal_r8"], faithful))
        # settle all 0 without weighting, on the frame's own counts
        ctx.denoise_history(render.denoise_params(faithful))
        assert np.array_equal(ctx.readback(abi.RT_BUF_LIGHTING_RGBA16), plain)
        # the next (still) frame rewrites the lighting plane; its counts are 2 everywhere
        ctx.draw_frame(_pose(1, 0))
        g2 = ctx.readback_all()
        assert (ctx.read_history() == 2).all()
        # weighting with every count 1 changes nothing: the multiplies are by 1.0f
        ones_t = _dev(np.ones((H, W), dtype=np.uint32))
        got = _run_counted(ctx, g["lighting_rgba16"], depth_t, normal_t, ones_t, render.denoise_params(faithful, True))
        assert np.array_equal(got, plain)
        # all settled: nobody filters, the plane comes back as it was, alpha included (planes, then the context's own frame)
        settled = render.denoise_params(faithful, True, (1,) * 6)
        cnt_t = _dev(ref.edge_counts(H, W))
        assert np.array_equal(_run_counted(ctx, g["lighting_rgba16"], depth_t, normal_t, cnt_t, settled), g["lighting_rgba16"])
        ctx.denoise_history(settled)
        assert np.array_equal(ctx.readback(abi.RT_BUF_LIGHTING_RGBA16), g2["lighting_rgba16"])
        assert (g2["lighting_rgba16"][..., 3] == 4096).all()


# ---- 7. rt_denoise_history on a reprojecting context -------------------------------------------------------------------------------
SEQUENCE = (0, 0, 0, 0, 1, 2)   # pose of frame k: a restart, three still frames, two moved ones
FRAME_PARAMS = ((False, PRESET, True), (True, ref.NEUTRAL, False), (True, PRESET, True), (False, ODD, False), (True, (0, 0, 16, 8, 4, 4), True),
                (False, PRESET, False))


def test_denoise_history_follows_the_history_and_leaves_it_alone(procedural_region, blue_noise):
    with _ctx(procedural_region, blue_noise) as ctx, _ctx(procedural_region, blue_noise) as twin:
        seen = set()
        for k, step in enumerate(SEQUENCE):
            u = _pose(k, step)
            ctx.draw_frame(u)
            twin.draw_frame(u)
            g, counts = ctx.readback_all(), ctx.read_history()
            t, tcounts = twin.readback_all(), twin.read_history()
            # the denoise of the frames before disturbed neither the sums nor the counts
            assert np.array_equal(counts, tcounts), k
            assert np.array_equal(g["lighting_f32"], t["lighting_f32"]) and np.array_equal(g["lighting_rgba16"], t["lighting_rgba16"]), k
            weight, settle, faithful = FRAME_PARAMS[k]
            ctx.denoise_history(render.denoise_params(faithful, weight, settle))
            got = ctx.readback(abi.RT_BUF_LIGHTING_RGBA16)
            want = ref.denoise(g["lighting_rgba16"], g["depth_r16"], g["normal_r8"], faithful, counts, weight, settle)
            assert np.array_equal(got, want), (k, int(np.count_nonzero(got != want)))
            # lighting_f32, the counts and the other planes are as they were
            after = ctx.readback_all()
            for name in g:
                if name != "lighting_rgba16":
                    assert np.array_equal(after[name], g[name], equal_nan=True), (k, name)
            assert np.array_equal(ctx.read_history(), counts)
            seen |= set(np.unique(counts).tolist())
        assert {1, 2, 3, 4, 5}.issubset(seen) and len(np.unique(counts)) > 2   # still frames counted up, moved frames mixed them


# ---- 8. two frames in flight -------------------------------------------------------------------------------------------------------
def test_two_frames_in_flight_read_their_own_counts(procedural_region, blue_noise):
    """draw, denoise, draw, denoise, draw, denoise without a sync between: each denoise reads the records its frame's pass wrote, and
    the frame after next, which overwrites that set, starts behind it.  rt_create accepts the two flags together."""
    params = render.denoise_params(True, True, PRESET)
    poses = [_pose(k, k) for k in range(3)]
    with _ctx(procedural_region, blue_noise, flags=ACC | REP | CACHE | FIF2) as ctx:
        assert ctx.info().frames_in_flight == 2
        for u in poses:
            ctx.draw_frame(u)
            ctx.denoise_history(params)
        got = ctx.readback(abi.RT_BUF_LIGHTING_RGBA16)
        counts = ctx.read_history()
    with _ctx(procedural_region, blue_noise) as one:
        for u in poses:
            one.draw_frame(u)
            one.sync()
            one.denoise_history(params)
            one.sync()
        want = one.readback(abi.RT_BUF_LIGHTING_RGBA16)
        assert np.array_equal(one.read_history(), counts) and len(np.unique(counts)) > 1
    assert np.array_equal(got, want), int(np.count_nonzero(got != want))


# ---- 9. the mirror, and the error codes --------------------------------------------------------------------------------------------
def test_the_mirror_draws_with_the_history_denoise(procedural_region, blue_noise):
    W, H = 96, 64
    cfg = render.make_config(W, H, spp=1, depth=2, flags=ACC | REP | CACHE)
    params = render.denoise_params(True, True, PRESET)
    g = render.Game(args=(-30, -128, 100, 1.5707964, -0.15, 0.3))
    g.set_world(*procedural_region)
    p = render.create_instance(cfg, g, blue_noise)
    p.enable_post_passes(faithful=True)
    p.enable_history_denoise(params)
    uniforms = []
    for k in range(4):
        g.borrow_camera().set(origin=(-30.0 + 0.25 * max(k - 1, 0), -128.0, 100.0))   # one still frame, then moves
        p.draw_frame(g)
        p.wait()
        uniforms.append(abi.RtUniforms.from_buffer_copy(bytes(p.uniforms())))
    final = p.context.readback(abi.RT_BUF_FINAL_BGRA8)
    counts = p.context.read_history()
    p.close()
    with _ctx(procedural_region, blue_noise) as ctx:
        for u in uniforms:
            ctx.draw_frame(u)
            ctx.denoise_history(params)
            ctx.finalize()
        assert np.array_equal(ctx.read_history(), counts) and len(np.unique(counts)) > 1
        assert np.array_equal(ctx.readback(abi.RT_BUF_FINAL_BGRA8), final)
    # refused on a pipeline whose context does not reproject, and for a block rt_denoise_history would refuse
    p2 = render.create_instance(render.make_config(W, H, spp=1, depth=2, flags=CACHE), g, blue_noise)
    p2.enable_post_passes()
    with pytest.raises(render.RtError) as e:
        p2.enable_history_denoise(params)
    assert e.value.code == abi.RT_ERR_INVALID_ARG
    p2.close()
    p3 = render.create_instance(cfg, g, blue_noise)
    bad = render.denoise_params(True, False, PRESET)
    bad.settle[2] = 128
    with pytest.raises(render.RtError) as e:
        p3.enable_history_denoise(bad)
    assert e.value.code == abi.RT_ERR_INVALID_ARG
    p3.close()
    g.close()


def _bad_blocks():
    out = []
    for field, value in (("struct_size", 44), ("weight_by_count", 2), ("weight_by_count", -1)):
        p = render.denoise_params()
        setattr(p, field, value)
        out.append(p)
    p = render.denoise_params()
    p.settle[5] = 128
    out.append(p)
    p = render.denoise_params()
    p.reserved[2] = 1
    out.append(p)
    return out


def test_error_codes_of_both_entry_points(procedural_region, blue_noise):
    import torch
    lib = _lib.amd()
    W, H = 96, 64
    good = render.denoise_params(True, False, PRESET)
    planes = [_dev(np.zeros(W * H * n, dtype=np.uint8)) for n in (8, 2, 1, 4)]   # lighting, depth, normal, counts
    ptrs = [C.c_void_p(t.data_ptr()) for t in planes]
    torch.cuda.synchronize()
    with _ctx(procedural_region, blue_noise) as ctx:
        h = ctx.handle
        assert lib.rt_denoise_history(h, C.byref(good)) == abi.RT_ERR_NOT_READY
        for bad in _bad_blocks():   # a bad block is RT_ERR_INVALID_ARG, drawn frame or not
            assert lib.rt_denoise_history(h, C.byref(bad)) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_denoise_history(h, None) == abi.RT_ERR_INVALID_ARG
        ctx.draw_frame(_pose(0, 0))
        before = ctx.readback(abi.RT_BUF_LIGHTING_RGBA16)
        for bad in _bad_blocks():
            assert lib.rt_denoise_history(h, C.byref(bad)) == abi.RT_ERR_INVALID_ARG
            assert b"rt_denoise_history" in lib.rt_last_error(h)
            assert lib.rt_denoise_planes_counted(h, *ptrs, C.byref(bad)) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_denoise_history(h, None) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_denoise_planes_counted(h, *ptrs, None) == abi.RT_ERR_INVALID_ARG
        for missing in range(4):
            args = list(ptrs)
            args[missing] = None
            assert lib.rt_denoise_planes_counted(h, *args, C.byref(good)) == abi.RT_ERR_INVALID_ARG
        assert np.array_equal(ctx.readback(abi.RT_BUF_LIGHTING_RGBA16), before)   # nothing was enqueued
        assert lib.rt_denoise_history(h, C.byref(good)) == abi.RT_OK
        ctx.sync()
    with _ctx(procedural_region, blue_noise, flags=ACC | CACHE) as ctx:   # accumulates, does not reproject
        ctx.draw_frame(_pose(0, 0))
        assert lib.rt_denoise_history(ctx.handle, C.byref(good)) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_denoise_planes_counted(ctx.handle, *ptrs, C.byref(good)) == abi.RT_OK   # valid on any context
        ctx.sync()
    with _ctx(procedural_region, blue_noise, flags=CACHE, tile_rank=0, tile_world=2) as ctx:
        ctx.draw_frame(_pose(0, 0))
        assert lib.rt_denoise_history(ctx.handle, C.byref(good)) == abi.RT_ERR_UNIMPLEMENTED
        ctx.sync()
