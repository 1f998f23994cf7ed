"""The history-aware denoise on the CPU: its numpy restatement (tests/denoise_history_ref.py) anchored to the oracle's six dispatches,
what settle and weight_by_count do to single pixels, the measured quality of the shipped preset, and the parts of the C ABI that need
no device."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from raytrace_amd import _lib, abi, render
from tests import denoise_history_ref as ref

ALL_SETTLED = (1, 1, 1, 1, 1, 1)


# ---- 1. anchor ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(40, 56), (77, 333)])
def test_neutral_parameters_are_the_oracle_bit_for_bit(h, w):
    lighting, depth, normal = ref.random_planes(h, w)
    assert (normal == 16).any() and (depth < 16).any()
    ones = np.ones((h, w), dtype=np.uint32)
    for faithful in (True, False):
        want = po.denoise(lighting, depth, normal, faithful)
        got = ref.denoise(lighting, depth, normal, faithful)
        assert np.array_equal(got, want), (faithful, int(np.count_nonzero(got != want)))
        if h == 40:   # counts all 1 with weight_by_count: every multiply is by 1.0f
            got = ref.denoise(lighting, depth, normal, faithful, counts=ones, weight_by_count=True)
            assert np.array_equal(got, want), ("counts 1", faithful, int(np.count_nonzero(got != want)))
    # the pong dispatches filtered the near patch: the two bindings differ there
    assert not np.array_equal(po.denoise(lighting, depth, normal, True)[:5, :7], po.denoise(lighting, depth, normal, False)[:5, :7])


def test_all_settled_returns_the_input_alpha_included():
    lighting, depth, normal = ref.random_planes(40, 56)
    counts = ref.random_counts(40, 56)   # holds zeros: m = 1 settles at 1 too
    assert (counts == 0).any()
    for weight in (False, True):
        got = ref.denoise(lighting, depth, normal, True, counts=counts, weight_by_count=weight, settle=ALL_SETTLED)
        assert np.array_equal(got, lighting)


# ---- 2. properties -----------------------------------------------------------------------------------------------------------------
def _flat(h=24, w=24, value=20000, outlier=40000):
    lighting = np.zeros((h, w, 4), dtype=np.uint16)
    lighting[..., :3] = value
    lighting[..., 3] = 4096
    lighting[12, 12, :3] = outlier
    return lighting, np.full((h, w), 800, dtype=np.uint16), np.full((h, w), 4, dtype=np.uint8)


def test_a_fresh_pixel_among_converged_neighbours_moves_to_them_and_a_converged_one_stays():
    lighting, depth, normal = _flat()
    fresh = np.full(depth.shape, 100, dtype=np.uint32)
    fresh[12, 12] = 1
    plain = ref.denoise(lighting, depth, normal, False).astype(np.int64)
    got = ref.denoise(lighting, depth, normal, False, counts=fresh, weight_by_count=True).astype(np.int64)
    # the outlier has 1 sample, its neighbours 100: its own weight is a hundredth of a neighbour's
    assert abs(got[12, 12, 0] - 20000) < abs(plain[12, 12, 0] - 20000)
    assert abs(got[12, 12, 0] - 20000) <= 40, got[12, 12, 0]
    assert abs(got[12, 13, 0] - 20000) < abs(plain[12, 13, 0] - 20000)     # and it pulls on them a hundred times less
    # the other way round: the outlier is the one with 100 samples, everybody else has 1
    old = np.ones(depth.shape, dtype=np.uint32)
    old[12, 12] = 100
    got = ref.denoise(lighting, depth, normal, False, counts=old, weight_by_count=True).astype(np.int64)
    assert abs(got[12, 12, 0] - 40000) < abs(plain[12, 12, 0] - 40000)     # it moves less than under plain denoise


def test_a_settled_pixel_is_unchanged_by_its_dispatch_and_still_read_as_a_tap():
    lighting, depth, normal = _flat()
    counts = np.ones(depth.shape, dtype=np.uint32)
    counts[12, 12] = 50
    m = ref.clamp_counts(counts)
    v0, c0 = ref.start(lighting)
    for size in (1, 4):
        v1, c1 = ref.dispatch(v0, c0, depth, normal, size, False, m, False, settle=50)
        plain, _ = ref.dispatch(v0, c0, depth, normal, size)
        assert np.array_equal(v1[12, 12], v0[12, 12]) and not c1[12, 12]                  # passed through, not marked computed
        assert c1[12, 12 + size] and not np.array_equal(v1[12, 12 + size], v0[12, 12 + size])   # its neighbour saw the outlier
        others = np.ones(depth.shape, dtype=bool)
        others[12, 12] = False
        assert np.array_equal(v1[others], plain[others])                                  # and exactly as plain denoise does
        v2, _ = ref.dispatch(v0, c0, depth, normal, size, False, m, False, settle=51)     # one above its count: it filters
        assert np.array_equal(v2, plain)
    # a never-filtered pixel keeps the input alpha through the whole chain
    out = ref.denoise(lighting, depth, normal, False, counts=counts, settle=(50,) * 6)
    assert out[12, 12, 3] == 4096 and tuple(out[12, 12, :3]) == (40000,) * 3 and (out[..., 3] == 65535).sum() == depth.size - 1
    # ... and settling ignores the normal binding: a sky pixel (copy branch anyway) and a surface pixel behave alike
    sky = normal.copy()
    sky[12, 12] = 16
    assert np.array_equal(ref.denoise(lighting, depth, sky, False)[12, 12], out[12, 12])


# ---- 3. quality --------------------------------------------------------------------------------------------------------------------
def test_the_preset_lowers_the_error_against_a_converged_frame(procedural_region, blue_noise):
    """24 one-sample frames of a slowly moving camera through the reprojection restatement, then the last frame denoised four ways
    and compared with the same camera's 256-sample frame (RMS of lighting_rgba16 / 65535 - lighting_f32.rgb, i.e. light / 16 units).
    The committed preset must beat plain denoise over all surface pixels and over those with 8 samples or more, in both bindings.

    Measured (consistent | faithful binding), also in DESIGN.md:
                                              all surface        counts >= 8        counts <= 2
        undenoised                            0.0234             0.0238             0.0206
        plain denoise                         0.0328 | 0.0292    0.0387 | 0.0344    0.0278 | 0.0235
        weight 0, settle 0,16,8,4,4,2         0.0299 | 0.0272    0.0306 | 0.0286    0.0280 | 0.0237
        weight 1, settle 0,0,16,8,4,4         0.0343 | 0.0300    0.0273 | 0.0254    0.0408 | 0.0344"""
    scene = ref.quality_scene(procedural_region, blue_noise)
    L, d, n, counts = scene["lighting"], scene["depth"], scene["normal"], scene["counts"]
    surface = n < 16
    assert (surface & (counts >= 8)).sum() > 500 and (surface & (counts <= 2)).sum() > 100   # both populations are there
    preset = render.HISTORY_DENOISE_PRESET
    print("undenoised", ref.rms_errors(L, scene))
    for faithful in (False, True):
        plain = po.denoise(L, d, n, faithful)
        e_plain = ref.rms_errors(plain, scene)
        e_preset = ref.rms_errors(ref.denoise(L, d, n, faithful, counts, preset["weight_by_count"], preset["settle"]), scene)
        e_weighted = ref.rms_errors(ref.denoise(L, d, n, faithful, counts, True, (0, 0, 16, 8, 4, 4)), scene)
        print("faithful" if faithful else "consistent", "plain", e_plain, "preset", e_preset, "weight 1, settle 0,0,16,8,4,4", e_weighted)
        assert e_preset[0] < e_plain[0], (faithful, e_preset, e_plain)
        assert e_preset[1] < e_plain[1], (faithful, e_preset, e_plain)


# ---- 4. ABI ------------------------------------------------------------------------------------------------------------------------
def test_params_struct_and_what_needs_no_device(native_built):
    assert C.sizeof(abi.RtDenoiseParams) == 48
    offsets = {"struct_size": 0, "faithful": 4, "weight_by_count": 8, "settle": 12, "reserved": 36}
    for name, off in offsets.items():
        assert getattr(abi.RtDenoiseParams, name).offset == off, name
    p = render.denoise_params()
    assert p.struct_size == 48 and p.faithful == 1 and p.weight_by_count == 0 and tuple(p.settle) == (0,) * 6 and tuple(p.reserved) == (0,) * 3
    p = render.denoise_params(faithful=False, **render.HISTORY_DENOISE_PRESET)
    assert p.faithful == 0 and p.weight_by_count == 0 and tuple(p.settle) == (0, 16, 8, 4, 4, 2)
    with pytest.raises(ValueError):
        render.denoise_params(settle=(1, 2, 3))
    lib = _lib.amd()
    assert "rt_denoise_history" in _lib.ABI_SYMBOLS and "rt_denoise_planes_counted" in _lib.ABI_SYMBOLS
    # a null context is RT_ERR_INVALID_ARG whatever else is passed, and nothing is dereferenced
    assert lib.rt_denoise_history(None, None) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_denoise_history(None, C.byref(p)) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_denoise_planes_counted(None, None, None, None, None, None) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_denoise_planes_counted(None, None, None, None, None, C.byref(p)) == abi.RT_ERR_INVALID_ARG
    host = _lib.host()
    assert hasattr(host, "rth_pipeline_enable_history_denoise")
