"""Progressive accumulation (RT_FLAG_ACCUMULATE), the part that needs no GPU: the premise the feature rests on, checked on the
oracle, and the C ABI surface (constant, symbols, null contexts, baselines rejected at rt_create).

The premise: every kernel adds a pixel's samples in sample order starting from 0, so K frames of M samples with seeds s, s + M,
s + 2M, ... whose ordered fp32 sum continues from where the previous frame left it ARE the frame of K*M samples with seed s.  A
one-sample frame's lighting_f32 is ((0 + light) / 1) / 16, so 16 * lighting_f32 is that sample's light exactly."""
import ctypes as C

import numpy as np
import pytest

from raytrace_amd import abi
from oracle import pyoracle as po

W, H = 72, 40
POSE = ((-30.0, -128.0, 100.0), np.pi / 2, -0.05, 0.3)


@pytest.fixture(scope="module")
def region():
    from raytrace_amd import world
    return world.generate_region(world.DEFAULT_SEED)


def _oracle(region, noise, seed, spp, depth):
    mats, mine = region
    origin, heading, pitch, sun = POSE
    return po.render(mats, mine, noise, po.camera_uniforms(origin, heading, pitch, sun, seed), W, H, spp, depth)[0]


def _fold(region, noise, seed0, n, depth):
    """16 * lighting_f32 of n one-sample oracle frames with seeds seed0 .. seed0 + n - 1 (mod RT_NOISE_BYTES), added in float32
    in that order — what an accumulating context sums."""
    acc = None
    for i in range(n):
        light = _oracle(region, noise, (seed0 + i) % abi.NOISE_BYTES, 1, depth)["lighting_f32"][..., :3] * np.float32(16.0)
        acc = light if acc is None else (acc + light).astype(np.float32)
    return acc


def _lighting(acc, n):
    """store_lighting's arithmetic with divisor n: (sum / n) / 16, alpha 1 / 16."""
    out = np.empty(acc.shape[:-1] + (4,), dtype=np.float32)
    out[..., :3] = (acc / np.float32(n)) / np.float32(16.0)
    out[..., 3] = np.float32(1.0 / 16.0)
    return out


@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("seed0", [7, abi.NOISE_BYTES - 2])   # the second run crosses the RT_NOISE_BYTES wrap
def test_five_one_sample_frames_fold_to_the_five_sample_frame(region, blue_noise, depth, seed0):
    acc = _fold(region, blue_noise, seed0, 5, depth)
    want = _oracle(region, blue_noise, seed0, 5, depth)["lighting_f32"]
    assert np.array_equal(_lighting(acc, 5), want, equal_nan=True)


@pytest.mark.parametrize("depth", [2, 4])
def test_three_frames_of_two_samples_fold_to_the_six_sample_frame(region, blue_noise, depth):
    """Three frames of two samples (seeds s, s + 2, s + 4) continuing one ordered sum: that is the fold of six one-sample frames,
    and the oracle's six-sample frame.  (A frame's own two-sample sum added to the previous total would NOT be: fp32 addition is
    not associative, which is why the multi-sample kernels start their sum from the running one.)"""
    seed0 = abi.NOISE_BYTES - 3
    acc = _fold(region, blue_noise, seed0, 6, depth)
    want = _oracle(region, blue_noise, seed0, 6, depth)["lighting_f32"]
    assert np.array_equal(_lighting(acc, 6), want, equal_nan=True)


def test_accumulate_flag_and_its_functions_are_in_the_abi():
    from raytrace_amd import _lib
    assert abi.RT_FLAG_ACCUMULATE == 0x40
    lib = _lib.amd()
    for name in ("rt_reset_accumulation", "rt_get_accumulation"):
        assert name in _lib.ABI_SYMBOLS
        assert hasattr(lib, name)
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt_abi.h")).read()
    assert "#define RT_FLAG_ACCUMULATE 0x40u" in header
    assert lib.rt_abi_version() == (1 << 16) | 3


def test_accumulation_calls_reject_a_null_context():
    from raytrace_amd import _lib
    lib = _lib.amd()
    assert lib.rt_reset_accumulation(None) == abi.RT_ERR_INVALID_ARG
    frames, samples = C.c_uint32(7), C.c_uint32(7)
    assert lib.rt_get_accumulation(None, C.byref(frames), C.byref(samples)) == abi.RT_ERR_INVALID_ARG


@pytest.mark.parametrize("kernel", [abi.RT_KERNEL_MEGA, abi.RT_KERNEL_WAVEFRONT])
def test_baseline_kernels_reject_the_flag_before_touching_a_device(kernel):
    from raytrace_amd import _lib, render
    lib = _lib.amd()
    cfg = render.make_config(64, 64, kernel=kernel, flags=abi.RT_FLAG_ACCUMULATE)
    h = C.c_void_p()
    assert lib.rt_create(C.byref(cfg), C.byref(h)) == abi.RT_ERR_UNIMPLEMENTED and not h
    assert b"RT_FLAG_ACCUMULATE" in lib.rt_last_error(None)
