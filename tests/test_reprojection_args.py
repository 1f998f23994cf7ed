"""RT_FLAG_REPROJECT: what rt_create rejects, before a device is touched (no GPU needed), and the ABI surface."""
import ctypes as C
import os

import pytest

from raytrace_amd import _lib, abi, render

ACC, REP = abi.RT_FLAG_ACCUMULATE, abi.RT_FLAG_REPROJECT


def _create(**kw):
    fields = {k: kw.pop(k) for k in ("tile_rank",) if k in kw}
    cfg = render.make_config(64, 64, **kw)
    for k, v in fields.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    rc = _lib.amd().rt_create(C.byref(cfg), C.byref(h))
    assert not h or rc == abi.RT_OK
    if h:
        _lib.amd().rt_destroy(h)
    return rc, _lib.amd().rt_last_error(None)


def test_reproject_needs_accumulate():
    rc, msg = _create(flags=REP)
    assert rc == abi.RT_ERR_INVALID_ARG and b"RT_FLAG_ACCUMULATE" in msg
    rc, _ = _create(flags=REP | abi.RT_FLAG_CACHE_PRIMARY)
    assert rc == abi.RT_ERR_INVALID_ARG


@pytest.mark.parametrize("bad", [dict(spp=2), dict(tile_world=2), dict(tile_world=2, tile_rank=1)])
def test_frames_of_more_samples_and_tile_contexts_are_unimplemented(bad):
    rc, msg = _create(flags=ACC | REP, **bad)
    assert rc == abi.RT_ERR_UNIMPLEMENTED and b"RT_FLAG_REPROJECT" in msg


@pytest.mark.parametrize("cap", [-1, 65536, -(1 << 31), (1 << 31) - 1])
def test_history_cap_out_of_range(cap):
    rc, msg = _create(flags=ACC | REP, history_cap=cap)
    assert rc == abi.RT_ERR_INVALID_ARG and b"history_cap" in msg


@pytest.mark.parametrize("kernel", [abi.RT_KERNEL_MEGA, abi.RT_KERNEL_WAVEFRONT])
def test_baseline_kernels_reject_it(kernel):
    rc, _ = _create(flags=ACC | REP, kernel=kernel)
    assert rc == abi.RT_ERR_UNIMPLEMENTED


def test_history_cap_is_ignored_without_the_flag():
    """A bad history_cap on a context without the flag is not an argument error: the call gets as far as looking for a device."""
    rc, _ = _create(flags=ACC, history_cap=-1)
    assert rc in (abi.RT_OK, abi.RT_ERR_NO_DEVICE)
    rc, _ = _create(flags=ACC | REP, history_cap=65535)
    assert rc in (abi.RT_OK, abi.RT_ERR_NO_DEVICE)


def test_the_abi_surface():
    assert abi.RT_FLAG_REPROJECT == 0x80
    assert C.sizeof(abi.RtConfig) == 64
    assert abi.RtConfig.history_cap.offset == 44 and abi.RtConfig.reserved.offset == 48 and abi.RtConfig.reserved.size == 16
    assert render.make_config(8, 8).history_cap == 0 and render.make_config(8, 8, history_cap=7).history_cap == 7
    assert "rt_read_history" in _lib.ABI_SYMBOLS and hasattr(_lib.amd(), "rt_read_history")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt_abi.h")).read()
    assert "#define RT_FLAG_REPROJECT 0x80u" in header and "int32_t  history_cap;" in header
    assert _lib.amd().rt_abi_version() == (1 << 16) | 3
    assert _lib.amd().rt_read_history(None, None, 0) == abi.RT_ERR_INVALID_ARG
