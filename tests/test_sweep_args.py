"""Box sweeps: the ABI surface (struct sizes and offsets, constants, header text, symbols) and every refusal that needs no device:
a null context, and what the binding's own argument checks (make_sweeps, check_sweep_tensors) turn away before an address can reach
the kernel.  The refusals that need a context (NOT_READY, the count limit, null pointers, the validated domain) are in
tests/test_gpu_sweeps.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from raytrace_amd import _lib, abi, render
from tests import sweep_ref as sr

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt_abi.h")).read()


def test_struct_layouts():
    assert C.sizeof(abi.RtBoxSweep) == 48 and C.sizeof(abi.RtSweepHit) == 64
    s = abi.RtBoxSweep
    assert (s.lo.offset, s.reserved0.offset, s.hi.offset, s.reserved1.offset, s.motion.offset, s.reserved2.offset) == (0, 12, 16, 28, 32, 44)
    h = abi.RtSweepHit
    assert (h.t.offset, h.kind.offset, h.normal.offset, h.material.offset, h.texel.offset, h.axis.offset) == (0, 4, 8, 12, 16, 28)
    assert (h.lo.offset, h.reserved0.offset, h.hi.offset, h.reserved1.offset) == (32, 44, 48, 60)
    for dtype, struct in ((render.SWEEP_DTYPE, s), (render.SWEEP_HIT_DTYPE, h), (sr.HIT_DTYPE, h)):
        assert dtype.itemsize == C.sizeof(struct)
        for name, _ in struct._fields_:
            assert dtype.fields[name][1] == getattr(struct, name).offset, name


def test_constants_and_header_text():
    assert (abi.RT_SWEEP_FREE, abi.RT_SWEEP_BLOCKED, abi.RT_SWEEP_EMBEDDED, abi.RT_SWEEP_INVALID) == (0, 1, 2, 3)
    assert (sr.FREE, sr.BLOCKED, sr.EMBEDDED, sr.INVALID) == (0, 1, 2, 3)
    for line in ("#define RT_SWEEP_FREE     0", "#define RT_SWEEP_BLOCKED  1", "#define RT_SWEEP_EMBEDDED 2", "#define RT_SWEEP_INVALID  3",
                 "typedef struct RtBoxSweep {", "typedef struct RtSweepHit {",
                 "int rt_sweep_boxes(RtContext* ctx, const RtBoxSweep* sweeps, uint32_t count, const int32_t lr[3], RtSweepHit* hits);",
                 "int rt_sweep_boxes_async(RtContext* ctx, const RtBoxSweep* sweeps_dev, uint32_t count, const int32_t lr[3], RtSweepHit* hits_dev);",
                 "RtBoxSweep, RtSweepHit, RT_SWEEP_*, rt_sweep_boxes, rt_sweep_boxes_async"):
        assert line in HEADER, line
    assert "#define RT_ABI_VERSION_MINOR 3" in HEADER


def test_symbols_and_null_context():
    lib = _lib.amd()
    assert "rt_sweep_boxes" in _lib.ABI_SYMBOLS and "rt_sweep_boxes_async" in _lib.ABI_SYMBOLS
    assert lib.rt_abi_version() == (1 << 16) | 3
    lr = (C.c_int32 * 3)(0, 0, 0)
    sweeps = render.make_sweeps([[[0, 0, 0], [1, 1, 1], [0, 0, 1]]])
    hits = np.full(1, 0x55, dtype=np.uint8).repeat(64)
    for fn in (lib.rt_sweep_boxes, lib.rt_sweep_boxes_async):
        assert fn(None, None, 0, None, None) == abi.RT_ERR_INVALID_ARG
        assert fn(None, sweeps.ctypes.data_as(C.c_void_p), 1, lr, hits.ctypes.data_as(C.c_void_p)) == abi.RT_ERR_INVALID_ARG
    assert (hits == 0x55).all()


def test_make_sweeps():
    rows = np.arange(18, dtype=np.float32).reshape(2, 3, 3)
    recs = render.make_sweeps(rows)
    assert recs.dtype == render.SWEEP_DTYPE and recs.shape == (2,)
    assert (recs["lo"] == rows[:, 0]).all() and (recs["hi"] == rows[:, 1]).all() and (recs["motion"] == rows[:, 2]).all()
    assert not recs["reserved0"].any() and not recs["reserved1"].any() and not recs["reserved2"].any()
    assert render.make_sweeps(recs).tobytes() == recs.tobytes()
    assert render.make_sweeps(np.zeros((0, 3, 3))).size == 0
    with pytest.raises(ValueError):
        render.make_sweeps(np.zeros((2, 8)))


@pytest.mark.parametrize("what", ["host sweeps", "host hits", "host both", "not tensors"])
def test_host_tensors_are_refused(what):
    sweeps = torch.zeros((4, 12), dtype=torch.float32)
    hits = torch.zeros((4, 64), dtype=torch.uint8)
    if what == "not tensors":
        sweeps, hits = sweeps.numpy(), hits.numpy()
    with pytest.raises(ValueError):
        render.check_sweep_tensors(sweeps, hits, 0)


def test_device_mismatch_and_sizes_are_refused_without_a_device():
    # every tensor here lives on the host: the device check refuses them first, whatever else is wrong with them
    for sweeps, hits in ((torch.zeros((4, 11)), torch.zeros((4, 64), dtype=torch.uint8)),
                         (torch.zeros((4, 12)), torch.zeros((4, 63), dtype=torch.uint8))):
        with pytest.raises(ValueError, match="cuda:1"):
            render.check_sweep_tensors(sweeps, hits, 1)


def test_the_restatement_and_the_host_agree_on_the_domain():
    """in_domain of the restatement on the edge of every limit (the library applies the same comparisons on the host and on the
    device; tests/test_gpu_sweeps.py checks that it does)."""
    ok = np.float32([[0, 0, 0], [1, 1, 1], [0, 0, 0]])
    assert sr.in_domain(*ok)
    for (i, j, v), good in (((0, 0, -2.0 ** 22), False), ((1, 0, 8.0), True), ((1, 0, np.nextafter(np.float32(8), np.float32(9))), False),
                            ((2, 1, 64.0), True), ((2, 1, -64.0), True), ((2, 1, np.nextafter(np.float32(64), np.float32(65))), False),
                            ((1, 2, 0.0), False), ((1, 2, -1.0), False), ((1, 2, 1e-30), True), ((2, 0, np.nan), False),
                            ((0, 1, -np.inf), False), ((1, 1, np.inf), False)):
        s = ok.copy()
        s[i, j] = v
        assert sr.in_domain(*s) == good, (i, j, v)
    far = np.float32([[2.0 ** 22 - 1, 0, 0], [2.0 ** 22, 1, 1], [64, 0, 0]])
    assert sr.in_domain(*far)
    far[1, 0] = np.nextafter(np.float32(2.0 ** 22), np.float32(np.inf))
    assert not sr.in_domain(*far)
