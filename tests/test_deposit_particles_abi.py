"""rt_deposit_particles / rt_deposit_particles_async without a GPU: the records' layouts in ctypes, numpy and the header, the
header's declarations, rule phrases and history line, the exported symbols, a null context, and what make_particle_deposit,
deposit_counts and deposit_tensor_count refuse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytrace_amd import _lib, abi, render
from tests import deposit_particles_ref as ref
from tests import deposit_particles_sets as sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
DEPOSIT_OFFSETS = [("lo", 0), ("max_speed", 12), ("hi", 16), ("reserved0", 28), ("lr", 32), ("reserved1", 44)]
COUNT_OFFSETS = [("deposited", 0), ("voxels", 4), ("occupied", 8), ("outside", 12)]


def test_structs_have_the_headers_sizes_and_offsets():
    assert C.sizeof(abi.RtParticleDeposit) == 48 and C.sizeof(abi.RtDepositCount) == 16
    assert [(n, getattr(abi.RtParticleDeposit, n).offset) for n, _ in abi.RtParticleDeposit._fields_] == DEPOSIT_OFFSETS
    assert [(n, getattr(abi.RtDepositCount, n).offset) for n, _ in abi.RtDepositCount._fields_] == COUNT_OFFSETS
    # the header's own member order
    body = HEADER.split("typedef struct RtParticleDeposit {")[1].split("} RtParticleDeposit;")[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m for decl in re.findall(r"(?:float|uint32_t|int32_t)\s+([^;]+);", body) for m in re.findall(r"([a-z_0-9]+)(?:\[\d\])?", decl)]
    assert members == [n for n, _ in DEPOSIT_OFFSETS]
    body = HEADER.split("typedef struct RtDepositCount {")[1].split("} RtDepositCount;")[0]
    assert re.findall(r"(\w+)[,;]", body.split("uint32_t")[1]) == [n for n, _ in COUNT_OFFSETS]
    assert "/* 48 bytes */" in HEADER.split("typedef struct RtParticleDeposit {")[1][:40]


def test_dtypes_match_the_structs_and_the_restatements_own():
    assert abi.DEPOSIT_DTYPE.itemsize == 48 == ref.DEPOSIT_DTYPE.itemsize and abi.DEPOSIT_COUNT_DTYPE.itemsize == 16 == ref.COUNT_DTYPE.itemsize
    for name, off in DEPOSIT_OFFSETS:
        assert abi.DEPOSIT_DTYPE.fields[name][1] == off == ref.DEPOSIT_DTYPE.fields[name][1], name
    for name, off in COUNT_OFFSETS:
        assert abi.DEPOSIT_COUNT_DTYPE.fields[name][1] == off == ref.COUNT_DTYPE.fields[name][1], name
    p = sets.cases()["seam"]["p"]
    c = abi.RtParticleDeposit.from_buffer_copy(p.tobytes())
    assert (list(c.lo), list(c.hi), list(c.lr), c.max_speed, c.reserved0, c.reserved1) == ([30, 120, 120], [50, 135, 140], list(sets.LR_SEAM), 0.0, 0, 0)
    assert abi.MAX_DEPOSIT_TEXELS == ref.MAX_TEXELS == 1 << 24


def test_header_declares_the_calls_the_rules_and_the_history_line():
    flat = re.sub(r"\s+", " ", HEADER)
    assert ("int rt_deposit_particles(RtContext* ctx, const RtParticleDeposit* params, RtParticleState* states, RtParticle* draw, "
            "uint32_t count, RtDepositCount* counts);") in flat
    assert ("int rt_deposit_particles_async(RtContext* ctx, const RtParticleDeposit* params, RtParticleState* states_dev, "
            "RtParticle* draw_dev, uint32_t count, RtDepositCount* counts_dev);") in flat
    assert "Additive, same minor version: RtParticleDeposit, RtDepositCount, rt_deposit_particles, rt_deposit_particles_async (particle" in flat
    assert "#define RT_ABI_VERSION_MINOR 3" in HEADER
    for phrase in ("(flags & RT_PSTATE_CONTACT) != 0", "|velocity_k| <= max_speed", "c_k = (lo_k + hi_k) * 0.5f", "v_k = (int)floorf(c_k)",
                   "x_k = (v_k + R/2) mod R", "lr_k - R/2 <= v_k < lr_k * + R/2", "|lr_k| <= 2^22 - R", "at most 2^24 texels", "LOWEST INDEX",
                   "outside += 1", "occupied += 1", "deposited += 1", "draw[i].half become * +0.0f", "RT_SELFTEST_SCENE_MAPS", "ADDED to",
                   "EMBEDDED at its next step", "Device work per call", "tests/deposit_particles_ref.py", "keeps the box tight",
                   "Bounds found on the device"):
        assert phrase in flat, phrase


def test_symbols_are_listed_and_exported():
    assert "rt_deposit_particles" in _lib.ABI_SYMBOLS and "rt_deposit_particles_async" in _lib.ABI_SYMBOLS
    lib = _lib.amd()
    assert hasattr(lib, "rt_deposit_particles") and hasattr(lib, "rt_deposit_particles_async")


def test_null_context_is_invalid_arg_for_both_calls():
    lib = _lib.amd()
    case = sets.cases()["count 1"]
    p = case["p"].reshape(1).view(abi.DEPOSIT_DTYPE)
    states, cnt = case["states"].copy(), np.zeros(1, dtype=abi.DEPOSIT_COUNT_DTYPE)
    pp, ps, pc = (a.ctypes.data_as(C.c_void_p) for a in (p, states, cnt))
    assert lib.rt_deposit_particles(None, pp, ps, None, 1, pc) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_deposit_particles_async(None, pp, ps, None, 1, pc) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_deposit_particles(None, None, None, None, 0, None) == abi.RT_ERR_INVALID_ARG
    assert states.tobytes() == case["states"].tobytes() and not cnt.view(np.uint8).any()


def test_make_particle_deposit_builds_the_record_and_refuses_what_the_calls_refuse():
    p = abi.make_particle_deposit((1, 2, 3), (4, 5, 6), max_speed=0.25, lr=(16, -32, 48))
    assert bytes(p) == ref.params((1, 2, 3), (4, 5, 6), 0.25, (16, -32, 48)).tobytes()
    assert ref.valid(np.frombuffer(bytes(p), ref.DEPOSIT_DTYPE)[0], 256)
    for bad in (dict(lo=(5, 5, 6), hi=(5, 5, 5)), dict(lo=(0, 0, 0), hi=(1, 1, 1), max_speed=-1.0), dict(lo=(0, 0, 0), hi=(1, 1, 1), max_speed=np.inf),
                dict(lo=(0, 0, 0), hi=(1, 1, 1), max_speed=np.nan), dict(lo=(0, 0), hi=(1, 1, 1))):
        with pytest.raises(ValueError):
            abi.make_particle_deposit(**bad)
    cnt = render.deposit_counts((5, 6, 7, 8))
    assert cnt.dtype == abi.DEPOSIT_COUNT_DTYPE and cnt[0].tolist() == (5, 6, 7, 8)
    assert render.deposit_counts(cnt[0])[0].tolist() == (5, 6, 7, 8) and render.deposit_counts(abi.RtDepositCount(1, 2, 3, 4))[0].tolist() == (1, 2, 3, 4)
    assert render.deposit_counts()[0].tolist() == (0, 0, 0, 0)


def test_deposit_tensor_count_refuses_what_the_kernel_could_not_use():
    import torch
    states, counts = torch.zeros((4, 16), dtype=torch.float32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="cuda"):
        render.deposit_tensor_count(states, None, counts, 0)                          # host tensors
    with pytest.raises(ValueError, match="states must be a torch tensor"):
        render.deposit_tensor_count(np.zeros((4, 16), np.float32), None, None, 0)
    with pytest.raises(ValueError, match="counts must be a torch tensor"):
        render.deposit_tensor_count(states, None, np.zeros(4, np.uint32), 0)
    with pytest.raises(ValueError, match="draw must be a torch tensor"):
        render.deposit_tensor_count(states, np.zeros((4, 8), np.float32), None, 0)
