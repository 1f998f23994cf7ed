"""rt_sweep_entities / rt_sweep_entities_async without a GPU: the record's layout in ctypes, numpy and the header, the header's
declarations, rule phrases and history line, the exported symbols, a null context, and what entity_sweep_tensor_counts refuses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytrace_amd import _lib, abi, render
from tests import sweep_entities_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
OFFSETS = [("t", 0), ("kind", 4), ("normal", 8), ("material", 12), ("entity", 16), ("index", 20), ("axis", 24), ("voxel", 28), ("cell", 32),
           ("reserved0", 44), ("lo", 48), ("reserved1", 60), ("hi", 64), ("reserved2", 76)]


def test_struct_has_the_headers_size_and_offsets():
    assert C.sizeof(abi.RtEntitySweepHit) == 80
    assert [(n, getattr(abi.RtEntitySweepHit, n).offset) for n, _ in abi.RtEntitySweepHit._fields_] == OFFSETS
    body = HEADER.split("typedef struct RtEntitySweepHit {")[1].split("} RtEntitySweepHit;")[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [n for decl in re.findall(r"(?:float|uint32_t|int32_t)\s+([^;]+);", body) for n in re.findall(r"(\w+)(?:\[3\])?", decl)]
    assert members == [n for n, _ in OFFSETS]
    assert "/* 80 bytes */" in HEADER.split("typedef struct RtEntitySweepHit {")[1][:40]


def test_dtypes_match_the_struct_and_the_restatements_own():
    dt = abi.ENTITY_SWEEP_HIT_DTYPE
    assert dt.itemsize == 80 == ref.HIT_DTYPE.itemsize and not hasattr(render, "ENTITY_SWEEP_HIT_DTYPE")   # the dtype lives in abi
    for name, off in OFFSETS:
        assert dt.fields[name][1] == off == ref.HIT_DTYPE.fields[name][1], name
    for name in ("lo", "reserved0", "hi", "reserved1", "motion", "reserved2"):
        assert render.SWEEP_DTYPE.fields[name][1] == ref.SWEEP_DTYPE.fields[name][1], name
    assert (ref.FREE, ref.BLOCKED, ref.EMBEDDED, ref.INVALID) == (abi.RT_SWEEP_FREE, abi.RT_SWEEP_BLOCKED, abi.RT_SWEEP_EMBEDDED, abi.RT_SWEEP_INVALID)
    assert (ref.NONE, ref.BOX, ref.MODEL) == (abi.RT_ENTITY_NONE, abi.RT_ENTITY_BOX, abi.RT_ENTITY_MODEL)


def test_header_declares_the_calls_the_rules_and_the_history_line():
    flat = re.sub(r"\s+", " ", HEADER)
    assert ("int rt_sweep_entities(RtContext* ctx, const RtBoxSweep* sweeps, uint32_t count, const int32_t lr[3], const RtDrawBox* boxes, "
            "uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels, RtSweepHit* world_hits, RtEntitySweepHit* entity_hits);") in flat
    assert ("int rt_sweep_entities_async(RtContext* ctx, const RtBoxSweep* sweeps_dev, uint32_t count, const int32_t lr[3], "
            "const RtDrawBox* boxes_dev, uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels, RtSweepHit* world_hits_dev, "
            "RtEntitySweepHit* entity_hits_dev);") in flat
    assert ("Additive, same minor version: RtEntitySweepHit, rt_sweep_entities, rt_sweep_entities_async (entity sweeps: box sweeps that * "
            "collide with the drawn boxes and models as well as with the world).") in flat
    assert "#define RT_ABI_VERSION_MINOR 3" in HEADER
    rules = flat.split("Entity sweeps: rt_sweep_boxes' box swept")[1].split("int rt_sweep_entities(")[0]
    rules = rules.replace(" * ", " ")
    for phrase in ("lo_k < ohi_k && olo_k < hi_k", "te_k = (olo_k - hi_k) / m_k", "tx_k = (ohi_k - lo_k) / m_k", "te_k = (ohi_k - lo_k) / m_k",
                   "the HIGHEST axis on equal values", "te_a >= 0, te_a < 1, and te_a < tx_k on every moving axis",
                   "plane_k(i) = rtm_fma(float(i), scale, origin_k)", "a cell with two equal planes on some axis",
                   "then the lowest blocked axis, then the first in ascending (z, y, x) order", "EMBEDDED beats BLOCKED",
                   "on equal t boxes come before models", "t_e < W.t: strict, the world wins ties", "a value s in 1..nboxes makes the sweep ignore box s - 1",
                   "reserved2 stays ignored", "hi' = F, lo' = max(F - size, float(c.lo_a))", "lo' = F, hi' = min(F + size, float(c.hi_a + 1))",
                   "after every world event with time < t_e", "is never world-EMBEDDED", "may graze a second entity",
                   "count <= 2^24; nboxes, nmodels <= 4096", "Every byte of every record is written", "tests/sweep_entities_ref.py",
                   "256^2 cells in every layer", "entities are no obstacles of rt_step_particles", "entities are not rotated",
                   "no acceleration structure over entities", "rt_stamp_destroy after an enqueued call waits for it"):
        assert phrase in rules, phrase


def test_symbols_are_listed_and_exported():
    assert "rt_sweep_entities" in _lib.ABI_SYMBOLS and "rt_sweep_entities_async" in _lib.ABI_SYMBOLS
    lib = _lib.amd()
    assert hasattr(lib, "rt_sweep_entities") and hasattr(lib, "rt_sweep_entities_async")
    assert len(_lib.AMD_FUNCTIONS["rt_sweep_entities"][1]) == len(_lib.AMD_FUNCTIONS["rt_sweep_entities_async"][1]) == 10


def test_null_context_is_invalid_arg_and_writes_nothing():
    lib = _lib.amd()
    sweeps = render.make_sweeps(np.float32([[[0, 0, 0], [1, 1, 1], [1, 0, 0]]]))
    boxes = np.zeros(1, dtype=render.DRAW_BOX_DTYPE)
    boxes["hi"] = 1.0
    world = np.full(64, 0x5A, dtype=np.uint8)
    hits = np.full(80, 0x5A, dtype=np.uint8)
    lr = (C.c_int32 * 3)(0, 0, 0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for fn in (lib.rt_sweep_entities, lib.rt_sweep_entities_async):
        assert fn(None, p(sweeps), 1, lr, p(boxes), 1, None, 0, p(world), p(hits)) == abi.RT_ERR_INVALID_ARG
        assert fn(None, None, 0, None, None, 0, None, 0, None, None) == abi.RT_ERR_INVALID_ARG
    assert (world == 0x5A).all() and (hits == 0x5A).all()


def test_entity_sweep_tensor_counts_refuses_what_the_kernel_could_not_use():
    import torch
    sweeps = torch.zeros((2, 12), dtype=torch.float32)
    hits = torch.zeros((2, 20), dtype=torch.float32)
    with pytest.raises(ValueError, match="cuda"):
        render.entity_sweep_tensor_counts(sweeps, None, None, hits, 0)                 # host tensors
    with pytest.raises(ValueError, match="sweeps must be a torch tensor"):
        render.entity_sweep_tensor_counts(np.zeros((2, 12), np.float32), None, None, hits, 0)
    with pytest.raises(ValueError, match="world_hits must be a torch tensor"):
        render.entity_sweep_tensor_counts(sweeps, None, np.zeros(32, np.float32), hits, 0)
    with pytest.raises(ValueError, match="at most"):
        render.record_count("sweeps", 48 * ((1 << 24) + 1), 48, abi.MAX_ENTITY_SWEEPS, "RtBoxSweep")
