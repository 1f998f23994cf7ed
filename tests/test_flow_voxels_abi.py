"""rt_flow_voxels / rt_flow_voxels_async without a GPU: the records' layouts in ctypes, numpy and the header, the header's
declarations, rule phrases and history line, the exported symbols, the unchanged ABI version, a null context, and what
make_voxel_flow and flow_counts refuse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytrace_amd import _lib, abi, render
from tests import flow_voxels_ref as ref
from tests import flow_voxels_sets as sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
FLOW_OFFSETS = [("lo", 0), ("ticks", 12), ("hi", 16), ("air_material", 28), ("fluid_mask", 32), ("fluid_value", 36), ("fluid_word", 40), ("reserved0", 44),
                ("level_shift", 48), ("max_level", 49), ("reserved1", 50), ("reserved2", 52)]
COUNT_OFFSETS = [("wetted", 0), ("dried", 4), ("changed", 8), ("active", 12), ("chunks", 16), ("reserved", 20)]


def test_structs_have_the_headers_sizes_and_offsets():
    assert C.sizeof(abi.RtVoxelFlow) == 64 and C.sizeof(abi.RtFlowCount) == 32
    assert [(n, getattr(abi.RtVoxelFlow, n).offset) for n, _ in abi.RtVoxelFlow._fields_] == FLOW_OFFSETS
    assert [(n, getattr(abi.RtFlowCount, n).offset) for n, _ in abi.RtFlowCount._fields_] == COUNT_OFFSETS
    # the header's own member order
    body = HEADER.split("typedef struct RtVoxelFlow {")[1].split("} RtVoxelFlow;")[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m for decl in re.findall(r"(?:uint8_t|uint32_t|int32_t)\s+([^;]+);", body) for m in re.findall(r"([a-z_0-9]+)(?:\[\d\])?", decl)]
    assert members == [n for n, _ in FLOW_OFFSETS]
    body = HEADER.split("typedef struct RtFlowCount {")[1].split("} RtFlowCount;")[0]
    assert re.findall(r"(\w+)(?:\[3\])?[,;]", body.split("uint32_t")[1]) == [n for n, _ in COUNT_OFFSETS]
    assert "/* 64 bytes */" in HEADER.split("typedef struct RtVoxelFlow {")[1][:40]


def test_dtypes_match_the_structs_and_the_restatements_own():
    assert abi.FLOW_DTYPE.itemsize == 64 == ref.FLOW_DTYPE.itemsize and abi.FLOW_COUNT_DTYPE.itemsize == 32 == ref.COUNT_DTYPE.itemsize
    for name, off in FLOW_OFFSETS:
        assert abi.FLOW_DTYPE.fields[name][1] == off == ref.FLOW_DTYPE.fields[name][1], name
    for name, off in COUNT_OFFSETS:
        assert abi.FLOW_COUNT_DTYPE.fields[name][1] == off == ref.COUNT_DTYPE.fields[name][1], name
    p = sets.cases()["clipped by the region"]["p"]
    c = abi.RtVoxelFlow.from_buffer_copy(p.tobytes())
    assert (list(c.lo), list(c.hi), c.ticks, c.air_material, c.fluid_mask, c.fluid_value, c.fluid_word, c.reserved0, c.level_shift, c.max_level,
            list(c.reserved1), list(c.reserved2)) == ([-5, 249, 128], [6, 262, 133], 12, sets.AIR, 0xFF000000, sets.WATER, sets.WATER, 0, 0, 7, [0, 0], [0, 0, 0])
    assert (abi.FLOW_MAX_TICKS, abi.FLOW_MAX_LEVEL, abi.FLOW_MAX_SHIFT) == (ref.MAX_TICKS, ref.MAX_LEVEL, ref.MAX_SHIFT) == (256, 13, 28)


def test_header_declares_the_calls_the_rules_and_the_history_line():
    flat = re.sub(r"\s+", " ", HEADER)
    assert "int rt_flow_voxels(RtContext* ctx, const RtVoxelFlow* params, RtFlowCount* counts);" in flat
    assert "int rt_flow_voxels_async(RtContext* ctx, const RtVoxelFlow* params, RtFlowCount* counts_dev);" in flat
    assert "Additive, same minor version: RtVoxelFlow, RtFlowCount, rt_flow_voxels, rt_flow_voxels_async (fluid flow" in flat
    for phrase in ("(material & * fluid_mask) == fluid_value", "FIELD = 0xF << level_shift", "v == 15 is a SOURCE", "strength min(v, max_level)", "Up is +z",
                   "is a floor, which counts * as FIXED", "e(n) = max_level + 1 for a source", "SPREADING iff it is a source, or the cell n - z is FIXED",
                   "s' = * max(D, S)", "e(n) - 1 over the four horizontal neighbours", "(w & * ~FIELD) | s << level_shift", "holds air_material",
                   "T calls of one tick and one call of T ticks agree", "dries and is wetted again", "one record per such cell", "dirties nothing",
                   "RT_SELFTEST_SCENE_MAPS", "ADDED to", "the host stops ticking when active is 0", "tests/flow_voxels_ref.py", "whether or not anything * changed",
                   "ticks outside 1..256", "max_level outside * 1..13", "(fluid_word & * fluid_mask) != fluid_value", "volume conservation and pressure",
                   "an up axis other than +z", "swimming", "Device work per call", "RT_FLOW_TICKS"):
        assert phrase in flat, phrase


def test_the_abi_version_is_unchanged():
    assert "#define RT_ABI_VERSION_MAJOR 1" in HEADER and "#define RT_ABI_VERSION_MINOR 3" in HEADER
    assert _lib.amd().rt_abi_version() == (1 << 16) | 3


def test_symbols_are_listed_and_exported():
    assert "rt_flow_voxels" in _lib.ABI_SYMBOLS and "rt_flow_voxels_async" in _lib.ABI_SYMBOLS
    lib = _lib.amd()
    assert hasattr(lib, "rt_flow_voxels") and hasattr(lib, "rt_flow_voxels_async")


def test_null_context_is_invalid_arg_for_both_calls():
    lib = _lib.amd()
    p = np.asarray(sets.cases()["ledge"]["p"]).reshape(1).copy()
    cnt = np.zeros(1, dtype=abi.FLOW_COUNT_DTYPE)
    pp, pc = (a.ctypes.data_as(C.c_void_p) for a in (p, cnt))
    assert lib.rt_flow_voxels(None, pp, pc) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_flow_voxels_async(None, pp, pc) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_flow_voxels(None, None, None) == abi.RT_ERR_INVALID_ARG
    assert not cnt.view(np.uint8).any()


def test_make_voxel_flow_builds_the_record_and_refuses_what_the_calls_refuse():
    p = abi.make_voxel_flow((1, 2, 3), (4, 5, 6), 0xFF000000, 0x5A000000, 0x5A001200, ticks=9, air_material=0xABCD, level_shift=4, max_level=13)
    assert bytes(p) == ref.params((1, 2, 3), (4, 5, 6), 0xFF000000, 0x5A000000, 0x5A001200, 9, 0xABCD, 4, 13).tobytes()
    assert ref.valid(np.frombuffer(bytes(p), ref.FLOW_DTYPE)[0], 256)
    assert bytes(abi.make_voxel_flow((1, 2, 3), (4, 5, 6), 0xFF000000, 0x5A000000)) == ref.params((1, 2, 3), (4, 5, 6), 0xFF000000, 0x5A000000).tobytes()
    ok = dict(lo=(0, 0, 0), hi=(1, 1, 1), fluid_mask=0xFF000000, fluid_value=0x5A000000)
    for bad in (dict(lo=(5, 5, 6), hi=(5, 5, 5)), dict(ticks=0), dict(ticks=257), dict(level_shift=29), dict(max_level=0), dict(max_level=14), dict(fluid_mask=0, fluid_value=0),
                dict(fluid_mask=0xFF000008), dict(fluid_value=0x5A000010), dict(fluid_word=0x5A000001), dict(fluid_word=0x5B000000), dict(lo=(0, 0))):
        with pytest.raises(ValueError):
            abi.make_voxel_flow(**dict(ok, **bad))
    cnt = render.flow_counts((5, 6, 7, 8, 9))
    assert cnt.dtype == abi.FLOW_COUNT_DTYPE and cnt[0].tolist()[:5] == (5, 6, 7, 8, 9)[:5] and list(cnt[0]["reserved"]) == [0, 0, 0]
    assert render.flow_counts(cnt[0]).tobytes() == cnt.tobytes() and render.flow_counts(abi.RtFlowCount(1, 2, 3, 4, 5)).tobytes()[:20] == np.arange(1, 6, dtype="<u4").tobytes()
    assert not render.flow_counts().view(np.uint8).any()
