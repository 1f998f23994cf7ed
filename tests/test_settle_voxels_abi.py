"""rt_settle_voxels / rt_settle_voxels_async without a GPU: the records' layouts in ctypes, numpy and the header, the header's
declarations, rule phrases and history line, the exported symbols, the unchanged ABI version, a null context, and what
make_voxel_settle and settle_counts refuse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytrace_amd import _lib, abi, render
from tests import settle_voxels_ref as ref
from tests import settle_voxels_sets as sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
SETTLE_OFFSETS = [("lo", 0), ("max_fall", 12), ("hi", 16), ("air_material", 28), ("loose_mask", 32), ("loose_value", 36), ("axis", 40), ("toward", 41),
                  ("reserved0", 42), ("reserved1", 44)]
COUNT_OFFSETS = [("moved", 0), ("falling", 4), ("distance", 8), ("chunks", 12)]


def test_structs_have_the_headers_sizes_and_offsets():
    assert C.sizeof(abi.RtVoxelSettle) == 48 and C.sizeof(abi.RtSettleCount) == 16
    assert [(n, getattr(abi.RtVoxelSettle, n).offset) for n, _ in abi.RtVoxelSettle._fields_] == SETTLE_OFFSETS
    assert [(n, getattr(abi.RtSettleCount, n).offset) for n, _ in abi.RtSettleCount._fields_] == COUNT_OFFSETS
    # the header's own member order
    body = HEADER.split("typedef struct RtVoxelSettle {")[1].split("} RtVoxelSettle;")[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m for decl in re.findall(r"(?:uint8_t|uint32_t|int32_t)\s+([^;]+);", body) for m in re.findall(r"([a-z_0-9]+)(?:\[\d\])?", decl)]
    assert members == [n for n, _ in SETTLE_OFFSETS]
    body = HEADER.split("typedef struct RtSettleCount {")[1].split("} RtSettleCount;")[0]
    assert re.findall(r"(\w+)[,;]", body.split("uint32_t")[1]) == [n for n, _ in COUNT_OFFSETS]
    assert "/* 48 bytes */" in HEADER.split("typedef struct RtVoxelSettle {")[1][:40]


def test_dtypes_match_the_structs_and_the_restatements_own():
    assert abi.SETTLE_DTYPE.itemsize == 48 == ref.SETTLE_DTYPE.itemsize and abi.SETTLE_COUNT_DTYPE.itemsize == 16 == ref.COUNT_DTYPE.itemsize
    for name, off in SETTLE_OFFSETS:
        assert abi.SETTLE_DTYPE.fields[name][1] == off == ref.SETTLE_DTYPE.fields[name][1], name
    for name, off in COUNT_OFFSETS:
        assert abi.SETTLE_COUNT_DTYPE.fields[name][1] == off == ref.COUNT_DTYPE.fields[name][1], name
    p = sets.cases()["outside the region"]["p"]
    c = abi.RtVoxelSettle.from_buffer_copy(p.tobytes())
    assert (list(c.lo), list(c.hi), c.max_fall, c.air_material, c.loose_mask, c.loose_value, c.axis, c.toward, list(c.reserved0), c.reserved1) == (
        [-20, 64, 248], [10, 70, 300], 4, sets.AIR, 0, 0, 2, 1, [0, 0], 0)
    assert abi.SETTLE_UNLIMITED == ref.UNLIMITED == 0xFFFFFFFF


def test_header_declares_the_calls_the_rules_and_the_history_line():
    flat = re.sub(r"\s+", " ", HEADER)
    assert "int rt_settle_voxels(RtContext* ctx, const RtVoxelSettle* params, RtSettleCount* counts);" in flat
    assert "int rt_settle_voxels_async(RtContext* ctx, const RtVoxelSettle* params, RtSettleCount* counts_dev);" in flat
    assert "Additive, same minor version: RtVoxelSettle, RtSettleCount, rt_settle_voxels, rt_settle_voxels_async (voxel settling" in flat
    for phrase in ("(material & loose_mask) == loose_value", "h = x - lo' for * toward = 0, h = hi' - x for toward = 1", "f = 1 + the highest fixed h' < h",
                   "h - min(max_fall, E(h))", "E(h2) - E(h1) <= h2 - h1 - 1", "There is no texel limit", "is a floor", "holds air_material",
                   "one solid = 0, air_material record per source", "RT_SELFTEST_SCENE_MAPS", "ADDED to", "E - drop > 0", "tests/settle_voxels_ref.py",
                   "whether or not anything * moved", "max_fall == 0", "loose_value & ~loose_mask != 0", "Device work per call"):
        assert phrase in flat, phrase


def test_the_abi_version_is_unchanged():
    assert "#define RT_ABI_VERSION_MAJOR 1" in HEADER and "#define RT_ABI_VERSION_MINOR 3" in HEADER
    assert _lib.amd().rt_abi_version() == (1 << 16) | 3


def test_symbols_are_listed_and_exported():
    assert "rt_settle_voxels" in _lib.ABI_SYMBOLS and "rt_settle_voxels_async" in _lib.ABI_SYMBOLS
    lib = _lib.amd()
    assert hasattr(lib, "rt_settle_voxels") and hasattr(lib, "rt_settle_voxels_async")


def test_null_context_is_invalid_arg_for_both_calls():
    lib = _lib.amd()
    p = np.asarray(sets.cases()["at rest"]["p"]).reshape(1).copy()
    cnt = np.zeros(1, dtype=abi.SETTLE_COUNT_DTYPE)
    pp, pc = (a.ctypes.data_as(C.c_void_p) for a in (p, cnt))
    assert lib.rt_settle_voxels(None, pp, pc) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_settle_voxels_async(None, pp, pc) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_settle_voxels(None, None, None) == abi.RT_ERR_INVALID_ARG
    assert not cnt.view(np.uint8).any()


def test_make_voxel_settle_builds_the_record_and_refuses_what_the_calls_refuse():
    p = abi.make_voxel_settle((1, 2, 3), (4, 5, 6), max_fall=7, air_material=0xABCD, loose_mask=0xFF00, loose_value=0x1200, axis=1, toward=1)
    assert bytes(p) == ref.params((1, 2, 3), (4, 5, 6), 7, 0xABCD, 0xFF00, 0x1200, 1, 1).tobytes()
    assert ref.valid(np.frombuffer(bytes(p), ref.SETTLE_DTYPE)[0], 256)
    assert bytes(abi.make_voxel_settle((1, 2, 3), (4, 5, 6))) == ref.params((1, 2, 3), (4, 5, 6)).tobytes()      # the game's defaults: down z, until at rest
    for bad in (dict(lo=(5, 5, 6), hi=(5, 5, 5)), dict(lo=(0, 0, 0), hi=(1, 1, 1), max_fall=0), dict(lo=(0, 0, 0), hi=(1, 1, 1), max_fall=1 << 32),
                dict(lo=(0, 0, 0), hi=(1, 1, 1), axis=3), dict(lo=(0, 0, 0), hi=(1, 1, 1), toward=2), dict(lo=(0, 0, 0), hi=(1, 1, 1), loose_value=1),
                dict(lo=(0, 0), hi=(1, 1, 1))):
        with pytest.raises(ValueError):
            abi.make_voxel_settle(**bad)
    cnt = render.settle_counts((5, 6, 7, 8))
    assert cnt.dtype == abi.SETTLE_COUNT_DTYPE and cnt[0].tolist() == (5, 6, 7, 8)
    assert render.settle_counts(cnt[0])[0].tolist() == (5, 6, 7, 8) and render.settle_counts(abi.RtSettleCount(1, 2, 3, 4))[0].tolist() == (1, 2, 3, 4)
    assert render.settle_counts()[0].tolist() == (0, 0, 0, 0)
