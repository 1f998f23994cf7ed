"""rt_detach_voxels / rt_detach_voxels_async without a GPU: the records' layouts in ctypes, numpy and the header, the header's
declarations, flag values, rule phrases and history line, the exported symbols, the unchanged ABI version, a null context, and what
make_voxel_detach and detach_result refuse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytrace_amd import _lib, abi, render
from tests import detach_voxels_ref as ref
from tests import detach_voxels_sets as sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
DETACH_OFFSETS = [("lo", 0), ("flags", 12), ("hi", 16), ("air_material", 28), ("anchor_mask", 32), ("anchor_value", 36), ("max_passes", 40),
                  ("anchor_faces", 44), ("reserved0", 45)]
RESULT_OFFSETS = [("detached", 0), ("supported", 4), ("passes", 8), ("unconverged", 12), ("lo", 16), ("chunks", 28), ("hi", 32), ("reserved", 44)]


def _members(name):
    body = HEADER.split("typedef struct %s {" % name)[1].split("} %s;" % name)[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [m for decl in re.findall(r"(?:uint8_t|uint32_t|int32_t)\s+([^;]+);", body) for m in re.findall(r"([a-z_0-9]+)(?:\[\d\])?", decl)]


def test_structs_have_the_headers_sizes_and_offsets():
    assert C.sizeof(abi.RtVoxelDetach) == 48 and C.sizeof(abi.RtDetachResult) == 48
    assert [(n, getattr(abi.RtVoxelDetach, n).offset) for n, _ in abi.RtVoxelDetach._fields_] == DETACH_OFFSETS
    assert [(n, getattr(abi.RtDetachResult, n).offset) for n, _ in abi.RtDetachResult._fields_] == RESULT_OFFSETS
    # the header's own member order
    assert _members("RtVoxelDetach") == [n for n, _ in DETACH_OFFSETS]
    assert _members("RtDetachResult") == [n for n, _ in RESULT_OFFSETS]
    for name in ("RtVoxelDetach", "RtDetachResult"):
        assert "/* 48 bytes */" in HEADER.split("typedef struct %s {" % name)[1][:40]


def test_dtypes_match_the_structs_and_the_restatements_own():
    assert abi.DETACH_DTYPE.itemsize == 48 == ref.DETACH_DTYPE.itemsize and abi.DETACH_RESULT_DTYPE.itemsize == 48 == ref.RESULT_DTYPE.itemsize
    for name, off in DETACH_OFFSETS:
        assert abi.DETACH_DTYPE.fields[name][1] == off == ref.DETACH_DTYPE.fields[name][1], name
    for name, off in RESULT_OFFSETS:
        assert abi.DETACH_RESULT_DTYPE.fields[name][1] == off == ref.RESULT_DTYPE.fields[name][1], name
    p = sets.cases()["outside the region"]["p"]
    c = abi.RtVoxelDetach.from_buffer_copy(p.tobytes())
    assert (list(c.lo), list(c.hi), c.flags, c.air_material, c.anchor_mask, c.anchor_value, c.max_passes, c.anchor_faces, list(c.reserved0)) == (
        [-10, 98, 138], [9, 106, 142], 3, sets.AIR, 0, 0, 256, 1, [0, 0, 0])
    assert (abi.RT_DETACH_CARVE, abi.RT_DETACH_CAPTURE, abi.RT_DETACH_ANCHOR_MATERIAL) == (ref.CARVE, ref.CAPTURE, ref.ANCHOR_MATERIAL) == (1, 2, 4)
    assert abi.DETACH_MAX_PASSES == ref.MAX_PASSES == 256 and (abi.RT_STAMP_ABSENT, abi.RT_STAMP_SOLID) == (ref.ABSENT, ref.SOLID)


def test_header_declares_the_calls_the_flags_the_rules_and_the_history_line():
    flat = re.sub(r"\s+", " ", HEADER)
    assert "int rt_detach_voxels(RtContext* ctx, const RtVoxelDetach* params, RtDetachResult* result, uint32_t* stamp_out);" in flat
    assert "int rt_detach_voxels_async(RtContext* ctx, const RtVoxelDetach* params, RtDetachResult* result_dev, uint32_t* stamp_out);" in flat
    assert "#define RT_DETACH_CARVE 0x1u" in flat and "#define RT_DETACH_CAPTURE 0x2u" in flat and "#define RT_DETACH_ANCHOR_MATERIAL 0x4u" in flat
    assert "Additive, same minor version: RtVoxelDetach, RtDetachResult, RT_DETACH_*, rt_detach_voxels, rt_detach_voxels_async (voxel * detachment" in flat
    for phrase in ("(material & anchor_mask) == anchor_value", "6-connectivity", "at most * 256", "S_0 be the anchors", "The first p with S_p = S_{p-1} ends the process",
                   "unconverged += 1, passes += max_passes", "no world byte changes", "a requested stamp holds no voxel", "one solid = 0, * air_material record per detached voxel",
                   "RT_SELFTEST_SCENE_MAPS", "detached or not, converged or not", "Stamp voxel d corresponds to texel lo' + d", "RT_STAMP_ABSENT with word 0",
                   "reads the world before the carve", "ordered like rt_stamp_capture", "does not reset the accumulation", "*stamp_out = 0", "anchor_value & ~anchor_mask != 0",
                   "max_passes outside 1..256", "anchor_faces * above 63", "tests/detach_voxels_ref.py", "Device work per call", "bit 2k: low face of axis k of the CLIPPED box"):
        assert phrase in flat, phrase


def test_the_abi_version_is_unchanged():
    assert "#define RT_ABI_VERSION_MAJOR 1" in HEADER and "#define RT_ABI_VERSION_MINOR 3" in HEADER
    assert _lib.amd().rt_abi_version() == (1 << 16) | 3


def test_symbols_are_listed_and_exported():
    assert "rt_detach_voxels" in _lib.ABI_SYMBOLS and "rt_detach_voxels_async" in _lib.ABI_SYMBOLS
    lib = _lib.amd()
    assert hasattr(lib, "rt_detach_voxels") and hasattr(lib, "rt_detach_voxels_async")


def test_null_context_is_invalid_arg_for_both_calls():
    lib = _lib.amd()
    p = np.asarray(sets.cases()["no anchors"]["p"]).reshape(1).copy()
    res = np.zeros(1, dtype=abi.DETACH_RESULT_DTYPE)
    stamp = np.full(1, 77, np.uint32)
    pp, pr, ps = (a.ctypes.data_as(C.c_void_p) for a in (p, res, stamp))
    assert lib.rt_detach_voxels(None, pp, pr, ps) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_detach_voxels_async(None, pp, pr, ps) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_detach_voxels(None, None, None, None) == abi.RT_ERR_INVALID_ARG
    assert not res.view(np.uint8).any() and stamp[0] == 77


def test_make_voxel_detach_builds_the_record_and_refuses_what_the_calls_refuse():
    p = abi.make_voxel_detach((1, 2, 3), (4, 5, 6), flags=7, anchor_faces=0x21, air_material=0xABCD, anchor_mask=0xFF00, anchor_value=0x1200, max_passes=9)
    assert bytes(p) == ref.params((1, 2, 3), (4, 5, 6), 7, 0x21, 0xABCD, 0xFF00, 0x1200, 9).tobytes()
    assert ref.valid(np.frombuffer(bytes(p), ref.DETACH_DTYPE)[0], 256)
    # the game's defaults: carve and capture what the ground (the low z face) does not hold
    assert bytes(abi.make_voxel_detach((1, 2, 3), (4, 5, 6))) == ref.params((1, 2, 3), (4, 5, 6), ref.CARVE | ref.CAPTURE, ref.FACE_LO_Z).tobytes()
    box = dict(lo=(0, 0, 0), hi=(1, 1, 1))
    for bad in (dict(lo=(5, 5, 6), hi=(5, 5, 5)), dict(box, max_passes=0), dict(box, max_passes=257), dict(box, flags=8), dict(box, anchor_faces=64),
                dict(box, anchor_faces=-1), dict(box, flags=7, anchor_mask=1, anchor_value=2), dict(box, anchor_mask=1), dict(box, anchor_value=1),
                dict(lo=(0, 0), hi=(1, 1, 1))):
        with pytest.raises(ValueError):
            abi.make_voxel_detach(**bad)
    res = render.detach_result()
    assert res.dtype == abi.DETACH_RESULT_DTYPE and res.tobytes() == ref.result0().tobytes()
    start = ref.result0(1, 2, 3, 4, (5, 6, 7), 8, (9, 10, 11), 12)
    assert render.detach_result(start.view(abi.DETACH_RESULT_DTYPE)).tobytes() == start.tobytes()
    assert render.detach_result(abi.RtDetachResult.from_buffer_copy(start.tobytes())).tobytes() == start.tobytes()
    with pytest.raises(ValueError):
        render.detach_result((1, 2, 3))
