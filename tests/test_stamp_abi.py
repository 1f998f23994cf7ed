"""The voxel stamps in the C ABI (include/rt_abi.h): RtStampPlace's layout in ctypes, numpy and the header, the declarations, the
rule phrases and the history line in the header, the listed symbols, and a NULL context on all six calls.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytrace_amd import _lib, abi, render
from tests import stamp_edits as st
from tests.conftest import ROOT

pytestmark = pytest.mark.usefixtures("native_built")

CALLS = ("rt_stamp_create", "rt_stamp_capture", "rt_stamp_info", "rt_stamp_read", "rt_stamp_destroy", "rt_edit_stamps")


def _header():
    return open(os.path.join(ROOT, "include", "rt_abi.h")).read()


def test_place_record_layout_in_ctypes_numpy_and_the_header():
    assert C.sizeof(abi.RtStampPlace) == 32 == render.STAMP_PLACE_DTYPE.itemsize
    assert render.STAMP_PLACE_DTYPE == st.PLACE_DTYPE
    offsets = {"at": 0, "stamp": 12, "orient": 16, "where": 17, "reserved0": 18, "reserved": 20}
    for name, off in offsets.items():
        assert getattr(abi.RtStampPlace, name).offset == off, name
        assert render.STAMP_PLACE_DTYPE.fields[name][1] == off, name
    body = _header().split("typedef struct RtStampPlace {")[1].split("} RtStampPlace;")[0]
    fields = re.findall(r"^\s*(int32_t|uint32_t|uint8_t)\s+([^;]+);\s*/\*\s*(\d+)", body, flags=re.M)
    assert [(t, n.replace(" ", ""), int(o)) for t, n, o in fields] == [("int32_t", "at[3]", 0), ("uint32_t", "stamp", 12),
                                                                        ("uint8_t", "orient,where,reserved0[2]", 16), ("uint32_t", "reserved[3]", 20)]
    row = render.stamp_place(0x01020304, (-1, 2, 3), 47, abi.RT_WHERE_AIR)
    raw = row.tobytes()
    assert np.frombuffer(raw, "<i4", 3).tolist() == [-1, 2, 3] and raw[12:16] == bytes([4, 3, 2, 1]) and raw[16:] == bytes([47, 2]) + bytes(14)
    assert st.place(0x01020304, (-1, 2, 3), 47, st.WHERE_AIR).tobytes() == raw


def test_constants_declarations_rules_and_history_line():
    text = _header()
    for name, value in (("RT_STAMP_ABSENT", 0), ("RT_STAMP_AIR", 1), ("RT_STAMP_SOLID", 2)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), text) and getattr(abi, name) == value
    assert re.search(r"#define RT_STAMP_SKIP_AIR\s+0x1u", text) and abi.RT_STAMP_SKIP_AIR == 1
    assert (st.ABSENT, st.AIR, st.SOLID, st.SKIP_AIR) == (0, 1, 2, 1)
    flat = re.sub(r"\s+", " ", text)
    for decl in ("int rt_stamp_create (RtContext* ctx, const int32_t extent[3], const uint32_t* materials, const uint8_t* state, uint32_t* id_out);",
                 "int rt_stamp_capture(RtContext* ctx, const int32_t lo[3], const int32_t extent[3], uint32_t flags, uint32_t* id_out);",
                 "int rt_stamp_info (RtContext* ctx, uint32_t id, int32_t extent_out[3]);",
                 "int rt_stamp_read (RtContext* ctx, uint32_t id, uint32_t* materials, uint8_t* state);",
                 "int rt_stamp_destroy(RtContext* ctx, uint32_t id);",
                 "int rt_edit_stamps(RtContext* ctx, const RtStampPlace* places, uint32_t count);"):
        assert decl in flat, decl
    flat = flat.replace(" * ", " ")                                 # (comment continuation stars)
    for phrase in ("[ez][ey][ex], x fastest", "rt_stamp_read returns it as 0", "At most 1024 live stamps", "Ids: non-zero",
                   "A voxel is SOLID iff its minefield byte is 0", "no accumulation reset, no pending box, no prepass dropped",
                   "orient = p << 3 | f", "(0,1,2), (0,2,1), (1,0,2), (1,2,0), (2,0,1), (2,1,0)", "E'_k = E[perm[k]]",
                   "s[perm[k]] = (f >> perm[k]) & 1 ? E[perm[k]] - 1 - d_k : d_k", "orient >= 48 is invalid", "the other 24 mirror",
                   "[at, at + E') clipped to [0, R)^3", "shifted by +-R", "count > 4096", "[-4 R, 4 R]", "RT_ERR_NOT_READY",
                   "one pending box per placement that has a bounding box", "Undo: capture a box with flags 0",
                   "RtInfo.device_bytes counts live stamps; rt_destroy frees the rest"):
        assert phrase in flat, phrase
    assert re.search(r"Additive, same minor version: RtStampPlace, RT_STAMP_\*, rt_stamp_create, rt_stamp_capture, rt_stamp_info, rt_stamp_read,\s*\*\s*"
                     r"rt_stamp_destroy, rt_edit_stamps \(voxel stamps", text)
    assert "#define RT_ABI_VERSION_MINOR 3" in text


def test_the_six_symbols_are_listed_and_exported():
    lib = _lib.amd()
    for name in CALLS:
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name), name


def test_null_context_is_invalid_arg_on_all_six_calls():
    lib = _lib.amd()
    ext, lo, out = (C.c_int32 * 3)(2, 2, 2), (C.c_int32 * 3)(0, 0, 0), C.c_uint32(7)
    mats, state = np.zeros(8, np.uint32), np.full(8, 2, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    places = st.batch([st.place(1, (0, 0, 0))])
    assert lib.rt_stamp_create(None, ext, p(mats), p(state), C.byref(out)) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_stamp_capture(None, lo, ext, 0, C.byref(out)) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_stamp_info(None, 1, ext) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_stamp_read(None, 1, p(mats), p(state)) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_stamp_destroy(None, 1) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_edit_stamps(None, places.ctypes.data_as(C.POINTER(abi.RtStampPlace)), 1) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_edit_stamps(None, None, 0) == abi.RT_ERR_INVALID_ARG
    assert out.value == 7 and list(ext) == [2, 2, 2]
