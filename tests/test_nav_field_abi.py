"""The navigation fields (rt_nav_*) without a GPU: the records' layouts in ctypes, numpy and the header, the header's declarations,
rule phrases and history line, the exported symbols, the unchanged ABI version, a null context, and what make_nav_build refuses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytrace_amd import _lib, abi
from tests import nav_field_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
CALLS = ("rt_nav_create", "rt_nav_info", "rt_nav_read", "rt_nav_destroy", "rt_nav_build", "rt_nav_build_async", "rt_nav_sample", "rt_nav_sample_async")
LAYOUTS = {
    "RtNavBuild": (32, [("lo", 0), ("max_dist", 12), ("height", 16), ("max_climb", 17), ("max_drop", 18), ("goal_snap", 19), ("reserved", 20)]),
    "RtNavGoal": (16, [("cell", 0), ("reserved", 12)]),
    "RtNavResult": (32, [("standable", 0), ("reached", 4), ("levels", 8), ("truncated", 12), ("goals_used", 16), ("goals_dropped", 20), ("reserved", 24)]),
    "RtNavAgent": (16, [("pos", 0), ("snap_down", 12), ("snap_up", 13), ("reserved", 14)]),
    "RtNavStep": (32, [("cell", 0), ("dist", 12), ("next", 16), ("move", 28)]),
}


def _members(name):
    body = re.split(r"typedef struct %s\s*\{" % name, HEADER)[1].split("} %s;" % name)[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [m for decl in re.findall(r"(?:uint8_t|uint32_t|int32_t|float)\s+([^;]+);", body) for m in re.findall(r"([a-z_0-9]+)(?:\[\d\])?", decl)]


def test_structs_have_the_headers_sizes_and_offsets():
    for name, (size, offsets) in LAYOUTS.items():
        s = getattr(abi, name)
        assert C.sizeof(s) == size, name
        assert [(n, getattr(s, n).offset) for n, _ in s._fields_] == offsets, name
        assert _members(name) == [n for n, _ in offsets], name
        assert "%d bytes" % size in re.split(r"typedef struct %s\s*\{" % name, HEADER)[1].split("\n")[0] + HEADER.split("} %s;" % name)[1].split("\n")[0], name


def test_dtypes_match_the_structs_and_the_restatements_own():
    for name, mine, theirs in (("RtNavGoal", abi.NAV_GOAL_DTYPE, ref.GOAL_DTYPE), ("RtNavResult", abi.NAV_RESULT_DTYPE, ref.RESULT_DTYPE),
                               ("RtNavAgent", abi.NAV_AGENT_DTYPE, ref.AGENT_DTYPE), ("RtNavStep", abi.NAV_STEP_DTYPE, ref.STEP_DTYPE)):
        size, offsets = LAYOUTS[name]
        assert mine.itemsize == size == theirs.itemsize
        for n, off in offsets:
            assert mine.fields[n][1] == off == theirs.fields[n][1], (name, n)
    assert (abi.RT_NAV_UNREACHED, abi.RT_NAV_NO_MOVE) == (ref.UNREACHED, ref.NO_MOVE) == (0xFFFF, 0xFF)
    assert (abi.MAX_NAV_FIELDS, abi.MAX_NAV_EXTENT, abi.MAX_NAV_DIST, abi.MAX_NAV_GOALS, abi.MAX_NAV_AGENTS) == (64, 256, 4096, 4096, 1 << 20)


def test_header_declares_the_calls_the_rules_and_the_history_line():
    flat = re.sub(r"\s+", " ", HEADER)
    for decl in ("int rt_nav_create (RtContext* ctx, const int32_t extent[3], uint32_t* id_out);",
                 "int rt_nav_info (RtContext* ctx, uint32_t id, int32_t extent_out[3], int32_t lo_out[3], uint32_t* built_out);",
                 "int rt_nav_read (RtContext* ctx, uint32_t id, uint16_t* dist, uint8_t* move);", "int rt_nav_destroy(RtContext* ctx, uint32_t id);",
                 "int rt_nav_build(RtContext* ctx, uint32_t id, const RtNavBuild* params, const RtNavGoal* goals, uint32_t goal_count, RtNavResult* result);",
                 "int rt_nav_build_async(RtContext* ctx, uint32_t id, const RtNavBuild* params, const RtNavGoal* goals_dev, uint32_t goal_count, RtNavResult* result_dev);",
                 "int rt_nav_sample(RtContext* ctx, uint32_t id, const RtNavAgent* agents, uint32_t count, RtNavStep* steps);",
                 "int rt_nav_sample_async(RtContext* ctx, uint32_t id, const RtNavAgent* agents_dev, uint32_t count, RtNavStep* steps_dev);"):
        assert decl in flat, decl
    assert "Additive, same minor version: RtNavBuild, RtNavGoal, RtNavResult, RtNavAgent, RtNavStep, RT_NAV_*, rt_nav_create" in flat
    for phrase in ("Up is +z", "Under the box's low * z face is a floor", "Above its high z face everything counts as unoccupied", "there is no clipping",
                   "c is STANDABLE * iff c-z is occupied and CLEAR(c) >= height", "the LOWER of the two cells has CLEAR >= |k| + height", "Moves are directed",
                   "h | (k + 8) << 2", "h ascending and, inside one h, k descending", "duplicates count each time", "A build overwrites every cell of the field",
                   "exactly max_dist + 1", "MERGED by maximum", "ordered like rt_stamp_capture", "records no pending box", "A rejected call changes nothing",
                   "Out of scope: agents wider than one cell; diagonal moves; move costs other than 1; swimming or flying; entities as obstacles",
                   "an up axis other than +z; incremental repair after an edit", "tests/nav_field_ref.py", "Device work per build", "at most 64 fields are live",
                   "cell = next = (-1,-1,-1)", "Every record is written", "a field never built: RT_ERR_NOT_READY"):
        assert phrase in flat, phrase


def test_the_abi_version_is_unchanged():
    assert "#define RT_ABI_VERSION_MAJOR 1" in HEADER and "#define RT_ABI_VERSION_MINOR 3" in HEADER
    assert _lib.amd().rt_abi_version() == (1 << 16) | 3


def test_symbols_are_listed_and_exported():
    lib = _lib.amd()
    for name in CALLS:
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name), name


def test_null_context_is_invalid_arg_for_every_call():
    lib = _lib.amd()
    out = np.full(8, 77, np.uint32)
    p = out.ctypes.data_as(C.c_void_p)
    ext = (C.c_int32 * 3)(4, 4, 4)
    assert lib.rt_nav_create(None, ext, out.ctypes.data_as(C.POINTER(C.c_uint32))) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_nav_info(None, 1, ext, ext, None) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_nav_read(None, 1, p, p) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_nav_destroy(None, 1) == abi.RT_ERR_INVALID_ARG
    params = abi.make_nav_build((0, 0, 0), 8)
    for f in (lib.rt_nav_build, lib.rt_nav_build_async):
        assert f(None, 1, C.byref(params), p, 1, p) == abi.RT_ERR_INVALID_ARG
    for f in (lib.rt_nav_sample, lib.rt_nav_sample_async):
        assert f(None, 1, p, 1, p) == abi.RT_ERR_INVALID_ARG
    assert (out == 77).all() and list(ext) == [4, 4, 4]


def test_make_nav_build_builds_the_record_and_refuses_what_the_call_refuses():
    p = abi.make_nav_build((1, 2, 3), 77, height=3, max_climb=2, max_drop=8, goal_snap=5)
    assert bytes(p) == np.array([1, 2, 3, 77], "<i4").tobytes() + bytes([3, 2, 8, 5]) + bytes(12)
    assert ref.build_verdict(77, 3, 2, 8, 5, (0, 0, 0), 0, 1) == 0
    for bad in (dict(max_dist=0), dict(max_dist=4097), dict(height=0), dict(height=5), dict(max_climb=3), dict(max_climb=-1), dict(max_drop=9), dict(goal_snap=9)):
        with pytest.raises(ValueError):
            abi.make_nav_build((0, 0, 0), **dict(dict(max_dist=8), **bad))
    with pytest.raises(ValueError):
        abi.make_nav_build((0, 0), 8)
    goals = abi.make_nav_goals([[1, 2, 3], [-4, 5, 6]])
    assert goals.dtype == abi.NAV_GOAL_DTYPE and goals["cell"].tolist() == [[1, 2, 3], [-4, 5, 6]] and not goals["reserved"].any()
    agents = abi.make_nav_agents([[0.5, 1.5, 2.0]], 8, 2)
    assert agents.tobytes() == np.array([0.5, 1.5, 2.0], "<f4").tobytes() + bytes([8, 2, 0, 0])
