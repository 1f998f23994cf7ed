"""rt_draw_boxes / rt_draw_boxes_async without a GPU: the record's layout in ctypes, numpy and the header, the header's declarations
and history line, the exported symbols, a null context, and what make_draw_boxes, face_probes and check_draw_box_tensors refuse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytrace_amd import _lib, abi, render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rt_abi.h")).read()


def test_struct_is_32_bytes_with_the_headers_offsets():
    assert C.sizeof(abi.RtDrawBox) == 32
    assert [(n, getattr(abi.RtDrawBox, n).offset) for n, _ in abi.RtDrawBox._fields_] == [("lo", 0), ("material", 12), ("hi", 16), ("emission", 28)]
    assert abi.MAX_DRAW_BOXES == 4096


def test_dtype_matches_the_struct():
    dt = render.DRAW_BOX_DTYPE
    assert dt.itemsize == C.sizeof(abi.RtDrawBox)
    for name, _ in abi.RtDrawBox._fields_:
        assert dt.fields[name][1] == getattr(abi.RtDrawBox, name).offset
    rec = np.zeros(1, dtype=dt)
    rec["lo"], rec["material"], rec["hi"], rec["emission"] = (1, 2, 3), 0xABCDE, (4, 5, 6), 0xFF102030
    c = abi.RtDrawBox.from_buffer_copy(rec.tobytes())
    assert (list(c.lo), c.material, list(c.hi), c.emission) == ([1, 2, 3], 0xABCDE, [4, 5, 6], 0xFF102030)


def test_header_declares_the_record_the_calls_and_the_history_line():
    flat = re.sub(r"\s+", " ", HEADER)
    assert "typedef struct RtDrawBox { /* 32 bytes */ float lo[3]; uint32_t material;" in flat
    assert "float hi[3]; uint32_t emission;" in flat
    assert ("int rt_draw_boxes(RtContext* ctx, const RtUniforms* u, const RtDrawBox* boxes, const RtProbeLight* face_lights, "
            "uint32_t count);") in flat
    assert ("int rt_draw_boxes_async(RtContext* ctx, const RtUniforms* u, const RtDrawBox* boxes_dev, const RtProbeLight* "
            "face_lights_dev, uint32_t count);") in flat
    assert "Additive, same minor version: RtDrawBox, rt_draw_boxes, rt_draw_boxes_async (" in flat
    assert "#define RT_ABI_VERSION_MINOR 3" in HEADER
    # the rules a host relies on are in the header, not only in a design note
    for phrase in ("t_in > 0 and t_in < t_out", "the lowest index", "depth_f < RT_BUF_DEPTH_F32[pixel]", "count > 4096", "tests/draw_boxes_ref.py"):
        assert phrase in flat, phrase


def test_symbols_are_listed_and_exported():
    assert "rt_draw_boxes" in _lib.ABI_SYMBOLS and "rt_draw_boxes_async" in _lib.ABI_SYMBOLS
    lib = _lib.amd()
    assert hasattr(lib, "rt_draw_boxes") and hasattr(lib, "rt_draw_boxes_async")
    assert hasattr(_lib.host(), "rth_pipeline_set_boxes")


def test_null_context_is_invalid_arg_for_both_calls():
    lib = _lib.amd()
    u = abi.RtUniforms()
    boxes = render.make_draw_boxes([(0, 0, 0)], [(1, 1, 1)], 7)
    lights = np.zeros(6, dtype=render.PROBE_LIGHT_DTYPE)
    pb, pl = boxes.ctypes.data_as(C.c_void_p), lights.ctypes.data_as(C.c_void_p)
    assert lib.rt_draw_boxes(None, C.byref(u), pb, pl, 1) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_draw_boxes_async(None, C.byref(u), pb, pl, 1) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_draw_boxes(None, None, None, None, 0) == abi.RT_ERR_INVALID_ARG


def test_make_draw_boxes_builds_records_and_refuses_invalid_boxes():
    b = render.make_draw_boxes([(0, 1, 2), (-5, -5, -5)], [(1, 2, 3), (5, 5, 5)], [3, 4])
    assert b.dtype == render.DRAW_BOX_DTYPE and b.size == 2
    assert b["lo"].tolist() == [[0, 1, 2], [-5, -5, -5]] and b["hi"].tolist() == [[1, 2, 3], [5, 5, 5]]
    assert b["material"].tolist() == [3, 4] and b["emission"].tolist() == [0xFF000000] * 2
    assert render.make_draw_boxes(np.zeros((0, 3)), np.zeros((0, 3)), 0).size == 0
    two22 = 4194304.0
    render.make_draw_boxes([(-two22, 0, 0)], [(two22, 1, 1)], 0)                      # the bound itself is inside
    for lo, hi in (((0, 0, 0), (1, 1, 0)), ((0, 0, 0), (1, -1, 1)), ((np.nan, 0, 0), (1, 1, 1)), ((0, 0, 0), (np.inf, 1, 1)),
                   ((0, 0, 0), (1, 1, 4194305.0)), ((-4194305.0, 0, 0), (1, 1, 1))):
        with pytest.raises(ValueError):
            render.make_draw_boxes([lo], [hi], 0)
    with pytest.raises(ValueError):
        render.make_draw_boxes(np.zeros((2, 3)), np.ones((3, 3)), 0)
    with pytest.raises(ValueError):
        render.make_draw_boxes(np.zeros((4097, 3)), np.ones((4097, 3)), 0)


def test_face_probes_sit_just_off_each_face():
    b = render.make_draw_boxes([(0, 10, 20), (1, 1, 1)], [(2, 14, 26), (2, 2, 2)], 0)
    p = render.face_probes(b, cells=[(3, 4), (5, 6)])
    assert p.dtype == render.PROBE_DTYPE and p.size == 12
    assert p["normal"].tolist() == list(range(6)) * 2
    assert p["cell"].tolist() == [[3, 4]] * 6 + [[5, 6]] * 6
    assert not p["reserved"].any()
    e = np.float32(0.001)
    want = [(np.float32(2) + e, 12, 23), (np.float32(0) - e, 12, 23), (1, np.float32(14) + e, 23), (1, np.float32(10) - e, 23),
            (1, 12, np.float32(26) + e), (1, 12, np.float32(20) - e)]
    assert p["position"][:6].tolist() == np.array(want, dtype=np.float32).tolist()
    # code 2a + 1 is the face a ray with d_a > 0 enters through: the low one
    assert p["position"][7][0] < 1 < 2 < p["position"][6][0]


def test_check_draw_box_tensors_refuses_what_the_kernel_could_not_read():
    import torch
    boxes = torch.zeros((2, 8), dtype=torch.float32)
    lights = torch.zeros((12, 4), dtype=torch.float32)
    with pytest.raises(ValueError, match="cuda"):
        render.check_draw_box_tensors(boxes, lights, 0)                # host tensors
    with pytest.raises(ValueError, match="boxes must be a torch tensor"):
        render.check_draw_box_tensors(np.zeros((2, 8), np.float32), lights, 0)
    with pytest.raises(ValueError, match="face_lights must be a torch tensor"):
        render.check_draw_box_tensors(boxes, None, 0)
