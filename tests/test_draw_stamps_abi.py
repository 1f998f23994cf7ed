"""rt_draw_stamps / rt_draw_stamps_async without a GPU: the record's layout in ctypes, numpy, the restatement and the header, the
header's declarations and history line, the exported symbols, a null context, and what make_draw_stamps, stamp_face_probes and
check_draw_stamp_lights build and refuse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytrace_amd import _lib, abi, render
from tests import draw_stamps_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rt_abi.h")).read()


def test_struct_is_32_bytes_with_the_headers_offsets():
    assert C.sizeof(abi.RtDrawStamp) == 32
    assert [(n, getattr(abi.RtDrawStamp, n).offset) for n, _ in abi.RtDrawStamp._fields_] == [
        ("origin", 0), ("scale", 12), ("stamp", 16), ("orient", 20), ("reserved0", 21), ("emission", 24), ("reserved", 28)]
    assert abi.MAX_DRAW_STAMPS == 4096 == ref.MAX_MODELS


def test_dtype_matches_the_struct_and_the_restatements():
    dt = render.DRAW_STAMP_DTYPE
    assert dt.itemsize == C.sizeof(abi.RtDrawStamp) and dt == ref.MODEL_DTYPE
    for name, _ in abi.RtDrawStamp._fields_:
        assert dt.fields[name][1] == getattr(abi.RtDrawStamp, name).offset
    rec = np.zeros(1, dtype=dt)
    rec["origin"], rec["scale"], rec["stamp"], rec["orient"], rec["emission"] = (1, 2, 3), 0.25, 0xABCDE, 47, 0xFF102030
    c = abi.RtDrawStamp.from_buffer_copy(rec.tobytes())
    assert (list(c.origin), c.scale, c.stamp, c.orient, list(c.reserved0), c.emission, c.reserved) == ([1, 2, 3], 0.25, 0xABCDE, 47, [0, 0, 0], 0xFF102030, 0)


def test_header_declares_the_record_the_calls_and_the_history_line():
    flat = re.sub(r"\s+", " ", HEADER)
    assert "typedef struct RtDrawStamp { /* 32 bytes */ float origin[3];" in flat
    for field in ("float scale;", "uint32_t stamp;", "uint8_t orient, reserved0[3];", "uint32_t emission;", "uint32_t reserved;"):
        assert field in flat[flat.index("typedef struct RtDrawStamp"):flat.index("} RtDrawStamp;")], field
    assert ("int rt_draw_stamps(RtContext* ctx, const RtUniforms* u, const RtDrawStamp* models, const RtProbeLight* face_lights, "
            "uint32_t count);") in flat
    assert ("int rt_draw_stamps_async(RtContext* ctx, const RtUniforms* u, const RtDrawStamp* models, const RtProbeLight* "
            "face_lights_dev, uint32_t count);") in flat
    assert "Additive, same minor version: RtDrawStamp, rt_draw_stamps, rt_draw_stamps_async (" in flat
    assert "#define RT_ABI_VERSION_MINOR 3" in HEADER
    # the rules a host relies on are in the header, not only in a design note
    for phrase in ("tests/draw_stamps_ref.py", "hi_k = rtm_fma(float(E'_k), scale, origin_k)", "2^-8 <= scale <= 64", "c_a = d_a > 0 ? 0 : E'_a - 1",
                   "t = t < tk ? tk : t", "so the lowest axis", "E'_x + E'_y + E'_z", "a camera inside the bounding box does not see the model",
                   "count > 4096", "rt_stamp_destroy after an enqueued draw waits for it", "RT_STAMP_ABSENT are both see-through"):
        assert phrase in flat, phrase


def test_symbols_are_listed_and_exported():
    assert "rt_draw_stamps" in _lib.ABI_SYMBOLS and "rt_draw_stamps_async" in _lib.ABI_SYMBOLS
    lib = _lib.amd()
    assert hasattr(lib, "rt_draw_stamps") and hasattr(lib, "rt_draw_stamps_async")
    assert hasattr(_lib.host(), "rth_pipeline_set_models")


def test_null_context_is_invalid_arg_for_both_calls():
    lib = _lib.amd()
    u = abi.RtUniforms()
    models = render.make_draw_stamps(1025, [(0, 0, 0)])
    lights = np.zeros(6, dtype=render.PROBE_LIGHT_DTYPE)
    pm, pl = models.ctypes.data_as(C.c_void_p), lights.ctypes.data_as(C.c_void_p)
    assert lib.rt_draw_stamps(None, C.byref(u), pm, pl, 1) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_draw_stamps_async(None, C.byref(u), pm, pl, 1) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_draw_stamps(None, None, None, None, 0) == abi.RT_ERR_INVALID_ARG


def test_make_draw_stamps_builds_records_and_refuses_what_needs_no_extent():
    m = render.make_draw_stamps([1025, 2050], [(0, 1, 2), (-5, -5, -5)], [0.0625, 2.5], [0, 47], 0xFF000007)
    assert m.dtype == render.DRAW_STAMP_DTYPE and m.size == 2
    assert m["origin"].tolist() == [[0, 1, 2], [-5, -5, -5]] and m["scale"].tolist() == [0.0625, 2.5]
    assert m["stamp"].tolist() == [1025, 2050] and m["orient"].tolist() == [0, 47] and m["emission"].tolist() == [0xFF000007] * 2
    assert not m["reserved0"].any() and not m["reserved"].any()
    assert render.make_draw_stamps(1, np.zeros((0, 3))).size == 0
    assert render.make_draw_stamps(1, np.zeros((3, 3)))["scale"].tolist() == [1.0] * 3
    two22 = 4194304.0
    render.make_draw_stamps(1, [(-two22, two22, 0)], 1.0 / 256.0)                      # the bounds themselves are inside
    render.make_draw_stamps(1, [(0, 0, 0)], 64.0)
    for origin, scale, orient in (((np.nan, 0, 0), 1, 0), ((0, np.inf, 0), 1, 0), ((0, 0, 4194305.0), 1, 0), ((0, 0, 0), np.nan, 0),
                                  ((0, 0, 0), 0.003, 0), ((0, 0, 0), 64.5, 0), ((0, 0, 0), 1, 48), ((0, 0, 0), 1, -1)):
        with pytest.raises(ValueError):
            render.make_draw_stamps(1, [origin], scale, orient)
    with pytest.raises(ValueError):
        render.make_draw_stamps(1, np.zeros((4097, 3)))


def test_stamp_face_probes_sit_just_off_each_face_of_the_oriented_bounding_box():
    m = render.make_draw_stamps(1, [(0, 10, 20), (1, 1, 1)], [0.5, 1.0], [0, 3 << 3])     # perm 3: (1, 2, 0)
    lo, hi = render.stamp_bounding_boxes(m, (4, 8, 12))
    assert lo.tolist() == [[0, 10, 20], [1, 1, 1]] and hi.tolist() == [[2, 14, 26], [9, 13, 5]]
    stamps = {1: (np.zeros((12, 8, 4), np.uint32), np.zeros((12, 8, 4), np.uint8))}
    assert np.array_equal(hi, ref.high_corners(m, ref.placed_extents(m, stamps)))
    p = render.stamp_face_probes(m, (4, 8, 12), cells=[(3, 4), (5, 6)])
    assert p.dtype == render.PROBE_DTYPE and p.size == 12
    assert p["normal"].tolist() == list(range(6)) * 2 and p["cell"].tolist() == [[3, 4]] * 6 + [[5, 6]] * 6
    e = np.float32(0.001)
    want = [(np.float32(2) + e, 12, 23), (np.float32(0) - e, 12, 23), (1, np.float32(14) + e, 23), (1, np.float32(10) - e, 23),
            (1, 12, np.float32(26) + e), (1, 12, np.float32(20) - e)]
    assert p["position"][:6].tolist() == np.array(want, dtype=np.float32).tolist()
    per_model = render.stamp_face_probes(m, [(4, 8, 12), (1, 1, 1)])
    assert per_model["position"][:6].tolist() == p["position"][:6].tolist() and per_model["position"][6][0] == np.float32(2) + e


def test_check_draw_stamp_lights_refuses_what_the_kernel_could_not_read():
    import torch
    lights = torch.zeros((12, 4), dtype=torch.float32)
    with pytest.raises(ValueError, match="cuda"):
        render.check_draw_stamp_lights(2, lights, 0)                    # a host tensor
    with pytest.raises(ValueError, match="torch tensor"):
        render.check_draw_stamp_lights(2, np.zeros((12, 4), np.float32), 0)
    with pytest.raises(ValueError, match="torch tensor"):
        render.check_draw_stamp_lights(2, None, 0)
