"""rt_add_lights / rt_add_lights_async without a GPU: the record's layout in ctypes, numpy and the header, the header's declarations,
rule phrases and history line, the exported symbols, a null context, what make_point_lights and check_point_light_tensors refuse, and
the record's validity test (raytrace_amd/csrc/api/lights_check.hpp) run by tests/point_lights_main.cpp as a program of its own under
the address and undefined-behaviour sanitizers.  Nothing sanitized is loaded into this process."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from raytrace_amd import _lib, abi, render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
SRC = os.path.join(ROOT, "tests", "point_lights_main.cpp")
BASE = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_struct_is_32_bytes_with_the_headers_offsets():
    assert C.sizeof(abi.RtPointLight) == 32
    assert [(n, getattr(abi.RtPointLight, n).offset) for n, _ in abi.RtPointLight._fields_] == [("position", 0), ("radius", 12), ("color", 16),
                                                                                                ("reserved", 28)]
    assert abi.MAX_POINT_LIGHTS == 1024


def test_dtype_matches_the_struct():
    dt = render.POINT_LIGHT_DTYPE
    assert dt.itemsize == C.sizeof(abi.RtPointLight)
    for name, _ in abi.RtPointLight._fields_:
        assert dt.fields[name][1] == getattr(abi.RtPointLight, name).offset
    rec = np.zeros(1, dtype=dt)
    rec["position"], rec["radius"], rec["color"], rec["reserved"] = (1, 2, 3), 7.5, (4, 5, 6), 9
    c = abi.RtPointLight.from_buffer_copy(rec.tobytes())
    assert (list(c.position), c.radius, list(c.color), c.reserved) == ([1, 2, 3], 7.5, [4, 5, 6], 9)


def test_header_declares_the_record_the_calls_the_rules_and_the_history_line():
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*(?=\s)", " ", HEADER))     # comment continuations joined: a rule may cross a line
    assert "typedef struct RtPointLight { /* 32 bytes */ float position[3]; float radius;" in flat
    assert "float color[3]; uint32_t reserved;" in flat
    assert "int rt_add_lights(RtContext* ctx, const RtUniforms* u, const RtPointLight* lights, uint32_t count);" in flat
    assert "int rt_add_lights_async(RtContext* ctx, const RtUniforms* u, const RtPointLight* lights_dev, uint32_t count);" in flat
    assert "Additive, same minor version: RtPointLight, rt_add_lights, rt_add_lights_async (" in flat
    assert "#define RT_ABI_VERSION_MINOR 3" in HEADER
    # the rules a host relies on are in the header, not only in a design note
    for phrase in ("0.03125f", "dist2 < r2", "after the sky test (:138-145) found the new position inside the window and before the hit test (:146)",
                   "rtm_dot3(pos - P', pos - P') >= dist2", "w = (cosine * (x * x)) / (1.0f + dist2)", "count > 1024",
                   "tests/point_light_ref.py", "rtm_unorm(float(q_k) / 65535.0f + s_k, 65535.0f)"):
        assert phrase in flat, phrase


def test_symbols_are_listed_and_exported():
    assert "rt_add_lights" in _lib.ABI_SYMBOLS and "rt_add_lights_async" in _lib.ABI_SYMBOLS
    lib = _lib.amd()
    assert hasattr(lib, "rt_add_lights") and hasattr(lib, "rt_add_lights_async")
    assert hasattr(_lib.host(), "rth_pipeline_set_lights")


def test_null_context_is_invalid_arg_for_both_calls():
    lib = _lib.amd()
    u = abi.RtUniforms()
    lights = render.make_point_lights([(0, 0, 0)], 4.0, (1, 1, 1))
    p = lights.ctypes.data_as(C.c_void_p)
    assert lib.rt_add_lights(None, C.byref(u), p, 1) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_add_lights_async(None, C.byref(u), p, 1) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_add_lights(None, None, None, 0) == abi.RT_ERR_INVALID_ARG


def test_make_point_lights_builds_records_and_refuses_invalid_lights():
    l = render.make_point_lights([(0, 1, 2), (-5, -5, -5)], [3.0, 4.0], (1.0, 0.5, 0.0))
    assert l.dtype == render.POINT_LIGHT_DTYPE and l.size == 2
    assert l["position"].tolist() == [[0, 1, 2], [-5, -5, -5]] and l["radius"].tolist() == [3.0, 4.0]
    assert l["color"].tolist() == [[1.0, 0.5, 0.0]] * 2 and l["reserved"].tolist() == [0, 0]
    assert render.make_point_lights(np.zeros((0, 3)), 1.0, (0, 0, 0)).size == 0
    two22, two20 = 4194304.0, 1048576.0
    render.make_point_lights([(-two22, two22, 0)], 1024.0, (two20, 0, 0))             # the bounds themselves are inside
    for pos, radius, color in (((np.nan, 0, 0), 1, (1, 1, 1)), ((0, np.inf, 0), 1, (1, 1, 1)), ((4194305.0, 0, 0), 1, (1, 1, 1)),
                               ((0, 0, -4194305.0), 1, (1, 1, 1)), ((0, 0, 0), 0.0, (1, 1, 1)), ((0, 0, 0), -1.0, (1, 1, 1)),
                               ((0, 0, 0), 1024.5, (1, 1, 1)), ((0, 0, 0), np.nan, (1, 1, 1)), ((0, 0, 0), 1, (-0.5, 1, 1)),
                               ((0, 0, 0), 1, (1, 1, 1048577.0)), ((0, 0, 0), 1, (1, np.nan, 1)), ((0, 0, 0), np.inf, (1, 1, 1))):
        with pytest.raises(ValueError):
            render.make_point_lights([pos], radius, color)
    with pytest.raises(ValueError):
        render.make_point_lights(np.zeros((1025, 3)), 1.0, (1, 1, 1))


def test_check_point_light_tensors_refuses_what_the_kernel_could_not_read():
    import torch
    with pytest.raises(ValueError, match="cuda"):
        render.check_point_light_tensors(torch.zeros((2, 8), dtype=torch.float32), 0)                # a host tensor
    with pytest.raises(ValueError, match="torch tensor"):
        render.check_point_light_tensors(np.zeros((2, 8), np.float32), 0)


def _build(exe):
    """With the sanitizers (their runtimes linked into the program where the compiler has the archives); without them where it has
    no runtime at all: the comparison with the model runs either way."""
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []):
        r = subprocess.run(BASE + extra + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            return extra, r
    raise AssertionError("point_lights_main.cpp does not compile:\n" + r.stderr[-4000:])


def test_the_validity_check_matches_its_model_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "point_lights_main")
    flags, _ = _build(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "flags %s\n%s\n%s" % (" ".join(flags), r.stdout[-2000:], r.stderr[-6000:])
    assert "all cases match the model" in r.stdout
