"""rt_shadow_entities / rt_shadow_entities_async without a GPU: the header's declarations, rule phrases and history line, the
unchanged ABI version, the exported symbols, every refusal that needs no device, what check_shadow_box_tensor refuses, and the host
checks (raytrace_amd/csrc/api/shadows_check.hpp) run by tests/entity_shadows_main.cpp as a program of its own under the address and
undefined-behaviour sanitizers.  Nothing sanitized is loaded into this process."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from raytrace_amd import _lib, abi, render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
SRC = os.path.join(ROOT, "tests", "entity_shadows_main.cpp")
BASE = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_header_declares_the_calls_the_rules_and_the_history_line():
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*(?=\s)", " ", HEADER))     # comment continuations joined: a rule may cross a line
    assert ("int rt_shadow_entities(RtContext* ctx, const RtUniforms* u, const RtDrawBox* boxes, uint32_t nboxes, const RtDrawStamp* models, "
            "uint32_t nmodels, float strength);") in flat
    assert ("int rt_shadow_entities_async(RtContext* ctx, const RtUniforms* u, const RtDrawBox* boxes_dev, uint32_t nboxes, "
            "const RtDrawStamp* models, uint32_t nmodels, float strength);") in flat
    assert "Additive, same minor version: rt_shadow_entities, rt_shadow_entities_async (" in flat
    # the rules a host relies on are in the header, not only in a design note
    for phrase in ("Entity shadows", "o = P', d = s and inv_k = 1.0f / s_k", "t_out > 0 and t_in < t_out", "t_out > 0 in place of t_in > 0",
                   "it is NOT jittered", "on EVERY axis p = o_k", "walk steps (1) to (3) unchanged", "leaves the window (RT_HIT_AIR)",
                   "sub_k = (sunlight_k * strength) / 16.0f", "rtm_max(L_k - sub_k, 0.0f)",
                   "rtm_unorm(rtm_max(float(q_k) / 65535.0f - sub_k, 0.0f), 65535.0f)", "strength not finite or outside (0, 1]",
                   "sunlight == (0, 0, 0): RT_OK", "tests/entity_shadow_ref.py", "Hard shadows only".lower(), "point lights still ignore entities",
                   "boxes, models, shadows, point lights, denoise"):
        assert phrase in flat, phrase


def test_the_abi_version_is_unchanged():
    assert "#define RT_ABI_VERSION_MAJOR 1" in HEADER and "#define RT_ABI_VERSION_MINOR 3" in HEADER
    assert _lib.amd().rt_abi_version() == (1 << 16) | 3


def test_symbols_are_listed_and_exported():
    assert "rt_shadow_entities" in _lib.ABI_SYMBOLS and "rt_shadow_entities_async" in _lib.ABI_SYMBOLS
    lib = _lib.amd()
    assert hasattr(lib, "rt_shadow_entities") and hasattr(lib, "rt_shadow_entities_async")
    assert hasattr(_lib.host(), "rth_pipeline_enable_entity_shadows")
    assert hasattr(render.Context, "shadow_entities") and hasattr(render.Context, "shadow_entities_async")
    assert hasattr(render.Pipeline, "enable_entity_shadows")


def test_null_context_is_invalid_arg_for_both_calls():
    lib = _lib.amd()
    u = abi.RtUniforms()
    boxes = np.zeros(1, dtype=render.DRAW_BOX_DTYPE)
    boxes["hi"] = 1.0
    p = boxes.ctypes.data_as(C.c_void_p)
    for call in (lib.rt_shadow_entities, lib.rt_shadow_entities_async):
        assert call(None, C.byref(u), p, 1, None, 0, 1.0) == abi.RT_ERR_INVALID_ARG
        assert call(None, None, None, 0, None, 0, 1.0) == abi.RT_ERR_INVALID_ARG
        assert call(None, C.byref(u), None, 0, None, 0, 0.5) == abi.RT_ERR_INVALID_ARG


def test_check_shadow_box_tensor_refuses_what_the_kernel_could_not_read():
    import torch
    with pytest.raises(ValueError, match="cuda"):
        render.check_shadow_box_tensor(torch.zeros((2, 8), dtype=torch.float32), 0)                  # a host tensor
    with pytest.raises(ValueError, match="torch tensor"):
        render.check_shadow_box_tensor(np.zeros((2, 8), np.float32), 0)


def _build(exe):
    """With the sanitizers (their runtimes linked into the program where the compiler has the archives); without them where it has
    no runtime at all: the comparison with the model runs either way."""
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []):
        r = subprocess.run(BASE + extra + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            return extra, r
    raise AssertionError("entity_shadows_main.cpp does not compile:\n" + r.stderr[-4000:])


def test_the_host_checks_match_their_model_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "entity_shadows_main")
    flags, _ = _build(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "flags %s\n%s\n%s" % (" ".join(flags), r.stdout[-2000:], r.stderr[-6000:])
    assert "all cases match the model" in r.stdout
