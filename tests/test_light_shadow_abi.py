"""rt_add_lights_occluded / rt_add_lights_occluded_async without a GPU: the header's declarations, rule phrases and history line, the
unchanged ABI version, the exported symbols, every refusal that needs no device, and the host checks
(raytrace_amd/csrc/api/light_shadows_check.hpp) run by tests/light_shadows_main.cpp as a program of its own under the address and
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
SRC = os.path.join(ROOT, "tests", "light_shadows_main.cpp")
BASE = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_header_declares_the_calls_the_rules_and_the_history_line():
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*(?=\s)", " ", HEADER))     # comment continuations joined: a rule may cross a line
    assert ("int rt_add_lights_occluded(RtContext* ctx, const RtUniforms* u, const RtPointLight* lights, uint32_t count, const RtDrawBox* boxes, "
            "uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels);") in flat
    assert ("int rt_add_lights_occluded_async(RtContext* ctx, const RtUniforms* u, const RtPointLight* lights_dev, uint32_t count, "
            "const RtDrawBox* boxes_dev, uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels);") in flat
    assert "Additive, same minor version: rt_add_lights_occluded, rt_add_lights_occluded_async (" in flat
    # the rules a host relies on are in the header, not only in a design note
    for phrase in ("Point-light shadows of entities", "o = P'; d = rtm_normalize3(v)", "inv_k = 1.0f / d_k", "len = rtm_sqrt(dist2)",
                   "t_out > 0 and t_in < t_out — and also t_in < len", "a box beyond the light does not shade it",
                   "a light inside a box lights nothing outside it", "one added stop between (2) and (3)", "is not < len",
                   "a solid cell of the same model behind the light does not block", "the call is rt_add_lights, every bit and every side effect",
                   "tests/light_shadow_ref.py", "hard shadows only", 'No per-light "owner" exemption', "Bounce light still ignores entities",
                   "count == 0: RT_OK, nothing enqueued, no prepass dropped, whatever the occluder counts",
                   "rt_stamp_destroy after an enqueued call waits for it"):
        assert phrase in flat, phrase
    # the two sentences that named the hole point at the call that fills it
    assert "shadow in a point light here (rt_add_lights_occluded is the call in which they do)" in flat
    assert "in rt_add_lights point lights still ignore entities (rt_add_lights_occluded is the call in which they do not)" in flat


def test_the_abi_version_is_unchanged():
    assert "#define RT_ABI_VERSION_MAJOR 1" in HEADER and "#define RT_ABI_VERSION_MINOR 3" in HEADER
    assert _lib.amd().rt_abi_version() == (1 << 16) | 3


def test_symbols_are_listed_and_exported():
    assert "rt_add_lights_occluded" in _lib.ABI_SYMBOLS and "rt_add_lights_occluded_async" in _lib.ABI_SYMBOLS
    assert _lib.AMD_FUNCTIONS["rt_add_lights_occluded"] == _lib.AMD_FUNCTIONS["rt_add_lights_occluded_async"]
    assert len(_lib.AMD_FUNCTIONS["rt_add_lights_occluded"][1]) == 8
    lib = _lib.amd()
    assert hasattr(lib, "rt_add_lights_occluded") and hasattr(lib, "rt_add_lights_occluded_async")
    assert hasattr(_lib.host(), "rth_pipeline_enable_light_shadows")
    assert hasattr(render.Context, "add_lights_occluded") and hasattr(render.Context, "add_lights_occluded_async")
    assert hasattr(render.Pipeline, "enable_light_shadows")


def test_null_context_is_invalid_arg_for_both_calls():
    lib = _lib.amd()
    u = abi.RtUniforms()
    lights = render.make_point_lights([(0.0, 0.0, 0.0)], 4.0, (1.0, 1.0, 1.0))
    boxes = np.zeros(1, dtype=render.DRAW_BOX_DTYPE)
    boxes["hi"] = 1.0
    pl, pb = lights.ctypes.data_as(C.c_void_p), boxes.ctypes.data_as(C.c_void_p)
    for call in (lib.rt_add_lights_occluded, lib.rt_add_lights_occluded_async):
        assert call(None, C.byref(u), pl, 1, pb, 1, None, 0) == abi.RT_ERR_INVALID_ARG
        assert call(None, None, None, 0, None, 0, None, 0) == abi.RT_ERR_INVALID_ARG
        assert call(None, C.byref(u), None, 0, None, 0, None, 0) == abi.RT_ERR_INVALID_ARG


def test_the_async_binding_refuses_what_the_kernel_could_not_read():
    import torch
    with pytest.raises(ValueError, match="cuda"):
        render.check_point_light_tensors(torch.zeros((2, 8), dtype=torch.float32), 0)                  # a host tensor
    with pytest.raises(ValueError, match="torch tensor"):
        render.check_shadow_box_tensor(np.zeros((2, 8), np.float32), 0)


def _build(exe):
    """With the sanitizers (their runtimes linked into the program where the compiler has the archives); without them where it has
    no runtime at all: the comparison with the model runs either way."""
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []):
        r = subprocess.run(BASE + extra + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            return extra, r
    raise AssertionError("light_shadows_main.cpp does not compile:\n" + r.stderr[-4000:])


def test_the_host_checks_match_their_model_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "light_shadows_main")
    flags, _ = _build(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "flags %s\n%s\n%s" % (" ".join(flags), r.stdout[-2000:], r.stderr[-6000:])
    assert "all cases match the model" in r.stdout
