"""rt_trace_entities / rt_trace_entities_async / rt_pick_entities without a GPU: the header's declarations, struct, rule phrases and
history line, the unchanged ABI version, the exported symbols, the refusal that needs no device, what check_entity_query_tensors
refuses, and the host checks (raytrace_amd/csrc/api/entity_query_check.hpp) run by tests/entity_query_main.cpp as a program of its
own under the address and undefined-behaviour sanitizers.  Nothing sanitized is loaded into this process."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from raytrace_amd import _lib, abi, render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
SRC = os.path.join(ROOT, "tests", "entity_query_main.cpp")
BASE = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_header_declares_the_calls_the_struct_the_rules_and_the_history_line():
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*(?=\s)", " ", HEADER))     # comment continuations joined: a rule may cross a line
    assert ("int rt_trace_entities(RtContext* ctx, const RtRay* rays, uint32_t count, const int32_t lr[3], const RtDrawBox* boxes, uint32_t nboxes, "
            "const RtDrawStamp* models, uint32_t nmodels, RtRayHit* world_hits, RtEntityHit* entity_hits);") in flat
    assert ("int rt_trace_entities_async(RtContext* ctx, const RtRay* rays_dev, uint32_t count, const int32_t lr[3], const RtDrawBox* boxes_dev, "
            "uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels, RtRayHit* world_hits_dev, RtEntityHit* entity_hits_dev);") in flat
    assert ("int rt_pick_entities(RtContext* ctx, const RtUniforms* u, const int32_t* xy, uint32_t count, const RtDrawBox* boxes, uint32_t nboxes, "
            "const RtDrawStamp* models, uint32_t nmodels, RtRayHit* world_hits, RtEntityHit* entity_hits);") in flat
    assert "typedef struct RtEntityHit { /* 48 bytes */" in flat
    for define in ("#define RT_ENTITY_NONE 0", "#define RT_ENTITY_BOX 1", "#define RT_ENTITY_MODEL 2"):
        assert define in flat
    assert "Additive, same minor version: RtEntityHit, RT_ENTITY_*, rt_trace_entities, rt_trace_entities_async, rt_pick_entities (" in flat
    # the rules a host relies on are in the header, not only in a design note
    for phrase in ("Entity queries", "d = rtm_normalize3(direction)", "o = u.origin, the same sx, sy and rtm_normalize3, and NO slide",
                   "inv_k = 1.0f / d_k", "exactly what rt_trace_rays writes", "exactly what rt_pick_pixels writes",
                   "t_in > 0 and t_in < t_out", "a mob never hits its own box", "with the ray's o in place of the camera's",
                   "on equal t boxes come before models", "the lowest index wins", "P_k = rtm_fma(d_k, t, o_k)",
                   "depth_f = rtm_length3(o - P) * 32.0f", "D = 65535.0f if the world hit's kind is RT_HIT_AIR",
                   "a limit exit counts as a hit there", "reported iff depth_f < D", "the world wins ties", "a NaN D reports none",
                   "normal = 2 axis + 1 if d_axis > 0, else 2 axis", "kind RT_ENTITY_NONE, index = 0xFFFFFFFF, normal = 6",
                   "Every byte of every record is written", "count > 2^24", "nboxes or nmodels above 4096",
                   "the device skips an invalid box", "No world resident: RT_ERR_NOT_READY", "count == 0: RT_OK, nothing enqueued",
                   "rt_stamp_destroy after an enqueued call waits for it", "tests/entity_query_ref.py",
                   "rays x entities slab tests", "Send rays that lie together in consecutive order",
                   "no acceleration structure over entities", "`models` is a HOST pointer"):
        assert phrase in flat, phrase


def test_the_abi_version_is_unchanged():
    assert "#define RT_ABI_VERSION_MAJOR 1" in HEADER and "#define RT_ABI_VERSION_MINOR 3" in HEADER
    assert _lib.amd().rt_abi_version() == (1 << 16) | 3


def test_symbols_are_listed_and_exported():
    lib = _lib.amd()
    for name in ("rt_trace_entities", "rt_trace_entities_async", "rt_pick_entities"):
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name)
    assert hasattr(_lib.host(), "rth_pipeline_pick_entity")
    for method in ("trace_entities", "trace_entities_async", "pick_entities"):
        assert hasattr(render.Context, method)
    assert hasattr(render.Pipeline, "pick_entity")
    assert (abi.RT_ENTITY_NONE, abi.RT_ENTITY_BOX, abi.RT_ENTITY_MODEL) == (0, 1, 2)
    assert render.ENTITY_HIT_DTYPE.itemsize == C.sizeof(abi.RtEntityHit) == 48
    for field in ("position", "t", "kind", "index", "normal", "material", "cell", "voxel"):
        assert render.ENTITY_HIT_DTYPE.fields[field][1] == getattr(abi.RtEntityHit, field).offset


def test_null_context_is_invalid_arg_for_all_three_calls():
    lib = _lib.amd()
    u = abi.RtUniforms()
    lr = (C.c_int32 * 3)(0, 0, 0)
    rays = np.zeros((1, 8), dtype=np.float32)
    xy = np.zeros((1, 2), dtype=np.int32)
    boxes = np.zeros(1, dtype=render.DRAW_BOX_DTYPE)
    boxes["hi"] = 1.0
    world, hits = np.zeros(1, dtype=render.HIT_DTYPE), np.full(1, 0x5A, dtype=np.uint8).repeat(48)
    before = hits.copy()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for call in (lib.rt_trace_entities, lib.rt_trace_entities_async):
        assert call(None, p(rays), 1, lr, p(boxes), 1, None, 0, p(world), p(hits)) == abi.RT_ERR_INVALID_ARG
        assert call(None, None, 0, None, None, 0, None, 0, None, None) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_pick_entities(None, C.byref(u), p(xy), 1, p(boxes), 1, None, 0, p(world), p(hits)) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_pick_entities(None, None, None, 0, None, 0, None, 0, None, None) == abi.RT_ERR_INVALID_ARG
    assert np.array_equal(hits, before) and not world.view(np.uint8).any()


def test_check_entity_query_tensors_refuses_what_the_kernel_could_not_read():
    import torch
    rays, hits = torch.zeros((2, 8), dtype=torch.float32), torch.zeros((2, 48), dtype=torch.uint8)
    with pytest.raises(ValueError, match="cuda"):
        render.check_entity_query_tensors(rays, None, None, hits, 0)                                  # host tensors
    with pytest.raises(ValueError, match="torch tensor"):
        render.check_entity_query_tensors(np.zeros((2, 8), np.float32), None, None, hits, 0)
    with pytest.raises(ValueError, match="torch tensor"):
        render.check_entity_query_tensors(rays, np.zeros((1, 8), np.float32), None, hits, 0)
    with pytest.raises(ValueError, match="torch tensor"):
        render.check_entity_query_tensors(rays, None, None, None, 0)                                  # entity_hits is not optional


def _build(exe):
    """With the sanitizers (their runtimes linked into the program where the compiler has the archives); without them where it has
    no runtime at all: the comparison with the model runs either way."""
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []):
        r = subprocess.run(BASE + extra + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            return extra, r
    raise AssertionError("entity_query_main.cpp does not compile:\n" + r.stderr[-4000:])


def test_the_host_checks_match_their_model_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "entity_query_main")
    flags, _ = _build(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "flags %s\n%s\n%s" % (" ".join(flags), r.stdout[-2000:], r.stderr[-6000:])
    assert "all cases match the model" in r.stdout
