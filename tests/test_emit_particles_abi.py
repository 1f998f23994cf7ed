"""rt_emit_particles / rt_emit_particles_async without a GPU: the records' layouts in ctypes, numpy and the header, the header's
declarations, rule phrases and history line, the exported symbols, a null context, and what make_particle_emitters and
emit_tensor_capacity refuse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytrace_amd import _lib, abi, render
from tests import emit_particles_ref as ref
from tests import emit_particles_sets as sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
EMIT_OFFSETS = [("a", 0), ("seed", 12), ("b", 16), ("kind", 28), ("response", 29), ("reserved0", 30), ("origin", 32), ("speed", 44), ("drift", 48),
                ("spread", 60), ("half", 64), ("life_min", 68), ("life_span", 72), ("density", 76), ("light", 80), ("emission", 84), ("reserved", 88)]
CURSOR_OFFSETS = [("next", 0), ("emitted", 4), ("dropped", 8), ("reserved", 12)]


def test_structs_have_the_headers_sizes_and_offsets():
    assert C.sizeof(abi.RtParticleEmit) == 96 and C.sizeof(abi.RtEmitCursor) == 16
    assert [(n, getattr(abi.RtParticleEmit, n).offset) for n, _ in abi.RtParticleEmit._fields_] == EMIT_OFFSETS
    assert [(n, getattr(abi.RtEmitCursor, n).offset) for n, _ in abi.RtEmitCursor._fields_] == CURSOR_OFFSETS
    # the header's own member order
    body = HEADER.split("typedef struct RtParticleEmit {")[1].split("} RtParticleEmit;")[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m for decl in re.findall(r"(?:float|uint32_t|int32_t|uint8_t)\s+([^;]+);", body) for m in re.findall(r"([a-z_0-9]+)(?:\[\d\])?", decl)]
    assert members == [n for n, _ in EMIT_OFFSETS]
    body = HEADER.split("typedef struct RtEmitCursor {")[1].split("} RtEmitCursor;")[0]
    assert re.findall(r"(\w+)[,;]", body.split("uint32_t")[1]) == [n for n, _ in CURSOR_OFFSETS]
    assert "/* 96 bytes */" in HEADER.split("typedef struct RtParticleEmit {")[1][:40]


def test_dtypes_match_the_structs_and_the_restatements_own():
    assert abi.EMIT_DTYPE.itemsize == 96 == ref.EMIT_DTYPE.itemsize and abi.EMIT_CURSOR_DTYPE.itemsize == 16 == ref.CURSOR_DTYPE.itemsize
    for name, off in EMIT_OFFSETS:
        assert abi.EMIT_DTYPE.fields[name][1] == off == ref.EMIT_DTYPE.fields[name][1], name
    for name, off in CURSOR_OFFSETS:
        assert abi.EMIT_CURSOR_DTYPE.fields[name][1] == off == ref.CURSOR_DTYPE.fields[name][1], name
    assert not hasattr(render, "EMIT_DTYPE")                      # the dtype lives in abi
    e = sets.cases()["sphere"]["emitters"]
    c = abi.RtParticleEmit.from_buffer_copy(e.tobytes())
    assert (list(c.a), list(c.b), c.kind, c.response, c.seed, c.density, c.half, c.light) == ([3, 129, 253], [49, 0, 0], 1, 3, 7, 256, 0.125, 3)


def test_header_declares_the_calls_the_rules_and_the_history_line():
    flat = re.sub(r"\s+", " ", HEADER)
    assert ("int rt_emit_particles(RtContext* ctx, const RtParticleEmit* emitters, uint32_t count, const int32_t lr[3], "
            "RtParticleState* states, uint32_t capacity, uint32_t max_emit, RtEmitCursor* cursor);") in flat
    assert ("int rt_emit_particles_async(RtContext* ctx, const RtParticleEmit* emitters, uint32_t count, const int32_t lr[3], "
            "RtParticleState* states_dev, uint32_t capacity, uint32_t max_emit, RtEmitCursor* cursor_dev);") in flat
    assert ("Additive, same minor version: RtParticleEmit, RtEmitCursor, rt_emit_particles, rt_emit_particles_async (particle emitters:"
            in flat)
    assert "#define RT_ABI_VERSION_MINOR 3" in HEADER
    for phrase in ("(h & 255) < density", "h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16",
                   "g_i = mix(h + i) for i = 1..4", "u_i = float(g_i >> 8) * 2^-24", "(z >> 2, * y >> 2, x >> 2, z & 3, y & 3, x & 3)",
                   "slot * (next + j) mod capacity", "emitted += n, dropped += N - n", "|lr_k| <= 2^22 - R", "c_k = float(v_k) + 0.5f",
                   "len = rtm_length3(r)", "dir_k = len > 0 ? r_k / len : 0", "life = life_min + u_4 * life_span", "2^-8 <= half <= 0.5",
                   "count <= 256; 1 <= max_emit <= capacity <= 2^20", "at most 2^18 bricks", "The debris recipe",
                   "tests/emit_particles_ref.py", "No atomic decides a slot"):
        assert phrase in flat, phrase
    # the old remarks still stand, and point to the new section
    assert "emitters (a host overwrites the oldest slots of a ring with hipMemcpyAsync)" in flat
    assert "rt_emit_particles" in flat.split("Out of scope: compaction of dead slots")[1].split("Device work per call")[0]


def test_symbols_are_listed_and_exported():
    assert "rt_emit_particles" in _lib.ABI_SYMBOLS and "rt_emit_particles_async" in _lib.ABI_SYMBOLS
    lib = _lib.amd()
    assert hasattr(lib, "rt_emit_particles") and hasattr(lib, "rt_emit_particles_async")
    assert (abi.MAX_EMITTERS, abi.MAX_EMIT_CAPACITY) == (ref.MAX_EMITTERS, ref.MAX_CAPACITY) == (256, 1 << 20)


def test_null_context_is_invalid_arg_for_both_calls():
    lib = _lib.amd()
    e = sets.cases()["sphere"]["emitters"].view(abi.EMIT_DTYPE)
    ring, cur = np.zeros(8, dtype=abi.PARTICLE_STATE_DTYPE), np.zeros(1, dtype=abi.EMIT_CURSOR_DTYPE)
    pe, pr, pc = (a.ctypes.data_as(C.c_void_p) for a in (e, ring, cur))
    lr = (C.c_int32 * 3)(0, 0, 0)
    assert lib.rt_emit_particles(None, pe, 1, lr, pr, 8, 8, pc) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_emit_particles_async(None, pe, 1, lr, pr, 8, 8, pc) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_emit_particles(None, None, 0, lr, None, 0, 0, None) == abi.RT_ERR_INVALID_ARG
    assert not ring.view(np.uint8).any() and not cur.view(np.uint8).any()


def test_make_particle_emitters_builds_records_and_refuses_what_the_calls_refuse():
    shapes = [render.box_shape((1, 2, 3), (4, 5, 6)), render.sphere_shape((10.5, 10.5, 10.5), 3.5)]
    e = render.make_particle_emitters(shapes, [(1.5, 2.5, 3.5), (0, 0, 0)], speeds=[6.0, 0.0], drifts=(0, 0, 2.0), spreads=1.5, halves=0.25,
                                      life_mins=[0.5, np.inf], life_spans=2.0, densities=[37, 256], responses=abi.RT_PARTICLE_BOUNCE, seeds=[7, 8],
                                      lights=3, emissions=0xFF102030)
    assert e.dtype == abi.EMIT_DTYPE and e.size == 2
    assert e["a"].tolist() == [[1, 2, 3], [21, 21, 21]] and e["b"].tolist() == [[4, 5, 6], [49, 0, 0]] and e["kind"].tolist() == [0, 1]
    assert e["origin"].tolist() == [[1.5, 2.5, 3.5], [0, 0, 0]] and e["speed"].tolist() == [6.0, 0.0] and e["drift"].tolist() == [[0, 0, 2.0]] * 2
    assert e["density"].tolist() == [37, 256] and e["response"].tolist() == [3, 3] and e["seed"].tolist() == [7, 8]
    assert e["life_min"].tolist() == [0.5, np.inf] and e["half"].tolist() == [0.25, 0.25] and e["light"].tolist() == [3, 3]
    assert not e["reserved"].any() and not e["reserved0"].any()
    assert all(ref.valid(r, 256) for r in e.view(ref.EMIT_DTYPE))
    one, at = [shapes[0]], [(0, 0, 0)]
    for bad in (dict(halves=0.6), dict(halves=0.001), dict(speeds=-1.0), dict(speeds=5000.0), dict(spreads=np.nan), dict(drifts=(0, 5000.0, 0)),
                dict(life_mins=0.0), dict(life_mins=np.nan), dict(life_spans=-1.0), dict(life_spans=np.inf), dict(densities=0), dict(densities=257),
                dict(responses=4)):
        with pytest.raises(ValueError):
            render.make_particle_emitters(one, at, **bad)
    with pytest.raises(ValueError):
        render.make_particle_emitters(one, [(2.0 ** 23, 0, 0)])
    with pytest.raises(ValueError, match="at most 256"):
        render.make_particle_emitters([shapes[0]] * 257, (0, 0, 0))
    cur = render.emit_cursor((5, 6, 7))
    assert cur.dtype == abi.EMIT_CURSOR_DTYPE and cur[0].tolist() == (5, 6, 7, 0)
    assert render.emit_cursor(cur[0])[0].tolist() == (5, 6, 7, 0) and render.emit_cursor(abi.RtEmitCursor(1, 2, 3, 0))[0].tolist() == (1, 2, 3, 0)


def test_emit_tensor_capacity_refuses_what_the_kernel_could_not_use():
    import torch
    states, cursor = torch.zeros((4, 16), dtype=torch.float32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="cuda"):
        render.emit_tensor_capacity(states, cursor, 0)                               # host tensors
    with pytest.raises(ValueError, match="states must be a torch tensor"):
        render.emit_tensor_capacity(np.zeros((4, 16), np.float32), cursor, 0)
    with pytest.raises(ValueError, match="cursor must be a torch tensor"):
        render.emit_tensor_capacity(states, np.zeros(4, np.uint32), 0)
    assert render.record_count("states", 256, 64, abi.MAX_EMIT_CAPACITY, "RtParticleState") == 4
    with pytest.raises(ValueError, match="at most"):
        render.record_count("states", 64 * ((1 << 20) + 1), 64, abi.MAX_EMIT_CAPACITY, "RtParticleState")
