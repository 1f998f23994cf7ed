"""rt_draw_particles / rt_draw_particles_async without a GPU: the record's layout in ctypes, numpy and the header, the header's
declarations, rule phrases and history line, the exported symbols, a null context, and what make_particles and
particle_tensor_counts refuse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytrace_amd import _lib, abi, render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rt_abi.h")).read()


def test_struct_is_32_bytes_with_the_headers_offsets():
    assert C.sizeof(abi.RtParticle) == 32
    assert [(n, getattr(abi.RtParticle, n).offset) for n, _ in abi.RtParticle._fields_] == [
        ("center", 0), ("half", 12), ("material", 16), ("emission", 20), ("light", 24), ("reserved", 28)]
    assert abi.MAX_PARTICLES == 1 << 20 and abi.MAX_PARTICLE_LIGHTS == 1 << 20


def test_dtype_matches_the_struct():
    dt = abi.PARTICLE_DTYPE
    assert dt.itemsize == C.sizeof(abi.RtParticle) == 32
    for name, _ in abi.RtParticle._fields_:
        assert dt.fields[name][1] == getattr(abi.RtParticle, name).offset
    rec = np.zeros(1, dtype=dt)
    rec["center"], rec["half"], rec["material"], rec["emission"], rec["light"], rec["reserved"] = (1, 2, 3), 0.5, 0xABCDE, 0xFF102030, 9, 4
    c = abi.RtParticle.from_buffer_copy(rec.tobytes())
    assert (list(c.center), c.half, c.material, c.emission, c.light, c.reserved) == ([1, 2, 3], 0.5, 0xABCDE, 0xFF102030, 9, 4)


def test_header_declares_the_record_the_calls_and_the_history_line():
    flat = re.sub(r"\s+", " ", HEADER)
    assert "typedef struct RtParticle { /* 32 bytes */ float center[3]; float half;" in flat
    assert "uint32_t material; uint32_t emission;" in flat and "uint32_t light; uint32_t reserved;" in flat
    assert ("int rt_draw_particles(RtContext* ctx, const RtUniforms* u, const RtParticle* particles, uint32_t count, const RtProbeLight* lights, "
            "uint32_t nlights);") in flat
    assert ("int rt_draw_particles_async(RtContext* ctx, const RtUniforms* u, const RtParticle* particles_dev, uint32_t count, "
            "const RtProbeLight* lights_dev, uint32_t nlights);") in flat
    assert "Additive, same minor version: RtParticle, rt_draw_particles, rt_draw_particles_async (" in flat
    assert "#define RT_ABI_VERSION_MINOR 3" in HEADER
    for phrase in ("lo_k = center_k - half, hi_k = center_k + half", "the smallest t_in, the lowest index","light < nlights, reserved == 0",
                   "count <= 2^20 and 1 <= nlights <= 2^20", "tests/draw_particles_ref.py", "8 + 8 lists + 72 count bytes"):
        assert phrase in flat, phrase


def test_symbols_are_listed_and_exported():
    assert "rt_draw_particles" in _lib.ABI_SYMBOLS and "rt_draw_particles_async" in _lib.ABI_SYMBOLS
    lib = _lib.amd()
    assert hasattr(lib, "rt_draw_particles") and hasattr(lib, "rt_draw_particles_async")


def test_null_context_is_invalid_arg_for_both_calls():
    lib = _lib.amd()
    u = abi.RtUniforms()
    p = render.make_particles([(0, 0, 0)], 0.5, 7)
    lights = np.zeros(1, dtype=render.PROBE_LIGHT_DTYPE)
    pp, pl = p.ctypes.data_as(C.c_void_p), lights.ctypes.data_as(C.c_void_p)
    assert lib.rt_draw_particles(None, C.byref(u), pp, 1, pl, 1) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_draw_particles_async(None, C.byref(u), pp, 1, pl, 1) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_draw_particles(None, None, None, 0, None, 0) == abi.RT_ERR_INVALID_ARG


def test_make_particles_builds_records():
    p = render.make_particles([(0, 1, 2), (-5, -5, -5)], [0.5, 0.25], [3, 4], [1, 0])
    assert p.dtype == abi.PARTICLE_DTYPE and p.size == 2
    assert p["center"].tolist() == [[0, 1, 2], [-5, -5, -5]] and p["half"].tolist() == [0.5, 0.25]
    assert p["material"].tolist() == [3, 4] and p["light"].tolist() == [1, 0] and p["emission"].tolist() == [0xFF000000] * 2
    assert not p["reserved"].any()
    assert render.make_particles(np.zeros((0, 3)), 1.0, 0).size == 0
    assert render.make_particles(np.zeros((3, 3)), 1.0, 5, emissions=7)["emission"].tolist() == [7, 7, 7]
    with pytest.raises(ValueError):
        render.make_particles(np.zeros(((1 << 20) + 1, 3)), 1.0, 0)


def test_particle_tensor_counts_refuses_what_the_kernel_could_not_read():
    import torch
    particles = torch.zeros((2, 8), dtype=torch.float32)
    lights = torch.zeros((3, 4), dtype=torch.float32)
    with pytest.raises(ValueError, match="cuda"):
        render.particle_tensor_counts(particles, lights, 0)                # host tensors
    with pytest.raises(ValueError, match="particles must be a torch tensor"):
        render.particle_tensor_counts(np.zeros((2, 8), np.float32), lights, 0)
    with pytest.raises(ValueError, match="lights must be a torch tensor"):
        render.particle_tensor_counts(particles, None, 0)
    assert render.record_count("particles", 64, 32, abi.MAX_PARTICLES, "RtParticle") == 2
    with pytest.raises(ValueError, match="whole 32-byte RtParticle records"):
        render.record_count("particles", 65, 32, abi.MAX_PARTICLES, "RtParticle")
    with pytest.raises(ValueError, match="at most"):
        render.record_count("particles", 32 * ((1 << 20) + 1), 32, abi.MAX_PARTICLES, "RtParticle")
