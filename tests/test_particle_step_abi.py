"""rt_step_particles / rt_step_particles_async without a GPU: the records' layouts in ctypes, numpy and the header, the header's
declarations, rule phrases and history line, the exported symbols, a null context, and what make_particle_states and
particle_step_tensor_count refuse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytrace_amd import _lib, abi, render
from tests import particle_step_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
STATE_OFFSETS = [("lo", 0), ("life", 12), ("hi", 16), ("flags", 28), ("velocity", 32), ("light", 44), ("material", 48), ("emission", 52),
                 ("half", 56), ("reserved", 60)]
STEP_OFFSETS = [("dt", 0), ("accel", 4), ("damping", 16), ("restitution", 20), ("friction", 24), ("rest_speed", 28), ("lr", 32), ("sweeps", 44)]


def test_structs_have_the_headers_sizes_and_offsets():
    assert C.sizeof(abi.RtParticleState) == 64 and C.sizeof(abi.RtParticleStep) == 48
    assert [(n, getattr(abi.RtParticleState, n).offset) for n, _ in abi.RtParticleState._fields_] == STATE_OFFSETS
    assert [(n, getattr(abi.RtParticleStep, n).offset) for n, _ in abi.RtParticleStep._fields_] == STEP_OFFSETS
    # the header's own member order and comment offsets
    body = HEADER.split("typedef struct RtParticleState {")[1].split("} RtParticleState;")[0]
    members = re.findall(r"(?:float|uint32_t|int32_t)\s+(\w+)(?:\[3\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert members == [n for n, _ in STATE_OFFSETS]
    body = HEADER.split("typedef struct RtParticleStep {")[1].split("} RtParticleStep;")[0]
    members = re.findall(r"(?:float|uint32_t|int32_t)\s+(\w+)(?:\[3\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert members == [n for n, _ in STEP_OFFSETS]


def test_dtypes_match_the_structs_and_the_restatements_own():
    dt = abi.PARTICLE_STATE_DTYPE
    assert dt.itemsize == 64 and ref.STATE_DTYPE.itemsize == 64
    for name, off in STATE_OFFSETS:
        assert dt.fields[name][1] == off == ref.STATE_DTYPE.fields[name][1], name
    for name, _ in abi.RtParticle._fields_:
        assert abi.PARTICLE_DTYPE.fields[name][1] == ref.DRAW_DTYPE.fields[name][1], name
    assert not hasattr(render, "PARTICLE_STATE_DTYPE")            # the dtype lives in abi
    rec = np.zeros(1, dtype=dt)
    rec["lo"], rec["hi"], rec["velocity"], rec["life"], rec["flags"], rec["half"], rec["light"] = (1, 2, 3), (4, 5, 6), (7, 8, 9), 2.5, 0x103, 0.5, 9
    c = abi.RtParticleState.from_buffer_copy(rec.tobytes())
    assert (list(c.lo), list(c.hi), list(c.velocity), c.life, c.flags, c.half, c.light) == ([1, 2, 3], [4, 5, 6], [7, 8, 9], 2.5, 0x103, 0.5, 9)


def test_constants_agree_with_the_header_and_the_restatement():
    for name in ("RT_PARTICLE_DIE", "RT_PARTICLE_STICK", "RT_PARTICLE_SLIDE", "RT_PARTICLE_BOUNCE", "RT_PSTATE_RESPONSE", "RT_PSTATE_DEAD",
                 "RT_PSTATE_INVALID", "RT_PSTATE_CONTACT"):
        value = int(re.search(r"#define %s\s+(0x[0-9a-fA-F]+|\d+)u?\b" % name, HEADER).group(1), 0)
        assert getattr(abi, name) == value, name
    assert (ref.DIE, ref.STICK, ref.SLIDE, ref.BOUNCE) == (abi.RT_PARTICLE_DIE, abi.RT_PARTICLE_STICK, abi.RT_PARTICLE_SLIDE, abi.RT_PARTICLE_BOUNCE)
    assert (ref.RESPONSE, ref.DEAD, ref.INVALID, ref.CONTACT) == (abi.RT_PSTATE_RESPONSE, abi.RT_PSTATE_DEAD, abi.RT_PSTATE_INVALID, abi.RT_PSTATE_CONTACT)


def test_header_declares_the_calls_the_rules_and_the_history_line():
    flat = re.sub(r"\s+", " ", HEADER)
    assert ("int rt_step_particles(RtContext* ctx, const RtParticleStep* params, const RtParticleState* in, RtParticleState* out, "
            "RtParticle* draw, uint32_t count);") in flat
    assert ("int rt_step_particles_async(RtContext* ctx, const RtParticleStep* params, const RtParticleState* in_dev, "
            "RtParticleState* out_dev, RtParticle* draw_dev, uint32_t count);") in flat
    assert "Additive, same minor version: RtParticleState, RtParticleStep, RT_PARTICLE_*, RT_PSTATE_*, rt_step_particles, rt_step_particles_async * (particle simulation:" in flat
    assert "#define RT_ABI_VERSION_MINOR 3" in HEADER
    for phrase in ("v_k = (v_k + accel_k * dt) * damping", "m_k = min(max(v_k * dt, -64), 64)", "stop when every m_k == 0",
                   "w = -(v_a * restitution)", "life = life - dt; if !(life > 0), set DEAD", "center_k = (lo_k + hi_k) * 0.5",
                   "`out` may equal `in`", "a live particle is never EMBEDDED", "Out of scope: compaction of dead slots",
                   "tests/particle_step_ref.py", "0 < dt <= 1; |accel_k| <= 4096"):
        assert phrase in flat, phrase
    assert "rt_step_particles_async" in flat.split("typedef struct RtParticle {")[0].split("Particles: many small cubes")[1]


def test_symbols_are_listed_and_exported():
    assert "rt_step_particles" in _lib.ABI_SYMBOLS and "rt_step_particles_async" in _lib.ABI_SYMBOLS
    lib = _lib.amd()
    assert hasattr(lib, "rt_step_particles") and hasattr(lib, "rt_step_particles_async")


def test_null_context_is_invalid_arg_for_both_calls():
    lib = _lib.amd()
    p = render.make_particle_step(1.0 / 60.0)
    s = render.make_particle_states([(0, 0, 0)], [(0.25, 0.25, 0.25)])
    out, draw = np.zeros_like(s), np.zeros(1, dtype=abi.PARTICLE_DTYPE)
    ps, po, pd = (a.ctypes.data_as(C.c_void_p) for a in (s, out, draw))
    assert lib.rt_step_particles(None, C.byref(p), ps, po, pd, 1) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_step_particles_async(None, C.byref(p), ps, po, pd, 1) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_step_particles(None, None, None, None, None, 0) == abi.RT_ERR_INVALID_ARG
    assert not out.view(np.uint8).any() and not draw.view(np.uint8).any()


def test_make_particle_states_builds_records():
    s = render.make_particle_states([(0, 1, 2), (-5, -5, -5)], [(0.5, 1.5, 2.5), (-4.75, -4.75, -4.75)], [(1, 2, 3), (0, 0, -9)],
                                    responses=[abi.RT_PARTICLE_BOUNCE, abi.RT_PARTICLE_STICK], lives=[2.0, np.inf], materials=[3, 4], lights=[1, 0])
    assert s.dtype == abi.PARTICLE_STATE_DTYPE and s.size == 2
    assert s["lo"].tolist() == [[0, 1, 2], [-5, -5, -5]] and s["velocity"].tolist() == [[1, 2, 3], [0, 0, -9]]
    assert s["half"].tolist() == [0.25, 0.125] and s["flags"].tolist() == [3, 1] and s["life"].tolist() == [2.0, np.inf]
    assert s["material"].tolist() == [3, 4] and s["light"].tolist() == [1, 0] and s["emission"].tolist() == [0xFF000000] * 2
    assert not s["reserved"].any()
    assert render.make_particle_states(np.zeros((0, 3)), np.zeros((0, 3))).size == 0
    assert render.make_particle_states(np.zeros((3, 3)), np.ones((3, 3)), halves=0.0625)["half"].tolist() == [0.0625] * 3
    with pytest.raises(ValueError):
        render.make_particle_states(np.zeros((2, 3)), np.ones((3, 3)))
    with pytest.raises(ValueError):
        render.make_particle_states(np.zeros(((1 << 20) + 1, 3)), np.ones(((1 << 20) + 1, 3)))


def test_particle_step_tensor_count_refuses_what_the_kernel_could_not_use():
    import torch
    states = torch.zeros((2, 16), dtype=torch.float32)
    with pytest.raises(ValueError, match="cuda"):
        render.particle_step_tensor_count(states, states, None, 0)                 # host tensors
    with pytest.raises(ValueError, match="states_in must be a torch tensor"):
        render.particle_step_tensor_count(np.zeros((2, 16), np.float32), states, None, 0)
    with pytest.raises(ValueError, match="draw must be a torch tensor"):
        render.particle_step_tensor_count(states, states, np.zeros(16, np.float32), 0)
    assert render.record_count("states_in", 128, 64, abi.MAX_PARTICLES, "RtParticleState") == 2
    with pytest.raises(ValueError, match="whole 64-byte RtParticleState records"):
        render.record_count("states_in", 65, 64, abi.MAX_PARTICLES, "RtParticleState")
    with pytest.raises(ValueError, match="at most"):
        render.record_count("states_in", 64 * ((1 << 20) + 1), 64, abi.MAX_PARTICLES, "RtParticleState")
