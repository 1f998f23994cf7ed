// particle_step_check.hpp — the host half of rt_step_particles that needs no context: the test of the call's plain arguments, of its
// RtParticleStep parameters and the validity of a batch of RtParticleState records.  Plain C++ with no HIP include, so that
// tests/particle_step_main.cpp runs this very code on the CPU.  The comparisons are the kernel's (rt_step_particles.hip): each is
// false for a NaN, so a record with a NaN fails; the box's extent is one fp32 subtraction, as on the device.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../../include/rt_abi.h"

namespace rta __attribute__((visibility("hidden"))) {

constexpr uint32_t kMaxStepParticles = 1u << 20;   // records per call

// What is wrong with the arguments that are tested before the context is looked at, or nullptr.  `out` may be `in`; any other
// overlap of the three ranges is refused.
inline const char* particle_step_args_error(const void* params, const void* in, const void* out, const void* draw, uint32_t count) {
    if (count > kMaxStepParticles) return "more than 2^20 particles in one call";
    if (count == 0u) return nullptr;
    if (!params || !in || !out) return "null pointer";
    const uintptr_t i = (uintptr_t)in, o = (uintptr_t)out, d = (uintptr_t)draw;
    const uintptr_t state_bytes = (uintptr_t)count * sizeof(RtParticleState), draw_bytes = (uintptr_t)count * sizeof(RtParticle);
    if (i != o && i < o + state_bytes && o < i + state_bytes) return "in and out overlap without being equal";
    if (draw && ((d < i + state_bytes && i < d + draw_bytes) || (d < o + state_bytes && o < d + draw_bytes))) return "draw overlaps in or out";
    return nullptr;
}

// What is wrong with the parameters, or nullptr: every float finite, 0 < dt <= 1, |accel_k| <= 4096, damping, restitution and friction in
// [0, 1], rest_speed >= 0, sweeps 1..4.
inline const char* particle_step_params_error(const RtParticleStep& p) {
    if (!(p.dt > 0.0f && p.dt <= 1.0f)) return "dt must be in (0, 1]";
    for (int k = 0; k < 3; k++)
        if (!(std::fabs(p.accel[k]) <= 4096.0f)) return "accel must lie within +-4096";
    if (!(p.damping >= 0.0f && p.damping <= 1.0f)) return "damping must be in [0, 1]";
    if (!(p.restitution >= 0.0f && p.restitution <= 1.0f)) return "restitution must be in [0, 1]";
    if (!(p.friction >= 0.0f && p.friction <= 1.0f)) return "friction must be in [0, 1]";
    if (!(p.rest_speed >= 0.0f && std::isfinite(p.rest_speed))) return "rest_speed must be finite and not negative";
    if (p.sweeps < 1u || p.sweeps > 4u) return "sweeps must be 1..4";
    return nullptr;
}

inline bool particle_state_inactive(const RtParticleState& s) { return (s.flags & (RT_PSTATE_DEAD | RT_PSTATE_INVALID)) != 0u; }

// One active record: every float finite except that life may be +inf, half > 0, reserved == 0, no flag bit outside RESPONSE | DEAD |
// CONTACT, the box inside rt_sweep_boxes' validated domain.  (An inactive record is copied through and is not judged.)
inline bool particle_state_valid(const RtParticleState& s) {
    if (!(s.half > 0.0f) || !std::isfinite(s.half) || s.reserved != 0u) return false;
    if ((s.flags & ~(RT_PSTATE_RESPONSE | RT_PSTATE_DEAD | RT_PSTATE_CONTACT)) != 0u) return false;
    if (!(s.life > -INFINITY)) return false;
    for (int k = 0; k < 3; k++) {
        const float e = s.hi[k] - s.lo[k];
        if (!(std::fabs(s.lo[k]) <= 4194304.0f && std::fabs(s.hi[k]) <= 4194304.0f && e > 0.0f && e <= 8.0f)) return false;
        if (!std::isfinite(s.velocity[k])) return false;
    }
    return true;
}

// The index of the first active record of a batch that is invalid, or `count` when there is none.
inline uint32_t first_invalid_particle_state(const RtParticleState* states, uint32_t count) {
    for (uint32_t i = 0; i < count; i++)
        if (!particle_state_inactive(states[i]) && !particle_state_valid(states[i])) return i;
    return count;
}

}  // namespace rta
