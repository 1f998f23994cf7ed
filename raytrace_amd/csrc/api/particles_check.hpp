// particles_check.hpp — the host half of rt_draw_particles that needs no context: the test of the call's plain arguments and the
// validity of a batch of RtParticle records.  Plain C++ with no HIP include, so that tests/draw_particles_main.cpp runs this very
// code on the CPU.  The comparisons are the kernel's (rt_particles.hip, particle_valid): each is false for a NaN, so a record with a
// NaN fails; the derived corners are one fp32 subtraction and one addition, as on the device.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../../include/rt_abi.h"

namespace rta __attribute__((visibility("hidden"))) {

constexpr uint32_t kMaxDrawParticles = 1u << 20, kMaxParticleLights = 1u << 20;   // records per call, of either kind

// What is wrong with the arguments that are tested before the context is looked at, or nullptr.
inline const char* particle_args_error(const void* u, const void* particles, uint32_t count, const void* lights, uint32_t nlights) {
    if (!u) return "null uniforms";
    if (count > kMaxDrawParticles) return "more than 2^20 particles in one call";
    if (nlights > kMaxParticleLights) return "more than 2^20 lights in one call";
    if (count > 0u && (!particles || !lights)) return "null pointer";
    if (count > 0u && nlights == 0u) return "particles need at least one light";
    return nullptr;
}

// One particle: every float finite, half > 0, the derived box lo_k = center_k - half, hi_k = center_k + half a valid RtDrawBox
// (|lo_k|, |hi_k| <= 2^22 and lo_k < hi_k after the rounding), light < nlights, reserved == 0.  material and emission play no part.
inline bool particle_valid(const RtParticle& p, uint32_t nlights) {
    if (!(p.half > 0.0f) || p.light >= nlights || p.reserved != 0u) return false;
    for (int k = 0; k < 3; k++) {
        const float lo = p.center[k] - p.half, hi = p.center[k] + p.half;
        if (!(std::fabs(lo) <= 4194304.0f && std::fabs(hi) <= 4194304.0f && lo < hi)) return false;
    }
    return true;
}

// The index of the first invalid particle of a batch, or `count` when every one is valid.
inline uint32_t first_invalid_particle(const RtParticle* particles, uint32_t count, uint32_t nlights) {
    for (uint32_t i = 0; i < count; i++)
        if (!particle_valid(particles[i], nlights)) return i;
    return count;
}

}  // namespace rta
