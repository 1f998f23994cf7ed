// rt_step_particles.hip — gfx950 kernel of rt_step_particles / rt_step_particles_async: one simulation tick of up to 2^20 particles
// against the resident region (include/rt_abi.h "Particle simulation"; the rules are restated in tests/particle_step_ref.py).
//
//   k_step_particles : one lane per particle.  The state record is four 16-byte loads and four 16-byte stores, the draw record two
//             more stores.  A lane reads its whole record before it writes anything and touches no other lane's, which is what lets
//             `out` be `in`.  Between them: validity, the velocity integration, up to four sub-sweeps through sweep_box
//             (rt_sweep_box.hpp: the one definition of rt_sweep_boxes' rules) with the contact response after each, and ageing.
//             The sub-sweep loop is not unrolled (one copy of sweep_box in the code) and its bound is the call's uniform `sweeps`;
//             a lane that has stopped — FREE, dead, stuck, no motion left — idles through the remaining rounds under EXEC.  The
//             blocked axis is a run-time value: every use of it is a chain of selects over k = 0..2, so velocity and motion stay in
//             registers and nothing goes to scratch.
//
// All float arithmetic is fp32 with one rounding per operation (-ffp-contract=off).  As in k_sweep, minefield values are not used
// to skip fetches.
#include <hip/hip_runtime.h>

#include "rt_kernels.hpp"
#include "rt_sweep_box.hpp"

namespace rtd {

namespace {

constexpr uint32_t kStepWg = 256;
constexpr uint32_t kInactive = RT_PSTATE_DEAD | RT_PSTATE_INVALID;
constexpr uint32_t kKnownFlags = RT_PSTATE_RESPONSE | RT_PSTATE_DEAD | RT_PSTATE_CONTACT;

__device__ __forceinline__ bool finite_f(float x) { return __builtin_fabsf(x) < __builtin_inff(); }   // false for a NaN

template <int LOGR>
__global__ __launch_bounds__(kStepWg) void k_step_particles(Scene sc, StepParticlesArgs a) {
    const uint32_t i = blockIdx.x * kStepWg + threadIdx.x;
    if (i >= a.count) return;
    const uint4* in = a.in + 4u * (size_t)i;
    const uint4 r0 = in[0], r1 = in[1], r2 = in[2], r3 = in[3];   // the whole record, before any store
    float lo[3] = {__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z)};
    float hi[3] = {__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z)};
    float v[3] = {__uint_as_float(r2.x), __uint_as_float(r2.y), __uint_as_float(r2.z)};
    float life = __uint_as_float(r0.w);
    const float half = __uint_as_float(r3.z);
    uint32_t flags = r1.w;

    // live: active on input and valid — the records the tick computes; every other one is copied through
    bool live = (flags & kInactive) == 0u;
    if (live) {
        bool ok = half > 0.0f && finite_f(half) && r3.w == 0u && (flags & ~kKnownFlags) == 0u && life > -__builtin_inff() &&
                  sweep_box_in_domain(lo, hi);
#pragma unroll
        for (int k = 0; k < 3; k++) ok = ok && finite_f(v[k]);
        if (!ok) { flags |= RT_PSTATE_INVALID; live = false; }
    }

    float m[3] = {0.0f, 0.0f, 0.0f};
    if (live) {
        flags &= ~RT_PSTATE_CONTACT;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            v[k] = (v[k] + a.accel[k] * a.dt) * a.damping;
            float d = v[k] * a.dt;
            d = d < -kSweepMaxMotion ? -kSweepMaxMotion : d;
            m[k] = d > kSweepMaxMotion ? kSweepMaxMotion : d;
        }
    }
    const uint32_t response = flags & RT_PSTATE_RESPONSE;
    bool run = live;
#pragma unroll 1
    for (uint32_t s = 0; s < a.sweeps; s++) {
        run = run && (m[0] != 0.0f || m[1] != 0.0f || m[2] != 0.0f);
        if (!run) continue;
        SweepResult h;
        sweep_box<LOGR>(sc.mine, a.lr, lo, hi, m, h);
        if (h.kind == RT_SWEEP_INVALID) { flags |= RT_PSTATE_INVALID; run = false; continue; }
        if (h.kind == RT_SWEEP_EMBEDDED) { flags |= RT_PSTATE_DEAD; run = false; continue; }
#pragma unroll
        for (int k = 0; k < 3; k++) { lo[k] = h.lo[k]; hi[k] = h.hi[k]; }
        if (h.kind == RT_SWEEP_FREE) { run = false; continue; }
        flags |= 0x10000u << h.axis;
        if (response == RT_PARTICLE_DIE) { flags |= RT_PSTATE_DEAD; run = false; continue; }
        if (response == RT_PARTICLE_STICK) {
            v[0] = v[1] = v[2] = 0.0f;
            run = false;
            continue;
        }
        const float rest = 1.0f - h.t;
        if (response == RT_PARTICLE_SLIDE) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const bool blocked = h.axis == (uint32_t)k;
                m[k] = blocked ? 0.0f : m[k] * rest;
                v[k] = blocked ? 0.0f : v[k];
            }
        } else {   // RT_PARTICLE_BOUNCE
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float mr = m[k] * rest;
                if (h.axis == (uint32_t)k) {
                    float w = -(v[k] * a.restitution);
                    if (__builtin_fabsf(w) < a.rest_speed) w = 0.0f;
                    v[k] = w;
                    m[k] = w != 0.0f ? -(mr * a.restitution) : 0.0f;
                } else {
                    v[k] = v[k] * a.friction;
                    m[k] = mr * a.friction;
                }
            }
        }
    }
    if (live) {
        life = life - a.dt;
        if (!(life > 0.0f)) flags |= RT_PSTATE_DEAD;
    }

    uint4* out = a.out + 4u * (size_t)i;
    if (live) {
        out[0] = make_uint4(__float_as_uint(lo[0]), __float_as_uint(lo[1]), __float_as_uint(lo[2]), __float_as_uint(life));
        out[1] = make_uint4(__float_as_uint(hi[0]), __float_as_uint(hi[1]), __float_as_uint(hi[2]), flags);
        out[2] = make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), r2.w);
        out[3] = r3;
    } else {   // the input bits, with INVALID set where the device found the record outside the domain
        out[0] = r0;
        out[1] = make_uint4(r1.x, r1.y, r1.z, flags);
        out[2] = r2;
        out[3] = r3;
    }
    if (a.draw) {
        uint4* draw = a.draw + 2u * (size_t)i;
        const float c0 = (lo[0] + hi[0]) * 0.5f, c1 = (lo[1] + hi[1]) * 0.5f, c2 = (lo[2] + hi[2]) * 0.5f;
        draw[0] = make_uint4(__float_as_uint(c0), __float_as_uint(c1), __float_as_uint(c2), (flags & kInactive) ? 0u : r3.z);
        draw[1] = make_uint4(r3.x, r3.y, r2.w, 0u);
    }
}

}  // namespace

hipError_t launch_step_particles(const Scene& sc, int logr, const StepParticlesArgs& a, hipStream_t st) {
    if (logr < 8 || logr > 10 || a.sweeps < 1u || a.sweeps > 4u || a.count > kMaxParticles) return hipErrorInvalidValue;
    if (a.count == 0u) return hipSuccess;
    const dim3 grid((a.count + kStepWg - 1u) / kStepWg), block(kStepWg);
    if (logr == 8) hipLaunchKernelGGL((k_step_particles<8>), grid, block, 0, st, sc, a);
    else if (logr == 9) hipLaunchKernelGGL((k_step_particles<9>), grid, block, 0, st, sc, a);
    else hipLaunchKernelGGL((k_step_particles<10>), grid, block, 0, st, sc, a);
    return hipGetLastError();
}

}  // namespace rtd
