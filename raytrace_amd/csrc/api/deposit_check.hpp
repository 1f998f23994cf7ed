// deposit_check.hpp — the host half of rt_deposit_particles that needs no context: the verdict on the call's plain arguments and on
// its RtParticleDeposit parameters, the clipped box with its texel count, the list of the chunks it meets, the pointer overlap test and
// the size of the device scratch.  Plain C++ with no HIP include, so that tests/deposit_particles_main.cpp runs this very code on the
// CPU.  The box's validity and clipping are rt_edit_shapes' (edit_shapes.hpp) and the window's bound is rt_emit_particles'
// (emit_check.hpp): nothing of them is restated here.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../../include/rt_abi.h"
#include "edit_shapes.hpp"
#include "emit_check.hpp"

namespace rta __attribute__((visibility("hidden"))) {

constexpr uint32_t kMaxDepositParticles = 1u << 20;   // records per call
constexpr uint64_t kMaxDepositBoxTexels = 1ull << 24; // texels of the clipped box: 64 MiB of claims

// The deposit box as rt_edit_shapes reads a box shape (where, solid, material and reserved 0).
inline RtShapeEdit deposit_shape(const RtParticleDeposit& p) {
    RtShapeEdit s{};
    for (int k = 0; k < 3; k++) { s.a[k] = p.lo[k]; s.b[k] = p.hi[k]; }
    s.kind = RT_SHAPE_BOX;
    return s;
}

// Two byte ranges share a byte (an empty or null range shares none).
inline bool deposit_ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    if (!a || !b || a_bytes == 0u || b_bytes == 0u) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}

// What is wrong with the arguments that are tested before the context is looked at, or nullptr.
inline const char* deposit_args_error(const void* params, const void* states, const void* draw, uint32_t count, const void* counts) {
    if (!params) return "null params";
    if (count > kMaxDepositParticles) return "more than 2^20 particles in one call";
    if (count == 0u) return nullptr;
    if (!states) return "null states";
    const size_t sb = (size_t)count * sizeof(RtParticleState), db = (size_t)count * sizeof(RtParticle);
    if (deposit_ranges_overlap(states, sb, draw, db) || deposit_ranges_overlap(states, sb, counts, sizeof(RtDepositCount)) ||
        deposit_ranges_overlap(draw, db, counts, sizeof(RtDepositCount)))
        return "states, draw and counts must not overlap";
    return nullptr;
}

// What is wrong with the parameters for a region of edge 2^logr, or nullptr.  Every comparison is false for a NaN.
inline const char* deposit_params_error(const RtParticleDeposit& p, int logr) {
    if (!(p.max_speed >= 0.0f && std::isfinite(p.max_speed))) return "max_speed must be finite and not negative";
    if (p.reserved0 != 0u || p.reserved1 != 0u) return "a reserved word is not 0";
    if (!shape_valid(deposit_shape(p), (int32_t)1 << logr)) return "the box must have lo <= hi and coordinates within [-4R, 4R]";
    if (!emit_window_valid(p.lr, logr)) return "|lr| must not exceed 2^22 - R";
    return nullptr;
}

// The clipped box of valid parameters, the chunks it meets and what the call needs on the device.
struct DepositPlan {
    bool empty = true;      // the box misses [0, R)^3: the call enqueues nothing
    EditBox box{};          // the clipped box, texels, inclusive
    uint64_t texels = 0;    // of the clipped box (the caller refuses more than kMaxDepositBoxTexels)
    uint32_t nc[3] = {0, 0, 0}, nchunks = 0;   // chunks per axis, and in all
    size_t need = 0;        // bytes of the staging block: the chunk ids
};

inline DepositPlan deposit_plan(const RtParticleDeposit& p, int logr) {
    DepositPlan d;
    if (!shape_bounding_box(deposit_shape(p), logr, &d.box)) return d;
    d.empty = false;
    d.texels = 1;
    d.nchunks = 1;
    for (int k = 0; k < 3; k++) {
        d.texels *= (uint64_t)(d.box.hi[k] - d.box.lo[k] + 1);
        d.nc[k] = (uint32_t)(d.box.hi[k] >> 6) - (uint32_t)(d.box.lo[k] >> 6) + 1u;
        d.nchunks *= d.nc[k];
    }
    d.need = align16((size_t)d.nchunks * 4u);
    return d;
}

// The ids of the plan's chunks, ascending — z-major over the box's chunks, which is the order of the device's flag words.
// h_chunks holds at least nchunks words; returns how many were written.
inline uint32_t deposit_fill_chunks(const DepositPlan& d, int logr, uint32_t* h_chunks) {
    const int nl = logr - 6;
    uint32_t t = 0;
    for (uint32_t cz = 0; cz < d.nc[2]; cz++)
        for (uint32_t cy = 0; cy < d.nc[1]; cy++)
            for (uint32_t cx = 0; cx < d.nc[0]; cx++)
                h_chunks[t++] = ((((uint32_t)(d.box.lo[2] >> 6) + cz) << nl | ((uint32_t)(d.box.lo[1] >> 6) + cy)) << nl) | ((uint32_t)(d.box.lo[0] >> 6) + cx);
    return t;
}

// Words of the device scratch: a claim per texel, a flag per chunk, a spare RtDepositCount (rtd::deposit_scratch_words).
inline size_t deposit_scratch_need(const DepositPlan& d) { return (size_t)d.texels + d.nchunks + 4u; }

}  // namespace rta
