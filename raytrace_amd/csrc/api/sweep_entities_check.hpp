// sweep_entities_check.hpp — the host half of rt_sweep_entities / rt_sweep_entities_async that needs no context: the verdict on the
// calls' plain arguments — the counts and the NULL pointers against them — the validated domain of a sweep in the kernel's own fp32
// operations and, through shadows_check.hpp's one host definition, the validity of the boxes.  Plain C++ with no HIP include, so that
// tests/sweep_entities_main.cpp runs this very code on the CPU.  (The models' records are draw_stamps.hpp's, unchanged: the calls
// resolve and validate them with draw_stamps_validate.)
#pragma once

#include <cmath>
#include <cstdint>

#include "../../../include/rt_abi.h"
#include "draw_stamps.hpp"
#include "shadows_check.hpp"

namespace rta __attribute__((visibility("hidden"))) {

constexpr uint32_t kMaxEntitySweeps = 1u << 24;                            // sweeps per call
static_assert(kMaxEntityModels <= kMaxDrawStamps, "the models travel as one rt_draw_stamps batch");
static_assert(sizeof(RtEntitySweepHit) == 80 && sizeof(RtBoxSweep) == 48 && sizeof(RtSweepHit) == 64,
              "the kernel reads three 16-byte words per sweep and writes four and five per hit");

// What is wrong with the counts and pointers of a call, or nullptr.  sweeps, lr and entity_hits are needed only when count > 0, an
// entity array only when its count is (entity_arrays_error); world_hits may always be NULL.  The order is the one the calls report
// in: every count comes before any pointer.
inline const char* sweep_entities_args_error(uint32_t count, const void* sweeps, const void* lr, const void* entity_hits, const void* boxes,
                                             uint32_t nboxes, const void* models, uint32_t nmodels) {
    if (count > kMaxEntitySweeps) return "more than 2^24 sweeps in one call";
    if (const char* e = entity_arrays_error(boxes, nboxes, models, nmodels)) return e;
    if (count > 0u && (!sweeps || !lr || !entity_hits)) return "null pointer";
    return nullptr;
}

// The validated domain of one record, rt_sweep_boxes' and rt_sweep_entities' alike, in the kernel's own fp32 operations (a NaN fails
// every comparison).  The reserved words play no part: rt_sweep_entities' reserved0 and reserved1 name the entity a sweep ignores,
// and every value is allowed there.
inline bool sweep_in_domain(const RtBoxSweep& s) {
    for (int k = 0; k < 3; k++) {
        const float e = s.hi[k] - s.lo[k];
        if (!(std::fabs(s.lo[k]) <= 4194304.0f && std::fabs(s.hi[k]) <= 4194304.0f && std::fabs(s.motion[k]) <= 64.0f && e > 0.0f && e <= 8.0f))
            return false;
    }
    return true;
}

// The index of the first sweep outside the domain, or `count`.
inline uint32_t first_invalid_sweep(const RtBoxSweep* sweeps, uint32_t count) {
    for (uint32_t i = 0; i < count; i++)
        if (!sweep_in_domain(sweeps[i])) return i;
    return count;
}

}  // namespace rta
