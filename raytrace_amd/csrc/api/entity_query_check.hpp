// entity_query_check.hpp — the host half of rt_trace_entities / rt_trace_entities_async / rt_pick_entities that needs no context: the
// verdict on the calls' plain arguments — the counts, the NULL pointers against them, the pixels against the frame — and, through
// shadows_check.hpp's one host definition, the validity of the boxes.  Plain C++ with no HIP include, so that
// tests/entity_query_main.cpp runs this very code on the CPU.  (The models' records are draw_stamps.hpp's, unchanged.)
#pragma once

#include <cstdint>

#include "../../../include/rt_abi.h"
#include "shadows_check.hpp"

namespace rta __attribute__((visibility("hidden"))) {

constexpr uint32_t kMaxEntityRays = 1u << 24;                               // rays or pixels per call

// What is wrong with the counts and pointers of a call, or nullptr.  `in` is rays or xy, `more` is lr or u; they and `entity_hits`
// are needed only when count > 0, an entity array only when its count is (entity_arrays_error).  The order is the one the calls
// report in: every count comes before any pointer.
inline const char* entity_query_args_error(uint32_t count, const void* in, const void* more, const void* entity_hits, const void* boxes,
                                           uint32_t nboxes, const void* models, uint32_t nmodels) {
    if (count > kMaxEntityRays) return "more than 2^24 rays in one call";
    if (const char* e = entity_arrays_error(boxes, nboxes, models, nmodels)) return e;
    if (count > 0u && (!in || !more || !entity_hits)) return "null pointer";
    return nullptr;
}

// The index of the first pixel of xy[2 i], xy[2 i + 1] outside width x height, or `count`.
inline uint32_t first_pixel_outside(const int32_t* xy, uint32_t count, int32_t width, int32_t height) {
    for (uint32_t i = 0; i < count; i++)
        if (xy[2u * i] < 0 || xy[2u * i] >= width || xy[2u * i + 1u] < 0 || xy[2u * i + 1u] >= height) return i;
    return count;
}

}  // namespace rta
