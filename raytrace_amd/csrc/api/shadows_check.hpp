// shadows_check.hpp — the host half of rt_shadow_entities that needs no context: the test of the call's plain arguments (with the
// one verdict on the two arrays of an entity set, entity_arrays_error, which the occluded lights, entity queries and sweeps share), the
// validity of a batch of RtDrawBox records (rt_draw_boxes' boxes and this call's occluders: the one host definition) and whether a
// frame has a sun term at all.  Plain C++ with no HIP include, so that tests/entity_shadows_main.cpp runs this very code on the CPU.
// The comparisons are the kernels' (rt_tile_pass.hpp, box_valid): each is false for a NaN, so a record with a NaN fails.  (The
// models' records are draw_stamps.hpp's, unchanged.)
#pragma once

#include <cmath>
#include <cstdint>

#include "../../../include/rt_abi.h"

namespace rta __attribute__((visibility("hidden"))) {

constexpr uint32_t kMaxEntityBoxes = 4096, kMaxEntityModels = 4096;   // an entity set (shadows, occluded lights, queries, sweeps): per call, of either kind

// What is wrong with the two arrays of an entity set, or nullptr: a count above 4096, a NULL array with its count above 0.
inline const char* entity_arrays_error(const void* boxes, uint32_t nboxes, const void* models, uint32_t nmodels) {
    if (nboxes > kMaxEntityBoxes) return "more than 4096 boxes in one call";
    if (nmodels > kMaxEntityModels) return "more than 4096 models in one call";
    if ((nboxes > 0u && !boxes) || (nmodels > 0u && !models)) return "null pointer";
    return nullptr;
}

// What is wrong with the arguments that are tested before the context is looked at, or nullptr: NULL uniforms, the arrays'
// verdict, a strength that is not finite or lies outside (0, 1].
inline const char* shadow_args_error(const void* u, const void* boxes, uint32_t nboxes, const void* models, uint32_t nmodels, float strength) {
    if (!u) return "null uniforms";
    if (const char* e = entity_arrays_error(boxes, nboxes, models, nmodels)) return e;
    if (!(strength > 0.0f && strength <= 1.0f)) return "strength must lie in (0, 1]";   // (false for a NaN)
    return nullptr;
}

// The valid RtDrawBox of rt_draw_boxes and rt_shadow_entities: every float finite, |lo_k|, |hi_k| <= 2^22 and lo_k < hi_k.  material
// and emission play no part.
inline bool draw_box_valid(const RtDrawBox& b) {
    for (int k = 0; k < 3; k++)
        if (!(std::fabs(b.lo[k]) <= 4194304.0f && std::fabs(b.hi[k]) <= 4194304.0f && b.lo[k] < b.hi[k])) return false;
    return true;
}

// The index of the first invalid box of a batch, or `count` when every one is valid.
inline uint32_t first_invalid_draw_box(const RtDrawBox* boxes, uint32_t count) {
    for (uint32_t i = 0; i < count; i++)
        if (!draw_box_valid(boxes[i])) return i;
    return count;
}

// A frame whose sun colour is (0, 0, 0) — the night — has no sun term to remove: the call enqueues nothing.  (-0 counts as 0; a NaN
// does not.)
inline bool shadow_sun_is_dark(const float sunlight[3]) { return sunlight[0] == 0.0f && sunlight[1] == 0.0f && sunlight[2] == 0.0f; }

}  // namespace rta
