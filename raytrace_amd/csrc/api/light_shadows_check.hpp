// light_shadows_check.hpp — the host half of rt_add_lights_occluded that needs no context: the test of the call's plain arguments,
// rt_add_lights' for the lights and rt_shadow_entities' for the two occluder arrays, in that order.  Plain C++ with no HIP include,
// so that tests/light_shadows_main.cpp runs this very code on the CPU.  The records' validity is lights_check.hpp's and
// shadows_check.hpp's, unchanged.
#pragma once

#include <cstdint>

#include "lights_check.hpp"
#include "shadows_check.hpp"

namespace rta __attribute__((visibility("hidden"))) {

// What is wrong with the arguments that are tested before the context is looked at, or nullptr: NULL uniforms, more than 1024 lights,
// a NULL `lights` with count > 0, an occluder count above 4096, a NULL occluder array with its count above 0.
inline const char* light_shadow_args_error(const void* u, const void* lights, uint32_t count, const void* boxes, uint32_t nboxes, const void* models,
                                           uint32_t nmodels) {
    if (!u) return "null uniforms";
    if (count > kMaxPointLights) return "more than 1024 lights in one call";
    if (count > 0u && !lights) return "null pointer";
    return shadow_args_error(u, boxes, nboxes, models, nmodels, 1.0f);
}

// The synchronous call's verdict on its records: which array holds the first invalid one (0 none, 1 lights, 2 boxes) and its index.
inline int light_shadow_first_invalid(const RtPointLight* lights, uint32_t count, const RtDrawBox* boxes, uint32_t nboxes, uint32_t* index) {
    *index = first_invalid_point_light(lights, count);
    if (*index != count) return 1;
    *index = first_invalid_draw_box(boxes, nboxes);
    if (*index != nboxes) return 2;
    return 0;
}

}  // namespace rta
