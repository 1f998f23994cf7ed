// lights_check.hpp — the host half of rt_add_lights: the validity test of a batch of RtPointLight records.  Plain C++ with no HIP
// include, so that tests/point_lights_main.cpp runs this very code on the CPU.  The comparisons are the kernel's (rt_lights.hip,
// light_valid): each is false for a NaN, so a record with a NaN fails.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../../include/rt_abi.h"

namespace rta __attribute__((visibility("hidden"))) {

constexpr uint32_t kMaxPointLights = 1024;   // lights per call

// One light: every float finite, |position_k| <= 2^22, 0 < radius <= 1024, 0 <= color_k <= 2^20, reserved == 0.
inline bool point_light_valid(const RtPointLight& l) {
    if (!(l.radius > 0.0f && l.radius <= 1024.0f) || l.reserved != 0u) return false;
    for (int k = 0; k < 3; k++)
        if (!(std::fabs(l.position[k]) <= 4194304.0f && l.color[k] >= 0.0f && l.color[k] <= 1048576.0f)) return false;
    return true;
}

// The index of the first invalid light of a batch, or `count` when every one is valid.
inline uint32_t first_invalid_point_light(const RtPointLight* lights, uint32_t count) {
    for (uint32_t i = 0; i < count; i++)
        if (!point_light_valid(lights[i])) return i;
    return count;
}

}  // namespace rta
