// bench_scene.hpp — the records rt_bench hands to the library: pure host code, functions of one drawn frame's uniforms, the
// seeded generator and their arguments.  Each record is built in one place; a mode calls the builders in the order that consumes
// the generator as its figures were measured with (the orders differ between the modes on purpose: see bench_modes.cpp).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/rt_abi.h"

namespace bench {

// the generator of every seeded scene: xorshift64, 24 bits per value
struct Rng {
    uint64_t x = 0x9E3779B97F4A7C15ull;
    float operator()() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (float)((x >> 40) * (1.0 / 16777216.0)); }   // [0, 1)
};

// one drawn frame's camera and its size in pixels
struct View {
    RtUniforms u{};
    int width = 0, height = 0;
};

// the material of entity i (and of voxel i of a model); the brush of the world edits has one material
inline uint32_t material_word(uint32_t i) { return (1u << 15) | ((40u + i % 80u) << 14) | ((30u + i % 90u) << 7) | (20u + i % 100u); }
constexpr uint32_t BRUSH_MATERIAL = (1u << 15) | (90u << 14) | (60u << 7) | 30u;

// the camera ray's direction through screen position (sx, sy) in [-1, 1]^2 (not normalised), the screen position of a pixel, and
// the point `dist` units along the ray
inline void view_direction(const RtUniforms& u, float sx, float sy, float v[3]) {
    for (int a = 0; a < 3; a++) v[a] = u.forward[a] + u.right[a] * sx + u.up[a] * sy;
}
inline float screen_coord(int pixel, int size) { return ((float)pixel / (float)size) * 2.0f - 1.0f; }
inline void view_point(const RtUniforms& u, float sx, float sy, float dist, float out[3]) {
    float v[3], len = 0.0f;
    view_direction(u, sx, sy, v);
    for (int a = 0; a < 3; a++) len += v[a] * v[a];
    len = std::sqrt(len);
    for (int a = 0; a < 3; a++) out[a] = u.origin[a] + v[a] / len * dist;
}
inline void pixel_point(const View& w, const int32_t xy[2], float dist, float out[3]) {
    view_point(w.u, screen_coord(xy[0], w.width), screen_coord(xy[1], w.height), dist, out);
}

// a seeded point over the whole view, near to 20 near units away, log-uniform (three values of the generator)
inline void scatter_point(const RtUniforms& u, Rng& rnd, float near_dist, float out[3]) {
    const float sx = rnd() * 2.0f - 1.0f, sy = rnd() * 2.0f - 1.0f, dist = near_dist * std::pow(20.0f, rnd());
    view_point(u, sx, sy, dist, out);
}

// a player's box round c: 0.6 x 0.6 x 1.8 (material and emission are the caller's)
inline void player_box(const float c[3], RtDrawBox* b) {
    for (int a = 0; a < 3; a++) { const float half = a == 2 ? 0.9f : 0.3f; b->lo[a] = c[a] - half; b->hi[a] = c[a] + half; }
}

// the models' stamp: a third of the voxels solid, the rest air and absent in turn, a material per voxel (one value of the generator
// per voxel); `id` is the pipeline's, once created there
struct SparseStamp {
    int32_t ext[3];
    std::vector<uint32_t> mats;
    std::vector<uint8_t> state;
    uint32_t id = 0;
};
inline SparseStamp sparse_stamp(Rng& rnd, int32_t ex, int32_t ey, int32_t ez) {
    SparseStamp s{{ex, ey, ez}, std::vector<uint32_t>((size_t)ex * ey * ez), {}, 0};
    s.state.resize(s.mats.size());
    for (size_t i = 0; i < s.mats.size(); i++) {
        s.state[i] = rnd() < 0.3333f ? RT_STAMP_SOLID : (i & 1u ? RT_STAMP_AIR : RT_STAMP_ABSENT);
        s.mats[i] = material_word((uint32_t)i);
    }
    return s;
}

// model i of the stamp, in orientation i % 48, centred at c; `box` (when given) gets its bounding box's corners
inline RtDrawStamp model_at(const SparseStamp& s, float scale, uint32_t i, const float c[3], RtDrawBox* box) {
    static const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    RtDrawStamp m{};
    m.stamp = s.id; m.scale = scale; m.orient = (uint8_t)(i % 48u); m.emission = 0xFF000000u;
    for (int a = 0; a < 3; a++) {
        const float ext = (float)s.ext[perms[m.orient >> 3][a]];
        m.origin[a] = c[a] - 0.5f * ext * scale;
        if (box) { box->lo[a] = m.origin[a]; box->hi[a] = std::fma(ext, scale, m.origin[a]); }
    }
    return m;
}

// the six probes of entity i's box: the face centres, 0.001 off the face along its normal
inline void face_probes(const RtDrawBox& b, uint32_t i, RtLightProbe six[6]) {
    for (uint32_t code = 0; code < 6u; code++) {
        RtLightProbe& q = six[code];
        q = RtLightProbe{};
        for (int a = 0; a < 3; a++) q.position[a] = (b.lo[a] + b.hi[a]) * 0.5f;
        const int a = (int)(code / 2u);
        q.position[a] = code % 2u == 0u ? b.hi[a] + 0.001f : b.lo[a] - 0.001f;
        q.normal = code;
        q.cell[0] = (uint16_t)(i % 16u); q.cell[1] = (uint16_t)((i / 16u) % 16u);
    }
}

// the particles share 64 whole-sphere probes, one per cluster, where the cluster's first particle is
constexpr uint32_t SHARED_LIGHTS = 64;
inline RtLightProbe sphere_probe(uint32_t i, const float at[3]) {
    RtLightProbe l{};
    for (int a = 0; a < 3; a++) l.position[a] = at[a];
    l.normal = RT_PROBE_SPHERE;
    l.cell[0] = (uint16_t)(i % 16u); l.cell[1] = (uint16_t)(i / 16u);
    return l;
}

// n seeded pixels of the view, as rt_pick_pixels takes them (two values of the generator each)
inline std::vector<int32_t> pixel_list(const View& w, Rng& rnd, uint32_t n) {
    std::vector<int32_t> xy(2u * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        xy[2u * i] = std::min(w.width - 1, (int)(rnd() * (float)w.width));
        xy[2u * i + 1] = std::min(w.height - 1, (int)(rnd() * (float)w.height));
    }
    return xy;
}

// lights of radius 8 just off what the picked pixels show: 1 to 4 units off the hit along the face's normal, 30 units along the ray
// where the pixel shows sky (four values of the generator each: the offset, then the colour)
inline std::vector<RtPointLight> lights_off_hits(const View& w, Rng& rnd, const std::vector<int32_t>& xy, const std::vector<RtRayHit>& hits) {
    std::vector<RtPointLight> lights(hits.size());
    for (size_t i = 0; i < hits.size(); i++) {
        RtPointLight& l = lights[i];
        l = RtPointLight{};
        const float off = 1.0f + 3.0f * rnd();
        if (hits[i].kind == RT_HIT_SOLID) {
            for (int a = 0; a < 3; a++) l.position[a] = hits[i].position[a];
            l.position[hits[i].normal / 2u] += hits[i].normal % 2u == 0u ? off : -off;
        } else {
            pixel_point(w, &xy[2u * i], 30.0f, l.position);
        }
        l.radius = 8.0f;
        l.color[0] = 20.0f + 20.0f * rnd(); l.color[1] = 15.0f + 15.0f * rnd(); l.color[2] = 5.0f + 10.0f * rnd();
    }
    return lights;
}

// n rays: the view's primary rays handed over as arbitrary rays, or seeded origins in the region and random directions (six values
// of the generator each)
inline std::vector<RtRay> ray_list(const View& w, Rng& rnd, uint32_t n, bool coherent) {
    std::vector<RtRay> rays(n);
    for (uint32_t i = 0; i < n; i++) {
        RtRay& r = rays[i];
        r = RtRay{};
        if (coherent) {
            const uint32_t px = i % (uint32_t)w.width, py = (i / (uint32_t)w.width) % (uint32_t)w.height;
            for (int a = 0; a < 3; a++) r.origin[a] = w.u.origin[a];
            view_direction(w.u, screen_coord((int)px, w.width), screen_coord((int)py, w.height), r.direction);
        } else {
            for (int a = 0; a < 3; a++) { r.origin[a] = (rnd() - 0.5f) * 254.0f; r.direction[a] = rnd() * 2.0f - 1.0f; }
        }
    }
    return rays;
}

// the world edits' brush: centred 16 texels ahead of the camera (texel coordinates of the 256 region)
inline void brush_centre(const float origin[3], int c[3]) {
    const int R = RT_ROOT_BLOCK_SIZE;
    c[0] = (int)origin[0] + R / 2; c[1] = (int)origin[1] + R / 2 + 16; c[2] = (int)origin[2] + R / 2;
}

}  // namespace bench
