// rt_boxes.hpp — what the kernels that composite entities into a frame's planes share (rt_boxes.hip: k_draw_boxes, rt_draw_stamps.hip:
// k_draw_stamps): the primary direction of a pixel, what the cull knows of an 8x8 tile's directions, the conservative test of a box
// against a tile and the exact slab test of one ray (include/rt_abi.h "Entity boxes").  Device code only.
//
// All arithmetic that decides a pixel is fp32 with one rounding per operation (-ffp-contract=off); the cull may only drop a box the
// exact test rejects for every pixel of the tile (DESIGN.md "Entity boxes" carries the argument for its margins).
#pragma once
#include <hip/hip_runtime.h>

#include "rt_device.hpp"

namespace rtd {
namespace {

constexpr float kBoxMaxCoord = 4194304.0f;   // 2^22
// the cull's margins: relative 2^-16 on a slab bound (the exact test's own error against real arithmetic is below 2^-21) and an
// absolute 1e-30 for products that went denormal; depth: 2^-12 relative (as its reciprocal), 2^-19 of the coordinates' size absolute
constexpr float kCullRel = 1.0f / 65536.0f;
constexpr float kCullAbs = 1.0e-30f;
constexpr float kCullInvDepthRel = 1.00025f;     // above 1 / (1 - 2^-12)
constexpr float kCullDepthAbs = 1.0f / 524288.0f;
constexpr float kCullMinDir = 9.094947e-13f;     // 2^-40: a direction component below it bounds nothing in the cull
constexpr float kCullMaxLen2 = 1.0995116e12f;    // 2^40: the cull trusts |v|^2 between 2^-40 and 2^40 only
constexpr float kCullMinLen2 = 9.094947e-13f;

// What the cull knows of a tile's directions, per axis.  A range that keeps clear of zero (`bounds`): mirrored to positive (`mirror`),
// the reciprocals of its ends.  A range that touches zero (`straddles`): the reciprocals of its positive end (inv_hi) and of minus its
// negative end (inv_lo), 0 where that end is too small to bound anything.
// (The flags are bits of one word — mirror at bit k, bounds at 3 + k, straddles at 6 + k, sane at 9 — so that they live in one
// register and not in a lane mask each.)
struct TileDirs {
    float inv_lo[3], inv_hi[3];
    uint32_t flags;
    __device__ __forceinline__ bool mirror(int k) const { return (flags >> k & 1u) != 0u; }
    __device__ __forceinline__ bool bounds(int k) const { return (flags >> (3 + k) & 1u) != 0u; }
    __device__ __forceinline__ bool straddles(int k) const { return (flags >> (6 + k) & 1u) != 0u; }
    __device__ __forceinline__ bool sane() const { return (flags >> 9 & 1u) != 0u; }
};

// The unnormalised primary direction of pixel (px, py), primary_ray's expression (Args: width, height, forward, right, up).
template <typename Args>
__device__ __forceinline__ vec3 primary_unnormalised(const Args& a, int px, int py) {
    const float sx = ((float)px / (float)a.width) * 2.0f - 1.0f;
    const float sy = ((float)py / (float)a.height) * 2.0f - 1.0f;
    return vadd(vadd(ld3(a.forward), vscale(ld3(a.right), sx)), vscale(ld3(a.up), sy));
}

// What the cull knows of the tile whose low pixel is (px0, py0) (the same in every lane); omax = the largest |o_k|.
// v is fl(fl(forward + fl(right * sx)) + fl(up * sy)) per component: monotone in sx and in sy, each in a direction that does not
// depend on the other, and sx / sy are monotone in the pixel — so every pixel's v lies between the four corners' values.
template <typename Args>
__device__ __forceinline__ TileDirs tile_dirs(const Args& a, int px0, int py0, float omax) {
    TileDirs td;
    td.flags = 0u;
    const vec3 c00 = primary_unnormalised(a, px0, py0), c10 = primary_unnormalised(a, px0 + 7, py0);
    const vec3 c01 = primary_unnormalised(a, px0, py0 + 7), c11 = primary_unnormalised(a, px0 + 7, py0 + 7);
    const float c[4][3] = {{c00.x, c00.y, c00.z}, {c10.x, c10.y, c10.z}, {c01.x, c01.y, c01.z}, {c11.x, c11.y, c11.z}};
    float len2_min = 0.0f, len2_max = 0.0f;
    bool finite = true;
    for (int k = 0; k < 3; k++) {
        float lo_v = c[0][k], hi_v = c[0][k];
        for (int q = 0; q < 4; q++) {
            lo_v = fminf(lo_v, c[q][k]); hi_v = fmaxf(hi_v, c[q][k]);
            finite = finite && rtm_abs(c[q][k]) <= 3.0e38f;
        }
        float vl = lo_v, vh = hi_v;
        const bool mirror = hi_v < 0.0f;
        if (mirror) { vl = -hi_v; vh = -lo_v; }
        const bool straddles = lo_v <= 0.0f && hi_v >= 0.0f;
        const bool bounds = !straddles && vl >= kCullMinDir;
        td.flags |= (mirror ? 1u : 0u) << k | (bounds ? 1u : 0u) << (3 + k) | (straddles ? 1u : 0u) << (6 + k);
        td.inv_lo[k] = 1.0f / vl; td.inv_hi[k] = 1.0f / vh;
        if (straddles) {
            td.inv_lo[k] = -lo_v >= kCullMinDir ? 1.0f / -lo_v : 0.0f;
            td.inv_hi[k] = hi_v >= kCullMinDir ? 1.0f / hi_v : 0.0f;
        }
        const float amax = rtm_max(rtm_abs(lo_v), rtm_abs(hi_v));
        const float amin = (lo_v <= 0.0f && hi_v >= 0.0f) ? 0.0f : rtm_min(rtm_abs(lo_v), rtm_abs(hi_v));
        len2_min = rtm_fma(amin, amin, len2_min);
        len2_max = rtm_fma(amax, amax, len2_max);
    }
    td.flags |= (finite && len2_min >= kCullMinLen2 && len2_max <= kCullMaxLen2 && omax <= 3.0e38f ? 1u : 0u) << 9;
    return td;
}

// Conservative: false only when the exact test below rejects the box for every pixel of the tile, or no pixel of it would pass the
// depth test.  Every rejection is a comparison that is false for a NaN, so a NaN keeps the box.
__device__ __forceinline__ bool box_may_touch_tile(const float lo[3], const float hi[3], const float o[3], const TileDirs& td, float omax,
                                                   float tile_depth) {
    if (!td.sane()) return true;
    float tn_lo = -INFINITY, tf_hi = INFINITY, dist2 = 0.0f, ext = 0.0f;
    for (int k = 0; k < 3; k++) {
        const float A = lo[k] - o[k], B = hi[k] - o[k];   // the exact test's own differences
        const float gap = rtm_max(rtm_max(A, -B), 0.0f);  // distance from o to the slab on this axis
        dist2 = rtm_fma(gap, gap, dist2);
        ext = rtm_max(ext, rtm_max(rtm_abs(A), rtm_abs(B)));
        if (td.straddles(k)) {
            // v in [-1 / inv_lo, 1 / inv_hi] round zero.  A ray that reaches a slab lying wholly on one side (A > 0 or B < 0) has v of
            // that side and enters no earlier than with the largest such |v|; rays of the other side (and v == 0) miss the box
            // outright.  No far bound: a ray with v near zero stays in a slab that contains o for ever.
            float tn = -INFINITY;
            if (A > 0.0f && td.inv_hi[k] > 0.0f) tn = A * td.inv_hi[k];
            else if (B < 0.0f && td.inv_lo[k] > 0.0f) tn = -B * td.inv_lo[k];
            tn_lo = rtm_max(tn_lo, tn - rtm_abs(tn) * kCullRel - kCullAbs);
            continue;
        }
        if (!td.bounds(k)) continue;                      // a one-signed range with an end below 2^-40: this axis bounds nothing here
        const float a0 = td.mirror(k) ? -B : A, b0 = td.mirror(k) ? -A : B;   // the axis mirrored: the direction is positive
        // tn = a0 / v, tf = b0 / v over v in [vl, vh], in units of 1 / |v| (the same positive factor on every axis of one pixel);
        // the tile's reciprocals stand in for the divisions: one more rounding, far inside the margin
        const float tn = a0 * (a0 >= 0.0f ? td.inv_hi[k] : td.inv_lo[k]);
        const float tf = b0 * (b0 >= 0.0f ? td.inv_lo[k] : td.inv_hi[k]);
        tn_lo = rtm_max(tn_lo, tn - rtm_abs(tn) * kCullRel - kCullAbs);
        tf_hi = rtm_min(tf_hi, tf + rtm_abs(tf) * kCullRel + kCullAbs);
    }
    if (tf_hi < 0.0f) return false;       // some far plane lies behind every ray: t_out < 0
    if (tn_lo >= tf_hi) return false;     // some near plane lies beyond some far plane for every ray: t_in >= t_out
    // no hit point can be nearer than the tile's farthest pixel: 32 (D (1 - 2^-12) - 2^-19 (omax + ext)) >= tile_depth, D = sqrt(dist2),
    // solved for D and squared
    const float need = (tile_depth * (1.0f / 32.0f) + (omax + ext) * kCullDepthAbs) * kCullInvDepthRel;
    if (need <= 0.0f || dist2 >= need * need) return false;
    return true;
}

// The exact slab test of one ray (o, d, inv = 1.0f / d per component) against the box [lo, hi]: hit, and then t_in, t_out and the
// entry axis (rt_abi.h "Slab test of box b").
__device__ __forceinline__ bool ray_box_slab(const float lo[3], const float hi[3], const float o[3], const float d[3], const float inv[3],
                                             float* t_in_out, float* t_out_out, uint32_t* axis_out) {
    bool bounded = false, miss = false;
    float t_in = 0.0f, t_out = 0.0f;
    uint32_t axis = 0u;
    for (int k = 0; k < 3; k++) {
        if (d[k] != 0.0f) {
            const float t0 = (lo[k] - o[k]) * inv[k], t1 = (hi[k] - o[k]) * inv[k];
            const float tn = rtm_min(t0, t1), tf = rtm_max(t0, t1);
            if (!bounded) { t_in = tn; t_out = tf; axis = (uint32_t)k; bounded = true; }
            else {
                if (tn > t_in) { t_in = tn; axis = (uint32_t)k; }
                if (tf < t_out) t_out = tf;
            }
        } else if (!(lo[k] < o[k] && o[k] < hi[k])) {
            miss = true;
        }
    }
    *t_in_out = t_in; *t_out_out = t_out; *axis_out = axis;
    return bounded && !miss && t_in > 0.0f && t_in < t_out;
}

}  // namespace
}  // namespace rtd
