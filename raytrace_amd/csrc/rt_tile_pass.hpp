// rt_tile_pass.hpp — the scaffold of the passes over a drawn frame, one wave64 per 8x8 pixel tile and four tiles per workgroup
// (rt_boxes.hip: k_draw_boxes, rt_draw_stamps.hip: k_draw_stamps, rt_lights.hip: k_add_lights and k_add_lights_occluded,
// rt_shadows.hip: k_shadow_entities, rt_particles.hip: k_draw_particles and the cull of its bin pass):
//   - TileLane: which tile a wave owns and which pixel a lane, and the grid of a launch;
//   - the batch idiom's small pieces: a record's words broadcast from lane j (bcast, rec_xyz), the valid box, a model record decoded;
//   - the entity draws' geometry: the primary direction of a pixel, what the cull knows of a tile's directions (tile_dirs), the
//     conservative test of a box against a tile (box_may_touch_tile), the hit's depth test and the seven planes of a drawn pixel;
//   - the lighting passes' geometry: the surface point P' of a pixel (surface_point) and a tile's bounds of it (tile_point_bounds);
//   - the exact slab test (slab_core; ray_box_slab for a primary ray) of include/rt_abi.h "Entity boxes".
// Device code only.
//
// A pass loads its records 64 at a time, lane l record base + l, tests each conservatively against the tile, makes the keepers a
// 64-bit mask with __ballot and, per set bit j, broadcasts record j's words so that every lane runs the exact test of its own pixel
// with scalar record operands.  That loop stays in each kernel: what a lane carries through it differs per pass.
//
// All arithmetic that decides a pixel is fp32 with one rounding per operation (-ffp-contract=off); the cull may only drop a box the
// exact test rejects for every pixel of the tile (DESIGN.md "Entity boxes" carries the argument for its margins).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rt_abi.h"
#include "rt_kernels.hpp"

namespace rtd {
namespace {

constexpr uint32_t kTileWg = 256;               // four waves, a tile each
constexpr uint32_t kNoRecord = 0xFFFFFFFFu;
constexpr float kPassMaxCoord = 4194304.0f;     // 2^22: the passes' records lie within it
constexpr float kFinite = 3.0e38f;

// The tile of this wave and the pixel of this lane in a frame of width x height.
struct TileLane {
    uint32_t lane;
    int px0, py0, px, py;   // the tile's low pixel, the lane's pixel
    bool live;              // false past the last tile: the whole wave ends (the kernels have no barrier)
    bool inside;            // the pixel lies in the frame (an edge tile's lanes may not)
    size_t pix;             // row-major index of the pixel
    __device__ __forceinline__ TileLane(int width, int height) {
        lane = threadIdx.x & 63u;
        const uint32_t tile = blockIdx.x * (kTileWg / 64u) + (threadIdx.x >> 6);
        const uint32_t tiles_x = ((uint32_t)width + 7u) / 8u, tiles_y = ((uint32_t)height + 7u) / 8u;
        live = tile < tiles_x * tiles_y;
        px0 = (int)(tile % tiles_x) * 8; py0 = (int)(tile / tiles_x) * 8;
        px = px0 + (int)(lane & 7u); py = py0 + (int)(lane >> 3);
        inside = px < width && py < height;
        pix = (size_t)py * (size_t)width + (size_t)px;
    }
    // the grid that gives every tile of a (non-empty) frame a wave
    static dim3 grid(int width, int height) {
        const uint32_t tiles = (((uint32_t)width + 7u) / 8u) * (((uint32_t)height + 7u) / 8u);
        return dim3((tiles + kTileWg / 64u - 1u) / (kTileWg / 64u));
    }
};

__device__ __forceinline__ uint32_t bcast(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }
// .xyz of a record's word as floats (a box's lo or hi corner, a light's position or colour): this lane's, or lane j's in every lane
__device__ __forceinline__ void rec_xyz(uint4 w, float out[3]) {
    out[0] = __uint_as_float(w.x); out[1] = __uint_as_float(w.y); out[2] = __uint_as_float(w.z);
}
__device__ __forceinline__ void rec_xyz(uint4 w, int j, float out[3]) {
    out[0] = __uint_as_float(bcast(w.x, j)); out[1] = __uint_as_float(bcast(w.y, j)); out[2] = __uint_as_float(bcast(w.z, j));
}

__device__ __forceinline__ float wave_max(float v) {   // (fmaxf drops a NaN)
    for (int s = 32; s > 0; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
    return v;
}

// The contract's valid box (every comparison is false for a NaN).
__device__ __forceinline__ bool box_valid(const float lo[3], const float hi[3]) {
    bool ok = true;
    for (int k = 0; k < 3; k++) ok = ok && rtm_abs(lo[k]) <= kPassMaxCoord && rtm_abs(hi[k]) <= kPassMaxCoord && lo[k] < hi[k];
    return ok;
}

// What a walk of a model's cells starts from: lane j's 64-byte record (api/draw_stamps.hpp, DrawStampRecord; words w0..w3) in every
// lane.  Cell c (0 <= c_k < ext[k]) shows state[base + sum_k stride[k] * c[k]]; the bounding box is rec_xyz(w2, j), rec_xyz(w3, j).
struct ModelRec {
    const uint8_t* state;
    int base, ext[3], stride[3];
    float scale;
};
__device__ __forceinline__ ModelRec model_rec(uint4 w0, uint4 w1, uint4 w2, int j) {
    ModelRec m;
    m.state = reinterpret_cast<const uint8_t*>((uint64_t)bcast(w0.z, j) | ((uint64_t)bcast(w0.w, j) << 32));
    m.base = (int)bcast(w1.x, j);
    const uint32_t se[3] = {bcast(w1.y, j), bcast(w1.z, j), bcast(w1.w, j)};
    for (int k = 0; k < 3; k++) {
        m.ext[k] = (int)((se[k] >> 18) & 0xFFu) + 1;
        m.stride[k] = (int)(se[k] << 14) >> 14;
    }
    m.scale = __uint_as_float(bcast(w2.w, j));
    return m;
}

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
// depend on the other, and sx / sy are monotone in the pixel — so every pixel's v lies between the four corners' values.  That holds
// for any pixel rectangle px0 .. px0 + dx, py0 .. py0 + dy, not only for a tile: rt_particles.hip bins with rectangles of many tiles.
template <typename Args>
__device__ __forceinline__ TileDirs tile_dirs(const Args& a, int px0, int py0, float omax, int dx = 7, int dy = 7) {
    TileDirs td;
    td.flags = 0u;
    const vec3 c00 = primary_unnormalised(a, px0, py0), c10 = primary_unnormalised(a, px0 + dx, py0);
    const vec3 c01 = primary_unnormalised(a, px0, py0 + dy), c11 = primary_unnormalised(a, px0 + dx, py0 + dy);
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

// The slab test of the line through o against the box [lo, hi] (rt_abi.h "Slab test of box b"): nonzero[k] says whether the
// direction's component k is not zero, inv[k] is its reciprocal.  Does the line cross the box at all — some axis bounds it and every
// zero-direction axis passes — and then t_in, t_out and the entry axis.
__device__ __forceinline__ bool slab_core(const float lo[3], const float hi[3], const float o[3], const bool nonzero[3], const float inv[3],
                                          float* t_in_out, float* t_out_out, uint32_t* axis_out) {
    bool bounded = false, miss = false;
    float t_in = 0.0f, t_out = 0.0f;
    uint32_t axis = 0u;
    for (int k = 0; k < 3; k++) {
        if (nonzero[k]) {
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
    return bounded && !miss;
}

// The exact test of one ray (o, d, inv = 1.0f / d per component): it enters the box from outside, in front of its origin.
__device__ __forceinline__ bool ray_box_slab(const float lo[3], const float hi[3], const float o[3], const float d[3], const float inv[3],
                                             float* t_in, float* t_out, uint32_t* axis) {
    const bool nonzero[3] = {d[0] != 0.0f, d[1] != 0.0f, d[2] != 0.0f};
    return slab_core(lo, hi, o, nonzero, inv, t_in, t_out, axis) && *t_in > 0.0f && *t_in < *t_out;
}

// ---- the entity draws: the ray of a pixel, and what a lane whose ray hit an entity at t, entering by `axis`, does with it ------------
// This lane's primary ray: d normalised, inv = 1.0f / d per component.
template <typename Args>
__device__ __forceinline__ void primary_dir(const Args& a, int px, int py, float d[3], float inv[3]) {
    const vec3 dv = vnormalize(primary_unnormalised(a, px, py));
    d[0] = dv.x; d[1] = dv.y; d[2] = dv.z;
    for (int k = 0; k < 3; k++) inv[k] = 1.0f / d[k];
}

// The depth test of the hit against the pixel's depth_f32 (store_primary_planes' expression); then the hit's depth and face.
__device__ __forceinline__ bool entity_hit_shows(const float o[3], const float d[3], float t, uint32_t axis, float depth, float* depth_f, uint32_t* normal) {
    const vec3 P = v3(rtm_fma(d[0], t, o[0]), rtm_fma(d[1], t, o[1]), rtm_fma(d[2], t, o[2]));
    *depth_f = vlength(vsub(v3(o[0], o[1], o[2]), P)) * 32.0f;
    const float da = axis == 0u ? d[0] : (axis == 1u ? d[1] : d[2]);
    *normal = 2u * axis + (da > 0.0f ? 1u : 0u);
    return *depth_f < depth;
}

// The seven planes of a pixel that shows an entity.
__device__ __forceinline__ void store_entity_pixel(const Planes& pl, size_t pix, float depth_f, uint32_t normal, uint32_t material, uint32_t emission,
                                                   float4 light) {
    pl.depth_f32[pix] = depth_f;
    pl.depth_r16[pix] = (uint16_t)rtm_f2u16(depth_f);
    pl.normal_r8[pix] = (uint8_t)normal;
    const vec3 alb = albedo_of(material);
    pl.albedo_rgba8[pix] = pack_rgba8(alb.x, alb.y, alb.z, 1.0f);
    pl.emission_rgba8[pix] = emission;
    store_lighting(pl, (uint32_t)pix, v3(light.x, light.y, light.z), 1);
}

// ---- the lighting passes: where a pixel's surface lies ------------------------------------------------------------------------------
// The surface point P' of pixel (px, py): its primary ray as far as the depth plane says, moved 1/32 off the face the normal names.
__device__ __forceinline__ void surface_point(const Frame& f, int px, int py, float depth, uint32_t normal, float P[3]) {
    const vec3 dv = vnormalize(primary_unnormalised(f, px, py));
    const float t = depth / 32.0f;
    P[0] = rtm_fma(dv.x, t, f.origin[0]); P[1] = rtm_fma(dv.y, t, f.origin[1]); P[2] = rtm_fma(dv.z, t, f.origin[2]);
    const uint32_t axis = (normal >> 1) & 3u;
    const float off = (normal & 1u) == 0u ? 0.03125f : -0.03125f;
    if (axis == 0u) P[0] = P[0] + off; else if (axis == 1u) P[1] = P[1] + off; else P[2] = P[2] + off;
}

// The bounds of the finite P' of the tile's surface pixels, the same in every lane; `bounded`: this lane's is one of them.
__device__ __forceinline__ bool tile_point_bounds(bool surface, const float P[3], float lo[3], float hi[3]) {
    const bool bounded = surface && rtm_abs(P[0]) <= kFinite && rtm_abs(P[1]) <= kFinite && rtm_abs(P[2]) <= kFinite;
    for (int k = 0; k < 3; k++) {
        lo[k] = bounded ? P[k] : INFINITY;
        hi[k] = bounded ? P[k] : -INFINITY;
        for (int s = 32; s > 0; s >>= 1) {   // (both at once: two exchanges in flight per step)
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], s, 64));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], s, 64));
        }
    }
    return bounded;
}

}  // namespace
}  // namespace rtd
