// rt_boxes.hip — gfx950 kernel of rt_draw_boxes / rt_draw_boxes_async: world-space axis-aligned boxes composited into the planes of
// the frame drawn last, by depth (include/rt_abi.h "Entity boxes"; the rules are restated, without a cull, in tests/draw_boxes_ref.py).
//
//   k_draw_boxes : one wave64 owns one 8x8 pixel tile, a workgroup four tiles.  Per batch of 64 boxes lane l loads box base + l (two
//                  16-byte loads), tests its validity and runs a conservative interval slab test against the tile (box_may_touch_tile);
//                  __ballot makes the candidates a 64-bit mask, and for each set bit the candidate's words are broadcast with
//                  v_readlane and every lane runs the exact slab test of its own ray with scalar box operands.  A lane keeps
//                  (t_in, index, axis) of its best box; winners compute the hit point, compare depths, gather their face light
//                  (16 bytes) and store seven planes.  No LDS, no atomics; the only cross-lane traffic is the ballot, the readlanes and
//                  one max reduction of the tile's depths.
//
// All arithmetic that decides a pixel is fp32 with one rounding per operation (-ffp-contract=off); the cull may only drop a box the
// exact test rejects for every pixel of the tile (DESIGN.md "Entity boxes" carries the argument for its margins).
#include <hip/hip_runtime.h>

#include "rt_kernels.hpp"

namespace rtd {

namespace {

constexpr uint32_t kBoxesWg = 256;
constexpr float kBoxMaxCoord = 4194304.0f;   // 2^22
constexpr uint32_t kNoBox = 0xFFFFFFFFu;
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
struct TileDirs { float inv_lo[3], inv_hi[3]; bool mirror[3], bounds[3], straddles[3]; bool sane; };

// The unnormalised primary direction of pixel (px, py), primary_ray's expression.
__device__ __forceinline__ vec3 primary_unnormalised(const DrawBoxesArgs& a, int px, int py) {
    const float sx = ((float)px / (float)a.width) * 2.0f - 1.0f;
    const float sy = ((float)py / (float)a.height) * 2.0f - 1.0f;
    return vadd(vadd(ld3(a.forward), vscale(ld3(a.right), sx)), vscale(ld3(a.up), sy));
}

__device__ __forceinline__ bool box_valid(const float lo[3], const float hi[3]) {
    bool ok = true;
    for (int k = 0; k < 3; k++) ok = ok && rtm_abs(lo[k]) <= kBoxMaxCoord && rtm_abs(hi[k]) <= kBoxMaxCoord && lo[k] < hi[k];
    return ok;
}

// Conservative: false only when the exact test below rejects the box for every pixel of the tile, or no pixel of it would pass the
// depth test.  Every rejection is a comparison that is false for a NaN, so a NaN keeps the box.
__device__ __forceinline__ bool box_may_touch_tile(const float lo[3], const float hi[3], const float o[3], const TileDirs& td, float omax,
                                                   float tile_depth) {
    if (!td.sane) return true;
    float tn_lo = -INFINITY, tf_hi = INFINITY, dist2 = 0.0f, ext = 0.0f;
    for (int k = 0; k < 3; k++) {
        const float A = lo[k] - o[k], B = hi[k] - o[k];   // the exact test's own differences
        const float gap = rtm_max(rtm_max(A, -B), 0.0f);  // distance from o to the slab on this axis
        dist2 = rtm_fma(gap, gap, dist2);
        ext = rtm_max(ext, rtm_max(rtm_abs(A), rtm_abs(B)));
        if (td.straddles[k]) {
            // v in [-1 / inv_lo, 1 / inv_hi] round zero.  A ray that reaches a slab lying wholly on one side (A > 0 or B < 0) has v of
            // that side and enters no earlier than with the largest such |v|; rays of the other side (and v == 0) miss the box
            // outright.  No far bound: a ray with v near zero stays in a slab that contains o for ever.
            float tn = -INFINITY;
            if (A > 0.0f && td.inv_hi[k] > 0.0f) tn = A * td.inv_hi[k];
            else if (B < 0.0f && td.inv_lo[k] > 0.0f) tn = -B * td.inv_lo[k];
            tn_lo = rtm_max(tn_lo, tn - rtm_abs(tn) * kCullRel - kCullAbs);
            continue;
        }
        if (!td.bounds[k]) continue;                      // a one-signed range with an end below 2^-40: this axis bounds nothing here
        const float a0 = td.mirror[k] ? -B : A, b0 = td.mirror[k] ? -A : B;   // the axis mirrored: the direction is positive
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

__global__ __launch_bounds__(kBoxesWg) void k_draw_boxes(Planes pl, DrawBoxesArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tile = blockIdx.x * (kBoxesWg / 64u) + (threadIdx.x >> 6);
    const uint32_t tiles_x = ((uint32_t)a.width + 7u) / 8u, tiles_y = ((uint32_t)a.height + 7u) / 8u;
    if (tile >= tiles_x * tiles_y) return;   // (a whole wave: the kernel has no barrier)
    const int px0 = (int)(tile % tiles_x) * 8, py0 = (int)(tile / tiles_x) * 8;
    const int px = px0 + (int)(lane & 7u), py = py0 + (int)(lane >> 3);
    const bool inside = px < a.width && py < a.height;
    const size_t pix = (size_t)py * (size_t)a.width + (size_t)px;

    const float o[3] = {a.origin[0], a.origin[1], a.origin[2]};
    const vec3 dv = vnormalize(primary_unnormalised(a, px, py));
    const float d[3] = {dv.x, dv.y, dv.z};
    float inv[3];
    for (int k = 0; k < 3; k++) inv[k] = 1.0f / d[k];
    const float depth = inside ? pl.depth_f32[pix] : -INFINITY;

    // ---- what the cull knows of the tile (the same in every lane) ----
    // v is fl(fl(forward + fl(right * sx)) + fl(up * sy)) per component: monotone in sx and in sy, each in a direction that does not
    // depend on the other, and sx / sy are monotone in the pixel — so every pixel's v lies between the four corners' values.
    const float omax = rtm_max(rtm_max(rtm_abs(o[0]), rtm_abs(o[1])), rtm_abs(o[2]));
    TileDirs td;
    {
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
            td.mirror[k] = hi_v < 0.0f;
            if (td.mirror[k]) { vl = -hi_v; vh = -lo_v; }
            td.straddles[k] = lo_v <= 0.0f && hi_v >= 0.0f;
            td.bounds[k] = !td.straddles[k] && vl >= kCullMinDir;
            td.inv_lo[k] = 1.0f / vl; td.inv_hi[k] = 1.0f / vh;
            if (td.straddles[k]) {
                td.inv_lo[k] = -lo_v >= kCullMinDir ? 1.0f / -lo_v : 0.0f;
                td.inv_hi[k] = hi_v >= kCullMinDir ? 1.0f / hi_v : 0.0f;
            }
            const float amax = rtm_max(rtm_abs(lo_v), rtm_abs(hi_v));
            const float amin = (lo_v <= 0.0f && hi_v >= 0.0f) ? 0.0f : rtm_min(rtm_abs(lo_v), rtm_abs(hi_v));
            len2_min = rtm_fma(amin, amin, len2_min);
            len2_max = rtm_fma(amax, amax, len2_max);
        }
        td.sane = finite && len2_min >= kCullMinLen2 && len2_max <= kCullMaxLen2 && omax <= 3.0e38f;
    }
    float tile_depth = depth;   // the largest depth_f32 of the tile's pixels (fmaxf drops a NaN: such a pixel is never drawn)
    for (int s = 32; s > 0; s >>= 1) tile_depth = fmaxf(tile_depth, __shfl_xor(tile_depth, s, 64));

    float best_t = INFINITY;
    uint32_t best = kNoBox, best_axis = 0u;
    for (uint32_t base = 0; base < a.count; base += 64u) {
        const uint32_t mine = base + lane;
        uint4 w0 = make_uint4(0u, 0u, 0u, 0u), w1 = w0;
        bool keep = false;
        if (mine < a.count) {
            w0 = a.boxes[2u * (size_t)mine];
            w1 = a.boxes[2u * (size_t)mine + 1u];
            const float lo[3] = {__uint_as_float(w0.x), __uint_as_float(w0.y), __uint_as_float(w0.z)};
            const float hi[3] = {__uint_as_float(w1.x), __uint_as_float(w1.y), __uint_as_float(w1.z)};
            keep = box_valid(lo, hi) && box_may_touch_tile(lo, hi, o, td, omax, tile_depth);
        }
        unsigned long long cand = __ballot(keep);
        while (cand) {
            const int j = __builtin_ctzll(cand);
            cand &= cand - 1ull;
            const float lo[3] = {__uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)w0.x, j)),
                                 __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)w0.y, j)),
                                 __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)w0.z, j))};
            const float hi[3] = {__uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)w1.x, j)),
                                 __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)w1.y, j)),
                                 __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)w1.z, j))};
            // the exact slab test of this lane's ray
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
            const bool hit = bounded && !miss && t_in > 0.0f && t_in < t_out;
            if (hit && t_in < best_t) { best_t = t_in; best = base + (uint32_t)j; best_axis = axis; }
        }
    }

    if (!inside || best == kNoBox) return;
    const vec3 P = v3(rtm_fma(d[0], best_t, o[0]), rtm_fma(d[1], best_t, o[1]), rtm_fma(d[2], best_t, o[2]));
    const float depth_f = vlength(vsub(v3(o[0], o[1], o[2]), P)) * 32.0f;    // store_primary_planes' expression
    if (!(depth_f < depth)) return;
    const float da = best_axis == 0u ? d[0] : (best_axis == 1u ? d[1] : d[2]);
    const uint32_t normal = 2u * best_axis + (da > 0.0f ? 1u : 0u);
    const uint32_t material = a.boxes[2u * (size_t)best].w, emission = a.boxes[2u * (size_t)best + 1u].w;
    const float4 light = a.lights[6u * (size_t)best + normal];
    pl.depth_f32[pix] = depth_f;
    pl.depth_r16[pix] = (uint16_t)rtm_f2u16(depth_f);
    pl.normal_r8[pix] = (uint8_t)normal;
    const vec3 alb = albedo_of(material);
    pl.albedo_rgba8[pix] = pack_rgba8(alb.x, alb.y, alb.z, 1.0f);
    pl.emission_rgba8[pix] = emission;
    store_lighting(pl, (uint32_t)pix, v3(light.x, light.y, light.z), 1);
}

}  // namespace

hipError_t launch_draw_boxes(const Planes& pl, const DrawBoxesArgs& a, hipStream_t st) {
    if (a.count == 0u || a.width <= 0 || a.height <= 0) return hipSuccess;
    const uint32_t tiles = (((uint32_t)a.width + 7u) / 8u) * (((uint32_t)a.height + 7u) / 8u);
    hipLaunchKernelGGL(k_draw_boxes, dim3((tiles + kBoxesWg / 64u - 1u) / (kBoxesWg / 64u)), dim3(kBoxesWg), 0, st, pl, a);
    return hipGetLastError();
}

}  // namespace rtd
