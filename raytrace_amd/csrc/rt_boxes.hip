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
// The cull and the exact slab test are rt_boxes.hpp's, shared with k_draw_stamps.
#include <hip/hip_runtime.h>

#include "rt_boxes.hpp"
#include "rt_kernels.hpp"

namespace rtd {

namespace {

constexpr uint32_t kBoxesWg = 256;
constexpr uint32_t kNoBox = 0xFFFFFFFFu;

__device__ __forceinline__ bool box_valid(const float lo[3], const float hi[3]) {
    bool ok = true;
    for (int k = 0; k < 3; k++) ok = ok && rtm_abs(lo[k]) <= kBoxMaxCoord && rtm_abs(hi[k]) <= kBoxMaxCoord && lo[k] < hi[k];
    return ok;
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
    const float omax = rtm_max(rtm_max(rtm_abs(o[0]), rtm_abs(o[1])), rtm_abs(o[2]));
    const TileDirs td = tile_dirs(a, px0, py0, omax);
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
            float t_in, t_out;
            uint32_t axis;
            const bool hit = ray_box_slab(lo, hi, o, d, inv, &t_in, &t_out, &axis);
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
