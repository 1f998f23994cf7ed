// rt_draw_stamps.hip — gfx950 kernel of rt_draw_stamps / rt_draw_stamps_async: voxel stamps placed as entities at float positions,
// scales and any of the 48 orientations, composited into the planes of the frame drawn last by depth (include/rt_abi.h "Voxel-model
// entities"; the rules are restated, without a cull, in tests/draw_stamps_ref.py).
//
//   k_draw_stamps : k_draw_boxes' shape: one wave64 owns one 8x8 pixel tile, a workgroup four tiles.  Per batch of 64 models lane l
//                   loads record base + l (four 16-byte loads) and runs box_may_touch_tile on its bounding box; __ballot makes the
//                   candidates a 64-bit mask, and for each set bit the record is broadcast with v_readlane, so that every lane runs
//                   the exact slab test and then the voxel walk of its own ray with scalar model operands.  The walk reads one state
//                   byte per cell from global memory (a model is a few KiB: the caches serve it) and keeps the cell's index in the
//                   stamp's arrays by adding a stride per step.  A lane keeps (t, model, axis, voxel) of its best hit; winners compute
//                   the hit point, compare depths, fetch the voxel's material word and the face light and store seven planes.  No
//                   LDS, no atomics.
//
// A model whose bounding box is entered no sooner than the lane's best hit so far is not walked: the walk only ever raises t above
// t_in, and on equal t the lower index wins.
#include <hip/hip_runtime.h>

#include "../../include/rt_abi.h"
#include "rt_boxes.hpp"
#include "rt_kernels.hpp"

namespace rtd {

namespace {

constexpr uint32_t kStampsWg = 256;
constexpr uint32_t kNoModel = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t bcast(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }

__global__ __launch_bounds__(kStampsWg) void k_draw_stamps(Planes pl, DrawStampsArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tile = blockIdx.x * (kStampsWg / 64u) + (threadIdx.x >> 6);
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

    const float omax = rtm_max(rtm_max(rtm_abs(o[0]), rtm_abs(o[1])), rtm_abs(o[2]));
    TileDirs td = tile_dirs(a, px0, py0, omax);
    float tile_depth = depth;   // the largest depth_f32 of the tile's pixels (fmaxf drops a NaN: such a pixel is never drawn)
    for (int s = 32; s > 0; s >>= 1) tile_depth = fmaxf(tile_depth, __shfl_xor(tile_depth, s, 64));

    float best_t = INFINITY;
    uint32_t best = kNoModel, best_axis = 0u, best_voxel = 0u;
    for (uint32_t first = 0; first < a.count; first += 64u) {
        const uint32_t mine = first + lane;
        uint4 w0 = make_uint4(0u, 0u, 0u, 0u), w1 = w0, w2 = w0, w3 = w0;
        bool keep = false;
        // (the cull's flags stay one word in a vector register: as ten lane masks, hoisted out of this loop, they would not fit
        // beside the walk's scalars)
        asm volatile("" : "+v"(td.flags));
        if (mine < a.count) {
            w0 = a.recs[4u * (size_t)mine];
            w1 = a.recs[4u * (size_t)mine + 1u];
            w2 = a.recs[4u * (size_t)mine + 2u];
            w3 = a.recs[4u * (size_t)mine + 3u];
            const float lo[3] = {__uint_as_float(w2.x), __uint_as_float(w2.y), __uint_as_float(w2.z)};
            const float hi[3] = {__uint_as_float(w3.x), __uint_as_float(w3.y), __uint_as_float(w3.z)};
            keep = box_may_touch_tile(lo, hi, o, td, omax, tile_depth);
        }
        unsigned long long cand = __ballot(keep);
        while (cand) {
            const int j = __builtin_ctzll(cand);
            cand &= cand - 1ull;
            const float lo[3] = {__uint_as_float(bcast(w2.x, j)), __uint_as_float(bcast(w2.y, j)), __uint_as_float(bcast(w2.z, j))};
            const float hi[3] = {__uint_as_float(bcast(w3.x, j)), __uint_as_float(bcast(w3.y, j)), __uint_as_float(bcast(w3.z, j))};
            float t_in, t_out;
            uint32_t axis;
            const bool enters = ray_box_slab(lo, hi, o, d, inv, &t_in, &t_out, &axis);
            if (!(inside && enters && t_in < best_t)) continue;   // (a lane past the frame's edge draws nothing)

            // ---- the walk of this lane's ray through the model's cells ----
            const float scale = __uint_as_float(bcast(w2.w, j));
            const uint8_t* state = reinterpret_cast<const uint8_t*>((uint64_t)bcast(w0.z, j) | ((uint64_t)bcast(w0.w, j) << 32));
            const uint32_t se0 = bcast(w1.y, j), se1 = bcast(w1.z, j), se2 = bcast(w1.w, j);
            const int ex = (int)((se0 >> 18) & 0xFFu) + 1, ey = (int)((se1 >> 18) & 0xFFu) + 1, ez = (int)((se2 >> 18) & 0xFFu) + 1;
            const int sx = (int)(se0 << 14) >> 14, sy = (int)(se1 << 14) >> 14, sz = (int)(se2 << 14) >> 14;
            // the first cell: the entry axis' first or last layer, elsewhere where the entry point lies
            int c[3];
            const int ext[3] = {ex, ey, ez};
            for (int k = 0; k < 3; k++) {
                const float p = d[k] == 0.0f ? o[k] : rtm_fma(d[k], t_in, o[k]);
                const float q = rtm_floor((p - lo[k]) / scale), qmax = (float)(ext[k] - 1);   // clamped as a float: the same cell
                const int ck = (int)(!(q > 0.0f) ? 0.0f : (q > qmax ? qmax : q));
                c[k] = (uint32_t)k == axis ? (d[k] > 0.0f ? 0 : ext[k] - 1) : ck;
            }
            int cx = c[0], cy = c[1], cz = c[2];
            // per axis: the step in cells and in voxels of the stamp's arrays, and which of the cell's two planes the ray leaves by
            const int dcx = d[0] > 0.0f ? 1 : -1, dcy = d[1] > 0.0f ? 1 : -1, dcz = d[2] > 0.0f ? 1 : -1;
            const int ox = d[0] > 0.0f ? 1 : 0, oy = d[1] > 0.0f ? 1 : 0, oz = d[2] > 0.0f ? 1 : 0;
            const bool gx = d[0] != 0.0f, gy = d[1] != 0.0f, gz = d[2] != 0.0f;
            int voxel = (int)bcast(w1.x, j) + sx * cx + sy * cy + sz * cz;
            float t = t_in;
            bool found = false;
            for (int n = ex + ey + ez; n > 0; n--) {   // (every step moves one coordinate the ray's way: at most E'x + E'y + E'z)
                if (state[voxel] == RT_STAMP_SOLID) { found = true; break; }
                bool have = false;
                float tmin = 0.0f;
                uint32_t ax = 0u;
                if (gx) { tmin = (rtm_fma((float)(cx + ox), scale, lo[0]) - o[0]) * inv[0]; have = true; }
                if (gy) {
                    const float tk = (rtm_fma((float)(cy + oy), scale, lo[1]) - o[1]) * inv[1];
                    if (!have || tk < tmin) { tmin = tk; ax = 1u; have = true; }
                }
                if (gz) {
                    const float tk = (rtm_fma((float)(cz + oz), scale, lo[2]) - o[2]) * inv[2];
                    if (!have || tk < tmin) { tmin = tk; ax = 2u; have = true; }
                }
                if (!have) break;
                bool out;
                if (ax == 0u) { cx += dcx; voxel += dcx * sx; out = cx < 0 || cx >= ex; }
                else if (ax == 1u) { cy += dcy; voxel += dcy * sy; out = cy < 0 || cy >= ey; }
                else { cz += dcz; voxel += dcz * sz; out = cz < 0 || cz >= ez; }
                if (out) break;
                t = t < tmin ? tmin : t;
                axis = ax;
            }
            if (found && t < best_t) { best_t = t; best = first + (uint32_t)j; best_axis = axis; best_voxel = (uint32_t)voxel; }
        }
    }

    if (!inside || best == kNoModel) return;
    const vec3 P = v3(rtm_fma(d[0], best_t, o[0]), rtm_fma(d[1], best_t, o[1]), rtm_fma(d[2], best_t, o[2]));
    const float depth_f = vlength(vsub(v3(o[0], o[1], o[2]), P)) * 32.0f;    // store_primary_planes' expression
    if (!(depth_f < depth)) return;
    const float da = best_axis == 0u ? d[0] : (best_axis == 1u ? d[1] : d[2]);
    const uint32_t normal = 2u * best_axis + (da > 0.0f ? 1u : 0u);
    const uint4 r0 = a.recs[4u * (size_t)best];
    const uint32_t* mats = reinterpret_cast<const uint32_t*>((uint64_t)r0.x | ((uint64_t)r0.y << 32));
    const uint32_t material = mats[best_voxel], emission = a.recs[4u * (size_t)best + 3u].w;
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

hipError_t launch_draw_stamps(const Planes& pl, const DrawStampsArgs& a, hipStream_t st) {
    if (a.count == 0u || a.width <= 0 || a.height <= 0) return hipSuccess;
    const uint32_t tiles = (((uint32_t)a.width + 7u) / 8u) * (((uint32_t)a.height + 7u) / 8u);
    hipLaunchKernelGGL(k_draw_stamps, dim3((tiles + kStampsWg / 64u - 1u) / (kStampsWg / 64u)), dim3(kStampsWg), 0, st, pl, a);
    return hipGetLastError();
}

}  // namespace rtd
