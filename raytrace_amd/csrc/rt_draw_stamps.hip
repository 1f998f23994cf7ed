// rt_draw_stamps.hip — gfx950 kernel of rt_draw_stamps / rt_draw_stamps_async: voxel stamps placed as entities at float positions,
// scales and any of the 48 orientations, composited into the planes of the frame drawn last by depth (include/rt_abi.h "Voxel-model
// entities"; the rules are restated, without a cull, in tests/draw_stamps_ref.py).
//
//   k_draw_stamps : a tile pass (rt_tile_pass.hpp), k_draw_boxes' shape.  Per batch of 64 models lane l loads record base + l (four
//                   16-byte loads) and runs box_may_touch_tile on its bounding box; for each candidate every lane runs the exact slab
//                   test and then the voxel walk of its own ray with scalar model operands (walk_model, rt_model_walk.hpp).  The walk
//                   reads one state byte per cell from global memory (a model is a few KiB: the caches serve it) and keeps the cell's
//                   index in the stamp's arrays by adding a stride per step.  A lane keeps (t, model, axis, voxel) of its best hit;
//                   winners compute the hit point, compare depths, fetch the voxel's material word and the face light and store
//                   seven planes.  No LDS, no atomics.
//
// A model whose bounding box is entered no sooner than the lane's best hit so far is not walked: the walk only ever raises t above
// t_in, and on equal t the lower index wins.
#include <hip/hip_runtime.h>

#include "rt_model_walk.hpp"
#include "rt_tile_pass.hpp"

namespace rtd {

namespace {

__global__ __launch_bounds__(kTileWg) void k_draw_stamps(Planes pl, DrawStampsArgs a) {
    const TileLane tl(a.width, a.height);
    if (!tl.live) return;
    const size_t pix = tl.pix;

    const float o[3] = {a.origin[0], a.origin[1], a.origin[2]};
    float d[3], inv[3];
    primary_dir(a, tl.px, tl.py, d, inv);
    const float depth = tl.inside ? pl.depth_f32[pix] : -INFINITY;

    const float omax = rtm_max(rtm_max(rtm_abs(o[0]), rtm_abs(o[1])), rtm_abs(o[2]));
    TileDirs td = tile_dirs(a, tl.px0, tl.py0, omax);
    const float tile_depth = wave_max(depth);   // the largest depth_f32 of the tile's pixels (a NaN pixel is never drawn)

    float best_t = INFINITY;
    uint32_t best = kNoRecord, best_axis = 0u, best_voxel = 0u;
    for (uint32_t first = 0; first < a.count; first += 64u) {
        const uint32_t mine = first + tl.lane;
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
            float lo[3], hi[3];
            rec_xyz(w2, lo); rec_xyz(w3, hi);
            keep = box_may_touch_tile(lo, hi, o, td, omax, tile_depth);
        }
        unsigned long long cand = __ballot(keep);
        while (cand) {
            const int j = __builtin_ctzll(cand);
            cand &= cand - 1ull;
            float lo[3], hi[3];
            rec_xyz(w2, j, lo); rec_xyz(w3, j, hi);
            float t_in, t_out;
            uint32_t axis;
            const bool enters = ray_box_slab(lo, hi, o, d, inv, &t_in, &t_out, &axis);
            if (!(tl.inside && enters && t_in < best_t)) continue;   // (a lane past the frame's edge draws nothing)

            // the walk of this lane's ray through the model's cells: entered from outside, t and the axis kept
            WalkHit h;
            if (walk_model<false, true>(model_rec(w0, w1, w2, j), lo, o, d, inv, t_in, axis, &h) && h.t < best_t) {
                best_t = h.t; best = first + (uint32_t)j; best_axis = h.axis; best_voxel = (uint32_t)h.voxel;
            }
        }
    }

    if (!tl.inside || best == kNoRecord) return;
    float depth_f;
    uint32_t normal;
    if (!entity_hit_shows(o, d, best_t, best_axis, depth, &depth_f, &normal)) return;
    const uint4 r0 = a.recs[4u * (size_t)best];
    const uint32_t* mats = reinterpret_cast<const uint32_t*>((uint64_t)r0.x | ((uint64_t)r0.y << 32));
    const uint32_t material = mats[best_voxel], emission = a.recs[4u * (size_t)best + 3u].w;
    store_entity_pixel(pl, pix, depth_f, normal, material, emission, a.lights[6u * (size_t)best + normal]);
}

}  // namespace

hipError_t launch_draw_stamps(const Planes& pl, const DrawStampsArgs& a, hipStream_t st) {
    if (a.count == 0u || a.width <= 0 || a.height <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_draw_stamps, TileLane::grid(a.width, a.height), dim3(kTileWg), 0, st, pl, a);
    return hipGetLastError();
}

}  // namespace rtd
