// rt_boxes.hip — gfx950 kernel of rt_draw_boxes / rt_draw_boxes_async: world-space axis-aligned boxes composited into the planes of
// the frame drawn last, by depth (include/rt_abi.h "Entity boxes"; the rules are restated, without a cull, in tests/draw_boxes_ref.py).
//
//   k_draw_boxes : a tile pass (rt_tile_pass.hpp).  Per batch of 64 boxes lane l loads box base + l (two 16-byte loads), tests its
//                  validity and runs a conservative interval slab test against the tile (box_may_touch_tile); for each candidate
//                  every lane runs the exact slab test of its own ray with scalar box operands.  A lane keeps (t_in, index, axis) of
//                  its best box; winners compute the hit point, compare depths, gather their face light (16 bytes) and store seven
//                  planes.  No LDS, no atomics; the only cross-lane traffic is the ballot, the readlanes and one max reduction of
//                  the tile's depths.
#include <hip/hip_runtime.h>

#include "rt_tile_pass.hpp"

namespace rtd {

namespace {

__global__ __launch_bounds__(kTileWg) void k_draw_boxes(Planes pl, DrawBoxesArgs a) {
    const TileLane tl(a.width, a.height);
    if (!tl.live) return;
    const size_t pix = tl.pix;

    const float o[3] = {a.origin[0], a.origin[1], a.origin[2]};
    float d[3], inv[3];
    primary_dir(a, tl.px, tl.py, d, inv);
    const float depth = tl.inside ? pl.depth_f32[pix] : -INFINITY;

    // ---- what the cull knows of the tile (the same in every lane) ----
    const float omax = rtm_max(rtm_max(rtm_abs(o[0]), rtm_abs(o[1])), rtm_abs(o[2]));
    const TileDirs td = tile_dirs(a, tl.px0, tl.py0, omax);
    const float tile_depth = wave_max(depth);   // the largest depth_f32 of the tile's pixels (a NaN pixel is never drawn)

    float best_t = INFINITY;
    uint32_t best = kNoRecord, best_axis = 0u;
    for (uint32_t base = 0; base < a.count; base += 64u) {
        const uint32_t mine = base + tl.lane;
        uint4 w0 = make_uint4(0u, 0u, 0u, 0u), w1 = w0;
        bool keep = false;
        if (mine < a.count) {
            w0 = a.boxes[2u * (size_t)mine];
            w1 = a.boxes[2u * (size_t)mine + 1u];
            float lo[3], hi[3];
            rec_xyz(w0, lo); rec_xyz(w1, hi);
            keep = box_valid(lo, hi) && box_may_touch_tile(lo, hi, o, td, omax, tile_depth);
        }
        unsigned long long cand = __ballot(keep);
        while (cand) {
            const int j = __builtin_ctzll(cand);
            cand &= cand - 1ull;
            float lo[3], hi[3];
            rec_xyz(w0, j, lo); rec_xyz(w1, j, hi);
            // the exact slab test of this lane's ray
            float t_in, t_out;
            uint32_t axis;
            const bool hit = ray_box_slab(lo, hi, o, d, inv, &t_in, &t_out, &axis);
            if (hit && t_in < best_t) { best_t = t_in; best = base + (uint32_t)j; best_axis = axis; }
        }
    }

    if (!tl.inside || best == kNoRecord) return;
    float depth_f;
    uint32_t normal;
    if (!entity_hit_shows(o, d, best_t, best_axis, depth, &depth_f, &normal)) return;
    const uint32_t material = a.boxes[2u * (size_t)best].w, emission = a.boxes[2u * (size_t)best + 1u].w;
    store_entity_pixel(pl, pix, depth_f, normal, material, emission, a.lights[6u * (size_t)best + normal]);
}

}  // namespace

hipError_t launch_draw_boxes(const Planes& pl, const DrawBoxesArgs& a, hipStream_t st) {
    if (a.count == 0u || a.width <= 0 || a.height <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_draw_boxes, TileLane::grid(a.width, a.height), dim3(kTileWg), 0, st, pl, a);
    return hipGetLastError();
}

}  // namespace rtd
