// rt_model_walk.hpp — the walk of one ray through the cells of a voxel model, shared by rt_draw_stamps.hip (k_draw_stamps),
// rt_entity_query.hip (k_entity_query) and rt_shadows.hip (k_shadow_entities).  Device code only.  rt_lights.hip's
// k_add_lights_occluded walks the same way with a stop at the light, in a loop of its own: built on this one it measured slower
// than it was, twice (DESIGN.md "One model walk" has the figures).  A change to the arithmetic here is made there too.
//
// The arithmetic is the contract of include/rt_abi.h "Voxel-model entities", which the restatements under tests/ pin bit for bit:
// the first cell, the three plane times (written out per axis: a loop over the axes inside the step loop kept its operands in
// memory), the strict `<` that orders ties x, y, z, the step bound and the solid test.  It is fp32 with one rounding per operation
// (-ffp-contract=off).  What the kernels differ in is compiled in or out by two switches, so that none pays for another's state
// (DESIGN.md "One model walk" has the resource table).
#pragma once
#include "rt_tile_pass.hpp"

namespace rtd {
namespace {

// What a KEEP walk hands back on a hit: t and the axis the ray entered the solid cell by, the cell, and its index in the stamp's
// arrays.
struct WalkHit {
    float t;
    uint32_t axis;
    int voxel, cx, cy, cz;
};

// Does the ray (o, d, inv = 1.0f / d per component) meet a solid cell of model m, whose bounding box has its low corner at lo?
// t_in and axis are slab_core's for that box; the caller has checked that the ray crosses it.
//   INSIDE : the ray may start inside the box (t_in <= 0); its first cell is then the cell of o on every axis.  Without it the first
//            cell is the entry axis' first or last layer and, on the other axes, where the entry point lies.
//   KEEP   : carry t = max(t, tmin) and the axis through the steps and fill *h, which means something on a hit only (filled only
//            on a hit, k_draw_stamps and k_entity_query took 4 and 10 more VGPRs).  Without KEEP h is not touched and may be nullptr.
template <bool INSIDE, bool KEEP>
__device__ __forceinline__ bool walk_model(const ModelRec& m, const float lo[3], const float o[3], const float d[3], const float inv[3], float t_in,
                                           uint32_t axis, WalkHit* h) {
    const float scale = m.scale;
    const int ex = m.ext[0], ey = m.ext[1], ez = m.ext[2], sx = m.stride[0], sy = m.stride[1], sz = m.stride[2];
    const bool outside = !INSIDE || t_in > 0.0f;
    int c[3];
    for (int k = 0; k < 3; k++) {
        const float p = (!outside || d[k] == 0.0f) ? o[k] : rtm_fma(d[k], t_in, o[k]);
        const float q = rtm_floor((p - lo[k]) / scale), qmax = (float)(m.ext[k] - 1);   // clamped as a float: every index lies in the model
        const int ck = (int)(!(q > 0.0f) ? 0.0f : (q > qmax ? qmax : q));
        c[k] = (outside && (uint32_t)k == axis) ? (d[k] > 0.0f ? 0 : m.ext[k] - 1) : ck;
    }
    int cx = c[0], cy = c[1], cz = c[2];
    // per axis: the step in cells, which of the cell's two planes the ray leaves by, and whether it moves at all
    const int dcx = d[0] > 0.0f ? 1 : -1, dcy = d[1] > 0.0f ? 1 : -1, dcz = d[2] > 0.0f ? 1 : -1;
    const int ox = d[0] > 0.0f ? 1 : 0, oy = d[1] > 0.0f ? 1 : 0, oz = d[2] > 0.0f ? 1 : 0;
    const bool gx = d[0] != 0.0f, gy = d[1] != 0.0f, gz = d[2] != 0.0f;
    int voxel = m.base + sx * cx + sy * cy + sz * cz;
    float t = t_in;
    bool found = false;
    for (int n = ex + ey + ez; n > 0; n--) {   // (every step moves one coordinate the ray's way: at most E'x + E'y + E'z)
        if (m.state[voxel] == RT_STAMP_SOLID) { found = true; break; }
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
        if constexpr (KEEP) {
            t = t < tmin ? tmin : t;
            axis = ax;
        }
    }
    if constexpr (KEEP) { h->t = t; h->axis = axis; h->voxel = voxel; h->cx = cx; h->cy = cy; h->cz = cz; }
    return found;
}

}  // namespace
}  // namespace rtd
