// rt_entity_query.hip — gfx950 kernel of rt_trace_entities / rt_trace_entities_async / rt_pick_entities: what a ray or a pixel hits
// among the entities a host draws — RtDrawBox boxes and RtDrawStamp voxel models — under the draws' own rules, depth-tested against
// the world the same ray hits (include/rt_abi.h "Entity queries"; restated, without a cull, in tests/entity_query_ref.py).
//
//   k_entity_query : 256 threads, one lane per ray, no LDS, no atomics.
//     Phase 1: the lane traces the world exactly as k_query does (rt_query_ray.hpp) and stores the RtRayHit where the caller wants it.
//              D is the depth the world leaves for this ray: store_primary_planes' expression on the position as returned.
//     Phase 2: the batch idiom of the tile passes (rt_tile_pass.hpp) applied to a wave of rays.  A lane whose D is NaN or not
//              positive, or whose origin or direction is not finite, can report nothing and is done.  Every other lane's segment
//              o .. o + d * reach bounds where its reported hit can lie; the wave reduces the bounds of its live lanes' segments.
//              Per batch of 64 records lane l loads record base + l — the boxes first, then the models' 64-byte DrawStampRecords —
//              and tests the record's box against the wave's bounds; per keeper the record's words are broadcast and each live lane
//              runs the exact slab test (and, for a model, the draw's walk) of its own ray.  Winners run the depth test, fetch the
//              material word and store three 16-byte words.
//
// The cull may only drop a record that the exact rules reject, or that fails the depth test, for every live lane of the wave
// (DESIGN.md "Entity queries" carries the argument for its margins).  Coherent rays — a screen region's pixels, a volley — are culled
// well; incoherent rays in one wave are not, and the cost then tends to rays x entities slab tests.
//
// The walk is k_draw_stamps' (walk_model, rt_model_walk.hpp) with the lane's own origin; the record also reports the cell it ends on.
#include <hip/hip_runtime.h>

#include "rt_model_walk.hpp"
#include "rt_query_ray.hpp"
#include "rt_tile_pass.hpp"

namespace rtd {

namespace {

constexpr uint32_t kEntityQueryWg = 256;
// the cull's margins: the reach of a lane is its depth bound grown by 2^-5 relative (the hit point lies within D / 32 (1 + 2^-21) of o,
// and a sane direction's length within 2^-6 of 1); coordinates carry 2^-18 of their size on the ray's side and 2^-19 on the box's,
// and 1e-18 absolute where squares went denormal
constexpr float kReachRel = 1.03125f;
constexpr float kRayAbs = 1.0f / 262144.0f;
constexpr float kBoxAbs = 1.0f / 524288.0f;
constexpr float kTinyAbs = 1.0e-18f;

__device__ __forceinline__ bool finite3(const float v[3]) { return rtm_abs(v[0]) <= kFinite && rtm_abs(v[1]) <= kFinite && rtm_abs(v[2]) <= kFinite; }

// Conservative: false only when no live lane of the wave can report the record whose box is [lo, hi] — the box, grown by its
// margin, misses the wave's bounds [wlo, whi] on some axis.  (A NaN keeps the record.)
__device__ __forceinline__ bool box_may_touch_wave(const float lo[3], const float hi[3], const float wlo[3], const float whi[3]) {
    bool keep = true;
    for (int k = 0; k < 3; k++) {
        const float m = (rtm_abs(lo[k]) + rtm_abs(hi[k])) * kBoxAbs;
        if (hi[k] + m < wlo[k] || lo[k] - m > whi[k]) keep = false;
    }
    return keep;
}

template <int LOGR, bool LRZ>
__global__ __launch_bounds__(kEntityQueryWg) void k_entity_query(Scene sc, Frame f, EntityQueryArgs a) {
    const uint32_t i = blockIdx.x * kEntityQueryWg + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool mine = i < a.count;   // (a lane past the last ray stays for the wave's broadcasts and stores nothing)

    // ---- phase 1: the world, as k_query traces it; then the entity ray (o, d) and the depth D the world leaves ----
    float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f}, inv[3];
    float D = 0.0f;
    if (mine) {
        constexpr float half = (float)((1 << LOGR) / 2);
        QueryArgs q;
        q.rays = a.rays; q.xy = a.xy; q.hits = nullptr; q.count = a.count;
        vec3 wo, wd;
        q_ray(q, f, i, &wo, &wd);
        RaySlot2 r;
        q_arm<LOGR, LRZ>(r, wo, wd, f, sc);
        unsigned long long unused = 0;
        while (r.tracing) dda_advance<LOGR, LRZ, false, false, false>(r, (uint32_t)sc.mine[r.vox], f, half, unused, nullptr);
        uint4 wh[3];
        q_finish<LOGR, LRZ>(r, wo, sc, wh);
        if (a.world_hits) {
            uint4* out = a.world_hits + 3u * (size_t)i;
            out[0] = wh[0]; out[1] = wh[1]; out[2] = wh[2];
        }
        // a ray as given: its origin and its direction normalised once; a pixel: rt_draw_boxes' ray — u.origin, no slide, and the
        // direction primary_ray normalised
        vec3 dn = wd;
        if (a.xy) wo = ld3(f.origin); else dn = vnormalize(wd);
        o[0] = wo.x; o[1] = wo.y; o[2] = wo.z;
        d[0] = dn.x; d[1] = dn.y; d[2] = dn.z;
        const vec3 wp = v3(__uint_as_float(wh[0].x), __uint_as_float(wh[0].y), __uint_as_float(wh[0].z));
        D = wh[2].y == (uint32_t)RT_HIT_AIR ? 65535.0f : vlength(vsub(wo, wp)) * 32.0f;
    }
    for (int k = 0; k < 3; k++) inv[k] = 1.0f / d[k];

    // ---- phase 2: the wave's bounds ----
    // (a lane with a non-finite o or d reports nothing under the exact rules — DESIGN.md "Entity queries" — so it is done too)
    const bool live = mine && D > 0.0f && finite3(o) && finite3(d);
    float wlo[3], whi[3];
    {
        const float omax = rtm_max(rtm_max(rtm_abs(o[0]), rtm_abs(o[1])), rtm_abs(o[2]));
        const float reach = (D * (1.0f / 32.0f)) * kReachRel;
        const float len2 = rtm_fma(d[2], d[2], rtm_fma(d[1], d[1], d[0] * d[0]));
        const bool sane = len2 >= 0.97f && len2 <= 1.03f;   // (else the hit point is only known to lie within `reach` of o)
        const float grow = (omax + reach) * kRayAbs + kTinyAbs;
        for (int k = 0; k < 3; k++) {
            const float ext = (sane ? rtm_abs(d[k]) : 1.0f) * reach + grow;
            // the hit point's coordinate lies on the direction's side of o_k (fma rounds monotonically); without a trusted
            // direction, on either side
            float lo_k = (sane && d[k] >= 0.0f) ? o[k] - grow : o[k] - ext;
            float hi_k = (sane && d[k] <= 0.0f) ? o[k] + grow : o[k] + ext;
            if (!live) { lo_k = INFINITY; hi_k = -INFINITY; }
            for (int s = 32; s > 0; s >>= 1) {
                lo_k = fminf(lo_k, __shfl_xor(lo_k, s, 64));
                hi_k = fmaxf(hi_k, __shfl_xor(hi_k, s, 64));
            }
            wlo[k] = lo_k; whi[k] = hi_k;
        }
    }

    float best_t = INFINITY;
    uint32_t best = kNoRecord, best_axis = 0u, best_voxel = 0xFFFFFFFFu, best_cell = 0u;   // best: boxes 0 .., models nboxes ..
    // ---- the boxes (rt_boxes.hip's loop) ----
    for (uint32_t base = 0; base < a.nboxes; base += 64u) {
        const uint32_t rec = base + lane;
        uint4 w0 = make_uint4(0u, 0u, 0u, 0u), w1 = w0;
        bool keep = false;
        if (rec < a.nboxes) {
            w0 = a.boxes[2u * (size_t)rec];
            w1 = a.boxes[2u * (size_t)rec + 1u];
            float lo[3], hi[3];
            rec_xyz(w0, lo); rec_xyz(w1, hi);
            keep = box_valid(lo, hi) && box_may_touch_wave(lo, hi, wlo, whi);
        }
        unsigned long long cand = __ballot(keep);
        while (cand) {
            const int j = __builtin_ctzll(cand);
            cand &= cand - 1ull;
            float lo[3], hi[3];
            rec_xyz(w0, j, lo); rec_xyz(w1, j, hi);
            float t_in, t_out;
            uint32_t axis;
            const bool hit = ray_box_slab(lo, hi, o, d, inv, &t_in, &t_out, &axis);
            if (live && hit && t_in < best_t) { best_t = t_in; best = base + (uint32_t)j; best_axis = axis; }
        }
    }
    // ---- the models (rt_draw_stamps.hip's loop, the lane's own o) ----
    for (uint32_t first = 0; first < a.nmodels; first += 64u) {
        const uint32_t rec = first + lane;
        uint4 w0 = make_uint4(0u, 0u, 0u, 0u), w1 = w0, w2 = w0, w3 = w0;
        bool keep = false;
        if (rec < a.nmodels) {
            w0 = a.recs[4u * (size_t)rec];
            w1 = a.recs[4u * (size_t)rec + 1u];
            w2 = a.recs[4u * (size_t)rec + 2u];
            w3 = a.recs[4u * (size_t)rec + 3u];
            float lo[3], hi[3];
            rec_xyz(w2, lo); rec_xyz(w3, hi);
            keep = box_may_touch_wave(lo, hi, wlo, whi);
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
            // on equal t a box, or a model of a lower index, keeps the hit: the walk only ever raises t above t_in
            if (!(live && enters && t_in < best_t)) continue;

            WalkHit h;
            if (walk_model<false, true>(model_rec(w0, w1, w2, j), lo, o, d, inv, t_in, axis, &h) && h.t < best_t) {
                best_t = h.t; best = a.nboxes + first + (uint32_t)j; best_axis = h.axis; best_voxel = (uint32_t)h.voxel;
                best_cell = (uint32_t)h.cx | ((uint32_t)h.cy << 8) | ((uint32_t)h.cz << 16);   // (0 <= c_k < 256)
            }
        }
    }

    if (!mine) return;
    // ---- the depth test against the world and the record: every byte of it is written ----
    uint4 h0 = make_uint4(0u, 0u, 0u, 0u);
    uint4 h1 = make_uint4((uint32_t)RT_ENTITY_NONE, 0xFFFFFFFFu, 6u, 0u);
    uint4 h2 = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    if (best != kNoRecord) {
        float depth_f;
        uint32_t normal;
        if (entity_hit_shows(o, d, best_t, best_axis, D, &depth_f, &normal)) {   // the draws' own depth test and face code
            const vec3 P = v3(rtm_fma(d[0], best_t, o[0]), rtm_fma(d[1], best_t, o[1]), rtm_fma(d[2], best_t, o[2]));
            h0 = make_uint4(__float_as_uint(P.x), __float_as_uint(P.y), __float_as_uint(P.z), __float_as_uint(best_t));
            if (best < a.nboxes) {
                h1 = make_uint4((uint32_t)RT_ENTITY_BOX, best, normal, a.boxes[2u * (size_t)best].w);
            } else {
                const uint32_t mi = best - a.nboxes;
                const uint4 r0 = a.recs[4u * (size_t)mi];
                const uint32_t* mats = reinterpret_cast<const uint32_t*>((uint64_t)r0.x | ((uint64_t)r0.y << 32));
                h1 = make_uint4((uint32_t)RT_ENTITY_MODEL, mi, normal, mats[best_voxel]);
                h2 = make_uint4(best_cell & 0xFFu, (best_cell >> 8) & 0xFFu, (best_cell >> 16) & 0xFFu, best_voxel);
            }
        }
    }
    uint4* out = a.entity_hits + 3u * (size_t)i;
    out[0] = h0; out[1] = h1; out[2] = h2;
}

}  // namespace

hipError_t launch_entity_query(const Scene& sc, const Frame& f, const EntityQueryArgs& a, hipStream_t st) {
    if (f.logr < 8 || f.logr > 10) return hipErrorInvalidValue;
    if (a.count == 0u) return hipSuccess;
    const dim3 grid((a.count + kEntityQueryWg - 1u) / kEntityQueryWg), block(kEntityQueryWg);
    launch_for_region(f, [&](auto L, auto Z) {
        hipLaunchKernelGGL((k_entity_query<decltype(L)::value, decltype(Z)::value>), grid, block, 0, st, sc, f, a);
    });
    return hipGetLastError();
}

}  // namespace rtd
