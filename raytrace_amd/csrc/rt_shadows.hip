// rt_shadows.hip — gfx950 kernel of rt_shadow_entities / rt_shadow_entities_async: the entities the host drew (RtDrawBox records and
// voxel models) take the sun's direct term out of the two lighting planes of the frame drawn last, at the pixels they shade
// (include/rt_abi.h "Entity shadows"; the rules are restated, without a cull, in tests/entity_shadow_ref.py).
//
//   k_shadow_entities : a tile pass (rt_tile_pass.hpp), k_add_lights' shape.  A lane rebuilds the surface point P' of its pixel from
//                       the depth and normal planes (surface_point); a tile without a surface pixel ends.  The wave reduces the
//                       per-axis bounds of its lanes' P' (tile_point_bounds).  Boxes, then model records, are taken 64 at a time:
//                       lane l loads record base + l and tests it against the tile's bounds (sun_may_cross_tile); for each
//                       candidate every lane not yet shaded runs the exact slab test of its sun ray (slab_core) with scalar box
//                       operands — and, for a model, the walk of the model's cells.
//                       Shading is a boolean OR: a lane stops testing once it is shaded, the wave once every surface lane is.  Lanes
//                       shaded at the end step the world's sun ray with the shared DDA of rt_dda.hpp (DIRECT, as k_add_lights and
//                       k_query) and, where it leaves the window, subtract the sun term.  No LDS, no atomics.
//
// All arithmetic that decides a pixel is fp32 with one rounding per operation (-ffp-contract=off).  The cull drops an occluder only
// where the exact test fails at every pixel of the tile; it needs no margin (DESIGN.md "Entity shadows"): every ray of a tile has the
// same direction, so the cull repeats the exact test's own operations — a difference, a product with the one reciprocal — on
// operands that bound every pixel's, and each of those operations is monotone.
//
// The walk of a model's cells is the shared walk_model (rt_model_walk.hpp) with the switch for a start inside the box and without
// t and the axis; the sun's direction and reciprocals stay wave-uniform operands of it.
#include <hip/hip_runtime.h>

#include "rt_dda.hpp"
#include "rt_model_walk.hpp"
#include "rt_tile_pass.hpp"

namespace rtd {

namespace {

// What the kernel knows of the sun's direction, the same in every lane: per axis whether the direction is not zero there (slab_core's
// `nonzero`) and whether its reciprocal is a number the cull can multiply by (the reciprocal of a denormal is inf: such an axis
// bounds nothing in the cull).
struct SunDir {
    float s[3], inv[3];
    bool nonzero[3], use[3];
};

// Conservative: false only when the exact test below fails for every pixel of the tile whose P' lies in [blo, bhi].  For such a
// pixel and an axis with s_k > 0 the exact test has tn_k = fl(fl(lo_k - o_k) * inv_k) and tf_k = fl(fl(hi_k - o_k) * inv_k) (lo_k <=
// hi_k and inv_k > 0 order them); o_k <= bhi_k gives fl(lo_k - o_k) >= fl(lo_k - bhi_k), and the product with inv_k > 0 keeps the
// order: tn_k >= TN_k.  Likewise tf_k <= TF_k, and mirrored for s_k < 0.  t_in is no smaller than any tn_k, t_out no larger than any
// tf_k, so max TN >= min TF means t_in >= t_out and min TF <= 0 means t_out <= 0, at every pixel.  No product here is a NaN: the
// differences are finite and so is inv_k.
__device__ __forceinline__ bool sun_may_cross_tile(const float lo[3], const float hi[3], const SunDir& sd, const float blo[3], const float bhi[3]) {
    bool have = false;
    float tn_max = 0.0f, tf_min = 0.0f;
    for (int k = 0; k < 3; k++) {
        if (!sd.nonzero[k]) {
            if (hi[k] <= blo[k] || lo[k] >= bhi[k]) return false;   // no pixel has lo_k < o_k < hi_k
            continue;
        }
        if (!sd.use[k]) continue;
        const bool pos = sd.s[k] > 0.0f;
        const float tn = ((pos ? lo[k] : hi[k]) - (pos ? bhi[k] : blo[k])) * sd.inv[k];
        const float tf = ((pos ? hi[k] : lo[k]) - (pos ? blo[k] : bhi[k])) * sd.inv[k];
        if (!have) { tn_max = tn; tf_min = tf; have = true; }
        else { tn_max = tn > tn_max ? tn : tn_max; tf_min = tf < tf_min ? tf : tf_min; }
    }
    if (!have) return true;
    return !(tn_max >= tf_min || tf_min <= 0.0f);
}

template <int LOGR, bool LRZ>
__global__ __launch_bounds__(kTileWg) void k_shadow_entities(Scene sc, Frame f, Planes pl, ShadowArgs a) {
    constexpr int R = 1 << LOGR, LB = LOGR - 2;
    constexpr float half = (float)(R / 2);
    const TileLane tl(f.width, f.height);
    if (!tl.live) return;
    const uint32_t lane = tl.lane;
    const size_t pix = tl.pix;

    const uint32_t normal = tl.inside ? (uint32_t)pl.normal_r8[pix] : 255u;
    const float depth = tl.inside ? pl.depth_f32[pix] : 65535.0f;
    const bool surface = normal < 6u && depth < 65535.0f;   // (false for a NaN depth)
    if (__ballot(surface) == 0ull) return;

    // ---- the surface point P' of this lane's pixel and the tile's bounds of it, the same in every lane; a surface pixel whose P' is
    // not finite switches the cull off for its tile ----
    float P[3], blo[3], bhi[3];
    surface_point(f, tl.px, tl.py, depth, normal, P);
    const bool bounded = tile_point_bounds(surface, P, blo, bhi);
    const bool cull = __ballot(surface && !bounded) == 0ull;

    SunDir sd;
    for (int k = 0; k < 3; k++) {
        sd.s[k] = f.sunangle[k];
        sd.inv[k] = 1.0f / sd.s[k];
        sd.nonzero[k] = sd.s[k] != 0.0f;   // (the slab test's `d_k != 0`: a NaN direction takes the bounded branch)
        sd.use[k] = rtm_abs(sd.inv[k]) <= kFinite && (sd.s[k] > 0.0f || sd.s[k] < 0.0f);
    }

    bool need = surface;   // a surface pixel no occluder shades yet
    bool shaded = false;

    // ---- boxes ----
    for (uint32_t base = 0; base < a.nboxes && __ballot(need) != 0ull; base += 64u) {
        const uint32_t mine = base + lane;
        uint4 w0 = make_uint4(0u, 0u, 0u, 0u), w1 = w0;
        bool keep = false;
        if (mine < a.nboxes) {
            w0 = a.boxes[2u * (size_t)mine];
            w1 = a.boxes[2u * (size_t)mine + 1u];
            float lo[3], hi[3];
            rec_xyz(w0, lo); rec_xyz(w1, hi);
            keep = box_valid(lo, hi) && (!cull || sun_may_cross_tile(lo, hi, sd, blo, bhi));
        }
        unsigned long long cand = __ballot(keep);
        while (cand) {
            const int j = __builtin_ctzll(cand);
            cand &= cand - 1ull;
            float lo[3], hi[3];
            rec_xyz(w0, j, lo); rec_xyz(w1, j, hi);
            float t_in, t_out;
            uint32_t axis;
            const bool crosses = slab_core(lo, hi, P, sd.nonzero, sd.inv, &t_in, &t_out, &axis);
            if (need && crosses && t_out > 0.0f && t_in < t_out) { shaded = true; need = false; }
            if (__ballot(need) == 0ull) break;
        }
    }

    // ---- models ----
    for (uint32_t first = 0; first < a.nmodels && __ballot(need) != 0ull; first += 64u) {
        const uint32_t mine = first + lane;
        uint4 w0 = make_uint4(0u, 0u, 0u, 0u), w1 = w0, w2 = w0, w3 = w0;
        bool keep = false;
        if (mine < a.nmodels) {
            w0 = a.recs[4u * (size_t)mine];
            w1 = a.recs[4u * (size_t)mine + 1u];
            w2 = a.recs[4u * (size_t)mine + 2u];
            w3 = a.recs[4u * (size_t)mine + 3u];
            float lo[3], hi[3];
            rec_xyz(w2, lo); rec_xyz(w3, hi);
            keep = !cull || sun_may_cross_tile(lo, hi, sd, blo, bhi);
        }
        unsigned long long cand = __ballot(keep);
        while (cand) {
            const int j = __builtin_ctzll(cand);
            cand &= cand - 1ull;
            float lo[3], hi[3];
            rec_xyz(w2, j, lo); rec_xyz(w3, j, hi);
            float t_in, t_out;
            uint32_t axis;
            const bool crosses = slab_core(lo, hi, P, sd.nonzero, sd.inv, &t_in, &t_out, &axis);
            if (need && crosses && t_out > 0.0f && t_in < t_out) {
                // the walk of this lane's sun ray through the model's cells: P' may lie inside the box, and only the verdict is kept
                if (walk_model<true, false>(model_rec(w0, w1, w2, j), lo, P, sd.s, sd.inv, t_in, axis, nullptr)) { shaded = true; need = false; }
            }
            if (__ballot(need) == 0ull) break;
        }
    }

    if (!shaded) return;
    // ---- the world's sun ray: trace_ray from P' along s; only a ray that leaves the window had a sun term to remove ----
    {
        const vec3 d = vnormalize(ld3(f.sunangle));
        int ix, iy, iz;
        const bool ok0 = wrap_texel(v3(P[0], P[1], P[2]), (float)R, &ix, &iy, &iz);
        RaySlot2 r;
        r.lx = 1.0f / rtm_abs(d.x); r.ly = 1.0f / rtm_abs(d.y); r.lz = 1.0f / rtm_abs(d.z);
        unsigned long long unused = 0;
        dda_arm<LOGR, LRZ, false, true, false>(r, d.x, d.y, d.z, P[0], P[1], P[2], ok0, swizzled_index(ix, iy, iz, LB), 0u, f, half, nullptr, sc,
                                               unused, nullptr);
        while (r.tracing) dda_advance<LOGR, LRZ, false, false, false>(r, (uint32_t)sc.mine[r.vox], f, half, unused, nullptr);
        if (r2_kind(r) != PX_AIR) return;
    }
    const float sub[3] = {(f.sunlight[0] * a.strength) / 16.0f, (f.sunlight[1] * a.strength) / 16.0f, (f.sunlight[2] * a.strength) / 16.0f};
    float4* lf = reinterpret_cast<float4*>(pl.lighting_f32) + pix;
    float4 lv = *lf;
    lv.x = rtm_max(lv.x - sub[0], 0.0f); lv.y = rtm_max(lv.y - sub[1], 0.0f); lv.z = rtm_max(lv.z - sub[2], 0.0f);
    *lf = lv;
    ushort4* lq = reinterpret_cast<ushort4*>(pl.lighting_rgba16) + pix;
    ushort4 q = *lq;
    q.x = (uint16_t)rtm_unorm(rtm_max((float)q.x / 65535.0f - sub[0], 0.0f), 65535.0f);
    q.y = (uint16_t)rtm_unorm(rtm_max((float)q.y / 65535.0f - sub[1], 0.0f), 65535.0f);
    q.z = (uint16_t)rtm_unorm(rtm_max((float)q.z / 65535.0f - sub[2], 0.0f), 65535.0f);
    *lq = q;
}

}  // namespace

hipError_t launch_shadow_entities(const Scene& sc, const Frame& f, const Planes& pl, const ShadowArgs& a, hipStream_t st) {
    if (f.logr < 8 || f.logr > 10) return hipErrorInvalidValue;
    if ((a.nboxes == 0u && a.nmodels == 0u) || f.width <= 0 || f.height <= 0) return hipSuccess;
    const dim3 grid = TileLane::grid(f.width, f.height), block(kTileWg);
    launch_for_region(f, [&](auto L, auto Z) { hipLaunchKernelGGL((k_shadow_entities<decltype(L)::value, decltype(Z)::value>), grid, block, 0, st, sc, f, pl, a); });
    return hipGetLastError();
}

}  // namespace rtd
