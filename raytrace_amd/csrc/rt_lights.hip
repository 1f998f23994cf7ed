// rt_lights.hip — gfx950 kernel of rt_add_lights / rt_add_lights_async: point lights added to the two lighting planes of the frame drawn
// last, each through one hard shadow ray per (pixel, light) (include/rt_abi.h "Point lights"; the rules are restated, without a cull,
// in tests/point_light_ref.py).
//
//   k_add_lights : a tile pass (rt_tile_pass.hpp).  A lane rebuilds the surface point P' of its pixel from the depth and normal planes
//                  (surface_point); a tile without a surface pixel ends.  The wave reduces the per-axis bounds of its lanes' P'
//                  (tile_point_bounds).  Per batch of 64 lights lane l loads light base + l (two 16-byte loads), tests its validity and
//                  its sphere against the tile's bounds (light_may_reach_tile); for each candidate every lane runs the exact test with
//                  scalar light operands.  Lanes that pass step the shadow ray with the shared DDA of rt_dda.hpp (DIRECT: minefield
//                  bytes straight from the swizzled array, as k_query) and test between two steps whether the ray has reached the
//                  light.  No LDS, no atomics.
//
// All arithmetic that decides a pixel is fp32 with one rounding per operation (-ffp-contract=off).  The cull drops a light only where
// the exact test skips it at every pixel of the tile; it needs no margin (DESIGN.md "Point lights"): it repeats the exact test's own
// operations on operands that are no larger in magnitude, and every one of those operations is monotone.
#include <hip/hip_runtime.h>

#include "rt_dda.hpp"
#include "rt_tile_pass.hpp"

namespace rtd {

namespace {

constexpr float kLightMaxRadius = 1024.0f;
constexpr float kLightMaxColor = 1048576.0f;   // 2^20

// The contract's valid light (every comparison is false for a NaN).
__device__ __forceinline__ bool light_valid(uint4 w0, uint4 w1) {
    float p[3], c[3];
    rec_xyz(w0, p); rec_xyz(w1, c);
    const float radius = __uint_as_float(w0.w);
    bool ok = radius > 0.0f && radius <= kLightMaxRadius && w1.w == 0u;
    for (int k = 0; k < 3; k++) ok = ok && rtm_abs(p[k]) <= kPassMaxCoord && c[k] >= 0.0f && c[k] <= kLightMaxColor;
    return ok;
}

// Conservative: false only when the exact test skips the light at every pixel of the tile.  [lo, hi] bounds the finite P' of the tile's
// surface pixels (a pixel whose P' is not finite has dist2 = inf or NaN and is skipped by every light).  For such a pixel
// v_k = fl(pos_k - P'_k) and, rounding being monotone, v_k >= fl(pos_k - hi_k) and -v_k >= fl(lo_k - pos_k): |v_k| >= g_k, exactly.
// dist2 = fma(v_z, v_z, fma(v_y, v_y, fl(v_x v_x))) is monotone in each |v_k| (every partial sum is >= 0), so dist2 >= gap2 when gap2
// is the same expression of g — and r2 is the exact test's own fl(radius * radius).  The comparison is false for a NaN: it keeps the
// light.
__device__ __forceinline__ bool light_may_reach_tile(const float pos[3], float radius, const float lo[3], const float hi[3]) {
    rtm_vec3 g;
    g.x = rtm_max(rtm_max(pos[0] - hi[0], lo[0] - pos[0]), 0.0f);
    g.y = rtm_max(rtm_max(pos[1] - hi[1], lo[1] - pos[1]), 0.0f);
    g.z = rtm_max(rtm_max(pos[2] - hi[2], lo[2] - pos[2]), 0.0f);
    const float gap2 = rtm_dot3(g, g), r2 = radius * radius;
    return !(gap2 >= r2);
}

template <int LOGR, bool LRZ>
__global__ __launch_bounds__(kTileWg) void k_add_lights(Scene sc, Frame f, Planes pl, LightsArgs a) {
    constexpr int R = 1 << LOGR, LB = LOGR - 2;
    constexpr float half = (float)(R / 2);
    const TileLane tl(f.width, f.height);
    if (!tl.live) return;
    const size_t pix = tl.pix;

    const uint32_t normal = tl.inside ? (uint32_t)pl.normal_r8[pix] : 255u;
    const float depth = tl.inside ? pl.depth_f32[pix] : 65535.0f;
    const bool surface = normal < 6u && depth < 65535.0f;   // (false for a NaN depth)
    if (__ballot(surface) == 0ull) return;

    // ---- the surface point P' of this lane's pixel and the tile's bounds of it, the same in every lane ----
    float P[3], lo[3], hi[3];
    surface_point(f, tl.px, tl.py, depth, normal, P);
    tile_point_bounds(surface, P, lo, hi);
    const uint32_t axis = (normal >> 1) & 3u;
    const bool even = (normal & 1u) == 0u;

    // the first texel of every shadow ray of this pixel (trace_ray's fetch at its origin)
    int ix, iy, iz;
    const bool ok0 = wrap_texel(v3(P[0], P[1], P[2]), (float)R, &ix, &iy, &iz);
    const uint32_t vox0 = swizzled_index(ix, iy, iz, LB);

    float add[3] = {0.0f, 0.0f, 0.0f};
    bool lit = false;
    for (uint32_t base = 0; base < a.count; base += 64u) {
        const uint32_t mine = base + tl.lane;
        uint4 w0 = make_uint4(0u, 0u, 0u, 0u), w1 = w0;
        bool keep = false;
        if (mine < a.count) {
            w0 = a.lights[2u * (size_t)mine];
            w1 = a.lights[2u * (size_t)mine + 1u];
            float pos[3];
            rec_xyz(w0, pos);
            keep = light_valid(w0, w1) && light_may_reach_tile(pos, __uint_as_float(w0.w), lo, hi);
        }
        unsigned long long cand = __ballot(keep);
        while (cand) {
            const int j = __builtin_ctzll(cand);
            cand &= cand - 1ull;
            float pos[3], col[3];
            rec_xyz(w0, j, pos); rec_xyz(w1, j, col);
            const float radius = __uint_as_float(bcast(w0.w, j));
            // the exact test of this lane's pixel
            const float v[3] = {pos[0] - P[0], pos[1] - P[1], pos[2] - P[2]};
            const float dist2 = rtm_dot3({v[0], v[1], v[2]}, {v[0], v[1], v[2]});
            const float r2 = radius * radius;
            const float va = axis == 0u ? v[0] : (axis == 1u ? v[1] : v[2]);
            const float c = even ? va : -va;
            if (!(surface && dist2 > 0.0f && dist2 < r2 && c > 0.0f)) continue;
            // the shadow ray: trace_ray from P' towards the light, ended as visible once it is as far from P' as the light
            const vec3 d = vnormalize(v3(v[0], v[1], v[2]));
            RaySlot2 r;
            r.lx = 1.0f / rtm_abs(d.x); r.ly = 1.0f / rtm_abs(d.y); r.lz = 1.0f / rtm_abs(d.z);
            unsigned long long unused = 0;
            dda_arm<LOGR, LRZ, false, true, false>(r, d.x, d.y, d.z, P[0], P[1], P[2], ok0, vox0, 0u, f, half, nullptr, sc, unused, nullptr);
            bool reached = false;
            while (r.tracing) {
                const float ex = r.px - P[0], ey = r.py - P[1], ez = r.pz - P[2];
                if (rtm_dot3({ex, ey, ez}, {ex, ey, ez}) >= dist2) { reached = true; break; }
                dda_advance<LOGR, LRZ, false, false, false>(r, (uint32_t)sc.mine[r.vox], f, half, unused, nullptr);
            }
            if (!(reached || r2_kind(r) == PX_AIR)) continue;
            const float len = rtm_sqrt(dist2);
            const float cosine = c / len;
            const float x = 1.0f - dist2 / r2;
            const float w = (cosine * (x * x)) / (1.0f + dist2);
            for (int k = 0; k < 3; k++) add[k] = add[k] + col[k] * w;
            lit = true;
        }
    }

    if (!lit) return;
    const float s[3] = {add[0] / 16.0f, add[1] / 16.0f, add[2] / 16.0f};
    float4* lf = reinterpret_cast<float4*>(pl.lighting_f32) + pix;
    float4 lv = *lf;
    lv.x += s[0]; lv.y += s[1]; lv.z += s[2];
    *lf = lv;
    ushort4* lq = reinterpret_cast<ushort4*>(pl.lighting_rgba16) + pix;
    ushort4 q = *lq;
    q.x = (uint16_t)rtm_unorm((float)q.x / 65535.0f + s[0], 65535.0f);
    q.y = (uint16_t)rtm_unorm((float)q.y / 65535.0f + s[1], 65535.0f);
    q.z = (uint16_t)rtm_unorm((float)q.z / 65535.0f + s[2], 65535.0f);
    *lq = q;
}

}  // namespace

hipError_t launch_add_lights(const Scene& sc, const Frame& f, const Planes& pl, const LightsArgs& a, hipStream_t st) {
    if (f.logr < 8 || f.logr > 10) return hipErrorInvalidValue;
    if (a.count == 0u || f.width <= 0 || f.height <= 0) return hipSuccess;
    const dim3 grid = TileLane::grid(f.width, f.height), block(kTileWg);
    launch_for_region(f, [&](auto L, auto Z) { hipLaunchKernelGGL((k_add_lights<decltype(L)::value, decltype(Z)::value>), grid, block, 0, st, sc, f, pl, a); });
    return hipGetLastError();
}

}  // namespace rtd
