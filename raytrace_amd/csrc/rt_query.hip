// rt_query.hip — gfx950 kernel of rt_trace_rays / rt_trace_rays_async / rt_pick_pixels: trace_ray (raytrace.comp:82-183) on rays
// the host hands over, with every field of HitResult plus the fetched texel, the iteration count and the border fetches.
//
//   k_query : one lane per ray, minefield bytes straight from the swizzled array (no LDS fill), the ray stepped with the shared DDA
//             of rt_dda.hpp (dda_arm / dda_advance with DIRECT = true, as k_frame steps its rays) and finished in q_finish.
//
// One kernel for every batch size: a persistent kernel with the nibble map in LDS and several rays per lane was measured slower at
// every size up to 16 M rays (DESIGN.md "Ray queries"), so it does not ship.
#include <hip/hip_runtime.h>

#include "rt_dda.hpp"
#include "rt_kernels.hpp"

namespace rtd {

namespace {

constexpr uint32_t kQueryWg = 256;

// ray i of the call: an RtRay (two 16-byte loads), or the primary ray of pixel xy[i] (raytrace.comp:296-297,306-315)
__device__ __forceinline__ void q_ray(const QueryArgs& a, const Frame& f, uint32_t i, vec3* o, vec3* d) {
    if (a.xy) {
        const int2 p = a.xy[i];
        primary_ray(f, p.x, p.y, o, d);
    } else {
        const float4 r0 = a.rays[2u * i], r1 = a.rays[2u * i + 1u];
        *o = v3(r0.x, r0.y, r0.z);
        *d = v3(r1.x, r1.y, r1.z);
    }
}

// Head of trace_ray (:83-107): normalize (:83), 1/|d| (:88), the first texel, then dda_arm.
template <int LOGR, bool LRZ>
__device__ __forceinline__ void q_arm(RaySlot2& r, vec3 o, vec3 dir, const Frame& f, const Scene& sc) {
    constexpr int R = 1 << LOGR, LB = LOGR - 2;
    const vec3 d = vnormalize(dir);
    r.lx = 1.0f / rtm_abs(d.x); r.ly = 1.0f / rtm_abs(d.y); r.lz = 1.0f / rtm_abs(d.z);
    int ix, iy, iz;
    const bool ok = wrap_texel(o, (float)R, &ix, &iy, &iz);
    unsigned long long unused = 0;
    dda_arm<LOGR, LRZ, false, true, false>(r, d.x, d.y, d.z, o.x, o.y, o.z, ok, swizzled_index(ix, iy, iz, LB), 0u, f, (float)(R / 2),
                                           nullptr, sc, unused, nullptr);
}

// The RtRayHit of an ended ray (48 bytes, three 16-byte stores).  `o` is the ray's origin as trace_ray received it.
template <int LOGR, bool LRZ>
__device__ __forceinline__ void q_finish(const RaySlot2& r, vec3 o, const Scene& sc, uint4* out) {
    constexpr int R = 1 << LOGR, LB = LOGR - 2;
    const uint32_t kind = r2_kind(r);
    const uint32_t nrm = r.axis == 0 ? (r.ndx < 0.0f ? 1u : 0u) : (r.axis == 1 ? (r.ndy < 0.0f ? 3u : 2u) : (r.ndz < 0.0f ? 5u : 4u));
    vec3 p = v3(r.px, r.py, r.pz);
    if (kind == PX_SPECIAL) p = v3(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));   // it never moved: mod(x, 0) (Q12)
    const float distance = vlength(vsub(o, p));                                                     // :164
    uint32_t material = 0, tx = 0xFFFFFFFFu, ty = 0xFFFFFFFFu, tz = 0xFFFFFFFFu;
    if (kind == PX_HIT && (LRZ || r.valid)) {
        // the hit texel is the texel of the last fetch (:150-154); its linear coordinates from the swizzled index
        material = sc.mat[r.vox];
        const uint32_t brick = r.vox >> 6, m = (1u << LB) - 1u;
        tx = ((brick & m) << 2) | (r.vox & 3u);
        ty = (((brick >> LB) & m) << 2) | ((r.vox >> 2) & 3u);
        tz = ((brick >> (2 * LB)) << 2) | ((r.vox >> 4) & 3u);
    }
    // border fetches (Q7): the fetch before the sky test of an air exit, the never-moved ray's fetches, a scrolled region's mid-ray
    // fetch outside the texture (it ends the ray as a hit on the border value)
    uint32_t border = r.fresh_invalid ? 1u : 0u;
    if (kind == PX_AIR) {
        int bx, by, bz;
        if (!wrap_texel(p, (float)R, &bx, &by, &bz)) border++;
    } else if (kind == PX_SPECIAL) {
        border++;
    } else if (!LRZ && kind == PX_HIT && !r.valid) {
        border++;
    }
    const float off = 0.001f;                                                                       // :166-180
    if (nrm == 0) p.x += off; else if (nrm == 1) p.x -= off;
    else if (nrm == 2) p.y += off; else if (nrm == 3) p.y -= off;
    else if (nrm == 4) p.z += off; else p.z -= off;
    const uint32_t hk = kind == PX_AIR ? (uint32_t)RT_HIT_AIR : (kind == PX_LIMIT ? (uint32_t)RT_HIT_LIMIT : (uint32_t)RT_HIT_SOLID);
    out[0] = make_uint4(__float_as_uint(p.x), __float_as_uint(p.y), __float_as_uint(p.z), __float_as_uint(distance));
    out[1] = make_uint4(tx, ty, tz, material);
    out[2] = make_uint4(nrm, hk, r.nk & 0xFFFFu, border);
}

template <int LOGR, bool LRZ>
__global__ __launch_bounds__(kQueryWg) void k_query(Scene sc, Frame f, QueryArgs a) {
    const uint32_t i = blockIdx.x * kQueryWg + threadIdx.x;
    if (i >= a.count) return;
    constexpr float half = (float)((1 << LOGR) / 2);
    vec3 o, d;
    q_ray(a, f, i, &o, &d);
    RaySlot2 r;
    q_arm<LOGR, LRZ>(r, o, d, f, sc);
    unsigned long long unused = 0;
    while (r.tracing) dda_advance<LOGR, LRZ, false, false, false>(r, (uint32_t)sc.mine[r.vox], f, half, unused, nullptr);
    q_finish<LOGR, LRZ>(r, o, sc, a.hits + 3u * i);
}

}  // namespace

hipError_t launch_query(const Scene& sc, const Frame& f, const QueryArgs& a, hipStream_t st) {
    if (f.logr < 8 || f.logr > 10) return hipErrorInvalidValue;
    if (a.count == 0u) return hipSuccess;
    const dim3 grid((a.count + kQueryWg - 1u) / kQueryWg), block(kQueryWg);
    launch_for_region(f, [&](auto L, auto Z) { hipLaunchKernelGGL((k_query<decltype(L)::value, decltype(Z)::value>), grid, block, 0, st, sc, f, a); });
    return hipGetLastError();
}

}  // namespace rtd
