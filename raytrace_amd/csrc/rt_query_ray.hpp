// rt_query_ray.hpp — one query ray of rt_query.hip (k_query) and rt_entity_query.hip (k_entity_query): where ray i of a call comes
// from (q_ray), the head of trace_ray (q_arm) and the RtRayHit of an ended ray (q_finish).  Between q_arm and q_finish the ray is
// stepped with dda_advance<LOGR, LRZ, false, false, false> on sc.mine[r.vox], as k_frame steps its rays.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_dda.hpp"
#include "rt_kernels.hpp"

namespace rtd {
namespace {

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

}  // namespace
}  // namespace rtd
