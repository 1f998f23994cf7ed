// rt_query.hip — gfx950 kernel of rt_trace_rays / rt_trace_rays_async / rt_pick_pixels: trace_ray (raytrace.comp:82-183) on rays
// the host hands over, with every field of HitResult plus the fetched texel, the iteration count and the border fetches.
//
//   k_query : one lane per ray, minefield bytes straight from the swizzled array (no LDS fill), the ray stepped with the shared DDA
//             of rt_dda.hpp (dda_arm / dda_advance with DIRECT = true, as k_frame steps its rays) and finished in q_finish
//             (rt_query_ray.hpp, shared with rt_entity_query.hip).
//
// One kernel for every batch size: a persistent kernel with the nibble map in LDS and several rays per lane was measured slower at
// every size up to 16 M rays (DESIGN.md "Ray queries"), so it does not ship.
#include <hip/hip_runtime.h>

#include "rt_query_ray.hpp"

namespace rtd {

namespace {

constexpr uint32_t kQueryWg = 256;

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
