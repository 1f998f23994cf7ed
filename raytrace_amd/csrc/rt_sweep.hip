// rt_sweep.hip — gfx950 kernel of rt_sweep_boxes / rt_sweep_boxes_async: an axis-aligned box moved through the resident region
// until it meets an occupied voxel (include/rt_abi.h "Box sweeps"; the rules are restated in tests/sweep_ref.py).
//
//   k_sweep : one lane per sweep.  The record is three 16-byte loads, the hit four 16-byte stores; between them the lane runs
//             sweep_box (rt_sweep_box.hpp: the one definition of the rules, which k_step_particles calls too) and looks up the
//             material and texel of the voxel it reports.  Nothing goes to scratch.
#include <hip/hip_runtime.h>

#include "rt_kernels.hpp"
#include "rt_sweep_box.hpp"

namespace rtd {

namespace {

constexpr uint32_t kSweepWg = 256;

template <int LOGR>
__global__ __launch_bounds__(kSweepWg) void k_sweep(Scene sc, SweepArgs a) {
    const uint32_t i = blockIdx.x * kSweepWg + threadIdx.x;
    if (i >= a.count) return;
    const uint4 r0 = a.sweeps[3u * i], r1 = a.sweeps[3u * i + 1u], r2 = a.sweeps[3u * i + 2u];
    const float lo[3] = {__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z)};
    const float hi[3] = {__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z)};
    const float m[3] = {__uint_as_float(r2.x), __uint_as_float(r2.y), __uint_as_float(r2.z)};
    uint4* out = a.hits + 4u * (size_t)i;

    SweepResult h;
    sweep_box<LOGR>(sc.mine, a.lr, lo, hi, m, h);
    uint32_t material = 0u, tx = 0xFFFFFFFFu, ty = 0xFFFFFFFFu, tz = 0xFFFFFFFFu;
    if (h.found) {   // the texel from the swizzled index, as q_finish does
        constexpr int LB = LOGR - 2;
        const uint32_t vox = h.vox;
        material = sc.mat[vox];
        const uint32_t brick = vox >> 6, bm = (1u << LB) - 1u;
        tx = ((brick & bm) << 2) | (vox & 3u);
        ty = (((brick >> LB) & bm) << 2) | ((vox >> 2) & 3u);
        tz = ((brick >> (2 * LB)) << 2) | ((vox >> 4) & 3u);
    }
    out[0] = make_uint4(__float_as_uint(h.t), h.kind, h.normal, material);
    out[1] = make_uint4(tx, ty, tz, h.axis);
    out[2] = make_uint4(__float_as_uint(h.lo[0]), __float_as_uint(h.lo[1]), __float_as_uint(h.lo[2]), 0u);
    out[3] = make_uint4(__float_as_uint(h.hi[0]), __float_as_uint(h.hi[1]), __float_as_uint(h.hi[2]), 0u);
}

}  // namespace

hipError_t launch_sweep(const Scene& sc, int logr, const SweepArgs& a, hipStream_t st) {
    if (logr < 8 || logr > 10) return hipErrorInvalidValue;
    if (a.count == 0u) return hipSuccess;
    const dim3 grid((a.count + kSweepWg - 1u) / kSweepWg), block(kSweepWg);
    if (logr == 8) hipLaunchKernelGGL((k_sweep<8>), grid, block, 0, st, sc, a);
    else if (logr == 9) hipLaunchKernelGGL((k_sweep<9>), grid, block, 0, st, sc, a);
    else hipLaunchKernelGGL((k_sweep<10>), grid, block, 0, st, sc, a);
    return hipGetLastError();
}

}  // namespace rtd
