// rt_sweep.hip — gfx950 kernel of rt_sweep_boxes / rt_sweep_boxes_async: an axis-aligned box moved through the resident region
// until it meets an occupied voxel (include/rt_abi.h "Box sweeps"; the rules are restated in tests/sweep_ref.py).
//
//   k_sweep : one lane per sweep, minefield bytes straight from the swizzled array as k_query fetches them (no LDS).  The record is
//             three 16-byte loads, the hit four 16-byte stores.  The events (a face of the box crossing an integer plane) are not
//             listed or sorted: per axis one pending trailing and one pending leading plane with its time live in registers, the
//             lane takes the earliest of the six by the contract's order and advances that sequence by one plane.  Every index
//             into the per-axis state is a compile-time constant after unrolling, so nothing goes to scratch.
//
// All float arithmetic is fp32 with one rounding per operation (-ffp-contract=off); once an event's time is known the rest is
// integers.  The minefield's distance values are not used to skip fetches inside a layer: rt_upload_world accepts worlds whose
// values bound no distance (any 0..30), and there a skip would change results.
#include <hip/hip_runtime.h>

#include "rt_kernels.hpp"

namespace rtd {

namespace {

constexpr uint32_t kSweepWg = 256;
constexpr float kSweepMaxCoord = 4194304.0f;   // 2^22
constexpr float kSweepMaxExtent = 8.0f;
constexpr float kSweepMaxMotion = 64.0f;
constexpr float kSweepNever = 2.0f;            // time of a sequence that has no event: only t < 1 exists
constexpr int kSweepMaxEvents = 512;           // above 3 x (65 leading + 73 trailing): the times of a sequence never decrease

// The first occupied voxel of the closed ranges in ascending (z, y, x) order.  A voxel outside the window lr - R/2 .. lr + R/2 is air;
// inside it the texel is (v + R/2) mod R per axis, always inside the arrays.
template <int LOGR>
__device__ __forceinline__ bool sweep_scan(const Scene& sc, const SweepArgs& a, int x0, int x1, int y0, int y1, int z0, int z1, uint32_t* vox) {
    constexpr uint32_t R = 1u << LOGR, H = R / 2u, M = R - 1u;
    for (int z = z0; z <= z1; z++) {
        if ((uint32_t)z - (uint32_t)a.lr[2] + H >= R) continue;
        for (int y = y0; y <= y1; y++) {
            if ((uint32_t)y - (uint32_t)a.lr[1] + H >= R) continue;
            for (int x = x0; x <= x1; x++) {
                if ((uint32_t)x - (uint32_t)a.lr[0] + H >= R) continue;
                const uint32_t v = swizzled_index((int)(((uint32_t)x + H) & M), (int)(((uint32_t)y + H) & M), (int)(((uint32_t)z + H) & M), LOGR - 2);
                if (sc.mine[v] == 0) { *vox = v; return true; }
            }
        }
    }
    return false;
}

__device__ __forceinline__ float sweep_time(int g, float face, float m) { return ((float)g - face) / m; }
__device__ __forceinline__ float clamp_lo(float x, int c) { const float f = (float)c; return x < f ? f : x; }
__device__ __forceinline__ float clamp_hi(float x, int c) { const float f = (float)c; return x > f ? f : x; }

template <int LOGR>
__global__ __launch_bounds__(kSweepWg) void k_sweep(Scene sc, SweepArgs a) {
    const uint32_t i = blockIdx.x * kSweepWg + threadIdx.x;
    if (i >= a.count) return;
    const uint4 r0 = a.sweeps[3u * i], r1 = a.sweeps[3u * i + 1u], r2 = a.sweeps[3u * i + 2u];
    const float lo[3] = {__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z)};
    const float hi[3] = {__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z)};
    const float m[3] = {__uint_as_float(r2.x), __uint_as_float(r2.y), __uint_as_float(r2.z)};
    uint4* out = a.hits + 4u * (size_t)i;

    // what the hit holds unless an event says otherwise
    float t = 0.0f;
    uint32_t kind = RT_SWEEP_INVALID, normal = 6u, axis = 3u, vox = 0u;
    bool found = false;
    float rl[3] = {lo[0], lo[1], lo[2]}, rh[3] = {hi[0], hi[1], hi[2]};

    bool ok = true;   // the validated domain (a NaN fails every comparison)
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float e = hi[k] - lo[k];
        ok = ok && __builtin_fabsf(lo[k]) <= kSweepMaxCoord && __builtin_fabsf(hi[k]) <= kSweepMaxCoord && __builtin_fabsf(m[k]) <= kSweepMaxMotion &&
             e > 0.0f && e <= kSweepMaxExtent;
    }
    if (ok) {
        int clo[3], chi[3];   // the cells of the box: closed integer ranges
#pragma unroll
        for (int k = 0; k < 3; k++) {
            clo[k] = (int)__builtin_floorf(lo[k]);
            chi[k] = (int)__builtin_ceilf(hi[k]) - 1;
        }
        if (sweep_scan<LOGR>(sc, a, clo[0], chi[0], clo[1], chi[1], clo[2], chi[2], &vox)) {
            kind = RT_SWEEP_EMBEDDED;
            found = true;
        } else {
            // per axis the pending trailing (T) and leading (L) plane and its time
            int gT[3], gL[3];
            float tT[3], tL[3], faceT[3], faceL[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const bool up = m[k] > 0.0f;
                gL[k] = up ? chi[k] + 1 : clo[k];
                gT[k] = up ? clo[k] + 1 : chi[k];
                faceL[k] = up ? hi[k] : lo[k];
                faceT[k] = up ? lo[k] : hi[k];
                const bool moves = m[k] != 0.0f;
                tL[k] = moves ? sweep_time(gL[k], faceL[k], m[k]) : kSweepNever;
                tT[k] = moves ? sweep_time(gT[k], faceT[k], m[k]) : kSweepNever;
            }
            kind = RT_SWEEP_FREE;
            t = 1.0f;
            int gb = 0;   // the plane a blocked sweep stopped at
            for (int n = 0; n < kSweepMaxEvents; n++) {
                // the earliest pending event: ascending t, trailing before leading, then x, y, z (a strict < keeps the first)
                int sel = -1;
                float bt = 1.0f;
#pragma unroll
                for (int k = 0; k < 3; k++) if (tT[k] < bt) { bt = tT[k]; sel = k; }
#pragma unroll
                for (int k = 0; k < 3; k++) if (tL[k] < bt) { bt = tL[k]; sel = 3 + k; }
                if (sel < 0) break;
                if (sel < 3) {
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        if (sel == k) {
                            const bool up = m[k] > 0.0f;
                            if (up) clo[k] = gT[k]; else chi[k] = gT[k] - 1;
                            gT[k] += up ? 1 : -1;
                            tT[k] = sweep_time(gT[k], faceT[k], m[k]);
                        }
                    }
                    continue;
                }
                const int ax = sel - 3;
                const int g = ax == 0 ? gL[0] : (ax == 1 ? gL[1] : gL[2]);
                const bool up = (ax == 0 ? m[0] : (ax == 1 ? m[1] : m[2])) > 0.0f;
                const int layer = up ? g : g - 1;
                if (sweep_scan<LOGR>(sc, a, ax == 0 ? layer : clo[0], ax == 0 ? layer : chi[0], ax == 1 ? layer : clo[1], ax == 1 ? layer : chi[1],
                                     ax == 2 ? layer : clo[2], ax == 2 ? layer : chi[2], &vox)) {
                    kind = RT_SWEEP_BLOCKED;
                    found = true;
                    t = bt;
                    axis = (uint32_t)ax;
                    normal = 2u * (uint32_t)ax + (up ? 1u : 0u);   // the code of a ray travelling the same way (raytrace.comp:89-93)
                    gb = g;
                    break;
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    if (ax == k) {
                        if (up) chi[k] = layer; else clo[k] = layer;
                        gL[k] += up ? 1 : -1;
                        tL[k] = sweep_time(gL[k], faceL[k], m[k]);
                    }
                }
            }
            // the returned box: the moved faces clamped to the cells found free; the blocked axis snapped to its plane
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (m[k] != 0.0f) {   // (an axis that does not move returns its input, bit for bit)
                    rl[k] = clamp_lo(lo[k] + m[k] * t, clo[k]);
                    rh[k] = clamp_hi(hi[k] + m[k] * t, chi[k] + 1);
                    if (axis == (uint32_t)k) {
                        const float size = hi[k] - lo[k];
                        if (m[k] > 0.0f) {
                            rh[k] = (float)gb;
                            rl[k] = clamp_lo((float)gb - size, clo[k]);
                        } else {
                            rl[k] = (float)gb;
                            rh[k] = clamp_hi((float)gb + size, chi[k] + 1);
                        }
                    }
                }
            }
        }
    }
    uint32_t material = 0u, tx = 0xFFFFFFFFu, ty = 0xFFFFFFFFu, tz = 0xFFFFFFFFu;
    if (found) {   // the texel from the swizzled index, as q_finish does
        constexpr int LB = LOGR - 2;
        material = sc.mat[vox];
        const uint32_t brick = vox >> 6, bm = (1u << LB) - 1u;
        tx = ((brick & bm) << 2) | (vox & 3u);
        ty = (((brick >> LB) & bm) << 2) | ((vox >> 2) & 3u);
        tz = ((brick >> (2 * LB)) << 2) | ((vox >> 4) & 3u);
    }
    out[0] = make_uint4(__float_as_uint(t), kind, normal, material);
    out[1] = make_uint4(tx, ty, tz, axis);
    out[2] = make_uint4(__float_as_uint(rl[0]), __float_as_uint(rl[1]), __float_as_uint(rl[2]), 0u);
    out[3] = make_uint4(__float_as_uint(rh[0]), __float_as_uint(rh[1]), __float_as_uint(rh[2]), 0u);
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
