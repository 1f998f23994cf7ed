// rt_sweep_box.hpp — the one definition of the box-sweep rules (include/rt_abi.h "Box sweeps"; restated in tests/sweep_ref.py), shared
// by k_sweep (rt_sweep.hip: rt_sweep_boxes) and k_step_particles (rt_step_particles.hip: rt_step_particles).
//
//   sweep_box : the domain test, the embedded scan, the event loop and the returned box of one sweep, for one lane.  Minefield bytes
//               come straight from the swizzled array as k_query fetches them (no LDS).  The events (a face of the box crossing an
//               integer plane) are not listed or sorted: per axis one pending trailing and one pending leading plane with its time
//               live in registers, the lane takes the earliest of the six by the contract's order and advances that sequence by one
//               plane.  Every index into the per-axis state is a compile-time constant after unrolling, so nothing goes to scratch.
//
// All float arithmetic is fp32 with one rounding per operation (-ffp-contract=off); once an event's time is known the rest is
// integers.  The minefield's distance values are not used to skip fetches inside a layer: rt_upload_world accepts worlds whose
// values bound no distance (any 0..30), and there a skip would change results.
#pragma once

#include <hip/hip_runtime.h>

#include "rt_kernels.hpp"

namespace rtd {

constexpr float kSweepMaxCoord = 4194304.0f;   // 2^22
constexpr float kSweepMaxExtent = 8.0f;
constexpr float kSweepMaxMotion = 64.0f;
constexpr float kSweepNever = 2.0f;            // time of a sequence that has no event: only t < 1 exists
constexpr int kSweepMaxEvents = 512;           // above 3 x (65 leading + 73 trailing): the times of a sequence never decrease

// What one sweep found: RtSweepHit without the material and the texel, which the caller derives from `vox` where it reports them.
struct SweepResult {
    float t;
    uint32_t kind, normal, axis;   // RT_SWEEP_*; the face code, 6 = none; the blocked axis, 3 = none
    uint32_t vox;                  // the swizzled index of the blocking / embedding voxel when `found`
    bool found;
    float lo[3], hi[3];            // the box where the sweep ended
};

// The first occupied voxel of the closed ranges in ascending (z, y, x) order.  A voxel outside the window lr - R/2 .. lr + R/2 is air;
// inside it the texel is (v + R/2) mod R per axis, always inside the arrays.
template <int LOGR>
__device__ __forceinline__ bool sweep_scan(const uint8_t* mine, const int32_t (&lr)[3], int x0, int x1, int y0, int y1, int z0, int z1,
                                           uint32_t* vox) {
    constexpr uint32_t R = 1u << LOGR, H = R / 2u, M = R - 1u;
    for (int z = z0; z <= z1; z++) {
        if ((uint32_t)z - (uint32_t)lr[2] + H >= R) continue;
        for (int y = y0; y <= y1; y++) {
            if ((uint32_t)y - (uint32_t)lr[1] + H >= R) continue;
            for (int x = x0; x <= x1; x++) {
                if ((uint32_t)x - (uint32_t)lr[0] + H >= R) continue;
                const uint32_t v = swizzled_index((int)(((uint32_t)x + H) & M), (int)(((uint32_t)y + H) & M), (int)(((uint32_t)z + H) & M), LOGR - 2);
                if (mine[v] == 0) { *vox = v; return true; }
            }
        }
    }
    return false;
}

__device__ __forceinline__ float sweep_time(int g, float face, float m) { return ((float)g - face) / m; }
__device__ __forceinline__ float clamp_lo(float x, int c) { const float f = (float)c; return x < f ? f : x; }
__device__ __forceinline__ float clamp_hi(float x, int c) { const float f = (float)c; return x > f ? f : x; }

// The validated domain of a box (a NaN fails every comparison); the motion has its own bound.
__device__ __forceinline__ bool sweep_box_in_domain(const float (&lo)[3], const float (&hi)[3]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float e = hi[k] - lo[k];
        ok = ok && __builtin_fabsf(lo[k]) <= kSweepMaxCoord && __builtin_fabsf(hi[k]) <= kSweepMaxCoord && e > 0.0f && e <= kSweepMaxExtent;
    }
    return ok;
}

// One sweep of the box (lo, hi) by m through the window centred on lr.
template <int LOGR>
__device__ __forceinline__ void sweep_box(const uint8_t* mine, const int32_t (&lr)[3], const float (&box_lo)[3], const float (&box_hi)[3],
                                          const float (&motion)[3], SweepResult& r) {
    // (copies: arrays used through the references stay in memory until late in the compiler, which costs k_sweep registers)
    const float lo[3] = {box_lo[0], box_lo[1], box_lo[2]}, hi[3] = {box_hi[0], box_hi[1], box_hi[2]};
    const float m[3] = {motion[0], motion[1], motion[2]};
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
        if (sweep_scan<LOGR>(mine, lr, clo[0], chi[0], clo[1], chi[1], clo[2], chi[2], &vox)) {
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
                if (sweep_scan<LOGR>(mine, lr, ax == 0 ? layer : clo[0], ax == 0 ? layer : chi[0], ax == 1 ? layer : clo[1], ax == 1 ? layer : chi[1],
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
    r.t = t; r.kind = kind; r.normal = normal; r.axis = axis; r.vox = vox; r.found = found;
#pragma unroll
    for (int k = 0; k < 3; k++) { r.lo[k] = rl[k]; r.hi[k] = rh[k]; }
}

}  // namespace rtd
