// rt_temporal.hip — gfx950 kernel of RT_FLAG_REPROJECT: the pass that replaces k_accumulate_frame on one-sample whole-frame
// contexts and carries a pixel's lighting history across a camera change.
//
//   k_temporal_frame<MODE> : one lane per pixel, grid-stride over the row-major frame, no LDS.  The context owns two history sets
//                            used in turn; a launch reads `prev` and writes `next`.  Per pixel a set holds the fp32 sum of the
//                            lights (float4) and an 8-byte record: the frame's depth_f32 and count | normal << 27.
//     TEMPORAL_RESTART  sum = 0 + L, n = 1
//     TEMPORAL_STILL    sum = prev sum + L, n = prev n + 1: k_accumulate_frame's arithmetic plus the count word (a context whose
//                       camera never moves is bit-identical to RT_FLAG_ACCUMULATE alone)
//     TEMPORAL_MOVED    the pixel's hit point is rebuilt from its depth, projected into the previous camera, and the history of
//                       the nearest previous pixel is taken if it lies on the same voxel face plane (same normal, at most 0.25
//                       apart along the normal's axis: faces lie on integer planes, so 1.0 is the next possibility); otherwise
//                       the pixel restarts.  An accepted history of more than `cap` samples is scaled down to `cap`.
//     TEMPORAL_MOVED_BOXES  a moved frame after voxel edits (RtConfig.edit_radius > 0): once the hit point P is rebuilt, it is tested
//                       against every edited box (kernel arguments: wave-uniform scalar loads, no LDS) — within edit_radius of
//                       the box, or on a ray from P towards the sun that meets the box grown by 1 (edit_touches) — and a pixel
//                       that is near or shadowed restarts; every other pixel goes on exactly as in TEMPORAL_MOVED.
//     TEMPORAL_MOVED_SLABS  a moved frame after streamed slabs (RtConfig.stream_history): TEMPORAL_MOVED_BOXES' test against the frame's
//                       edit boxes (there may be none), then against the boxes k_place_slab_boxes (rt_slab.hip) wrote in front
//                       of this launch — their count and bounds are wave-uniform loads from device memory, same arithmetic.
//   L = 16 x lighting_f32 of the frame just drawn (exact); the lighting planes become store_lighting(sum, n).
//
// All fp32, every operation rounded on its own (-ffp-contract=off); only the two normalizes fuse, as primary_ray's does: the CPU
// restatement (tests/temporal_ref.py) reproduces the lighting planes and the counts bit for bit.
// Bytes per pixel, moved: 16 + 4 + 1 of the frame's planes, a gather of 8 (+ 16 when accepted) from the previous set, 16 + 8 to the
// new set, 16 + 8 of lighting.  Neighbouring pixels gather from neighbouring addresses under any smooth camera motion.
#include <hip/hip_runtime.h>

#include "rt_kernels.hpp"

namespace rtd {

namespace {

constexpr uint32_t kTemporalWg = 256;
constexpr uint32_t kCountMask = (1u << 27) - 1u;

__device__ __forceinline__ float dotp(vec3 a, vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// the direction primary_ray computes for pixel (px, py) under camera (fwd, right, up): its own expression, its own normalize
__device__ __forceinline__ vec3 pixel_dir(vec3 fwd, vec3 right, vec3 up, float px, float py, float w, float h) {
    const float sx = (px / w) * 2.0f - 1.0f;
    const float sy = (py / h) * 2.0f - 1.0f;
    return vnormalize(vadd(vadd(fwd, vscale(right, sx)), vscale(up, sy)));
}

__device__ __forceinline__ float axis_of(vec3 v, uint32_t k) { return k == 0u ? v.x : (k == 1u ? v.y : v.z); }

// one axis of edit_touches: the distance from p to [lo, hi], and the slab [lo - 1, hi + 1] cut out of the ray p + t s
// (s == 0, uniform over the launch: the ray stays inside the slab for every t, or misses the box)
__device__ __forceinline__ float edit_axis(float lo, float hi, float p, float s, float inv_s, float& tn, float& tf, bool& miss) {
    if (s != 0.0f) {
        const float ta = ((lo - 1.0f) - p) * inv_s, tb = ((hi + 1.0f) - p) * inv_s;
        tn = rtm_max(tn, rtm_min(ta, tb));
        tf = rtm_min(tf, rtm_max(ta, tb));
    } else if (!(lo - 1.0f <= p && p <= hi + 1.0f)) {
        miss = true;
    }
    return rtm_max(rtm_max(lo - p, p - hi), 0.0f);
}

// TEMPORAL_MOVED_BOXES: can an edit have changed the light that arrives at P?  For each box: near — the squared distance from P to
// the box is at most r2; shadowed — the ray from P along the sun vector meets the box grown by 1 on every side (the 1 covers the
// 0.001 face offset and the rounding of P) at some t > 0.
__device__ __forceinline__ bool edit_touches(const TemporalArgs& a, vec3 P) {
    bool touched = false;
    for (uint32_t b = 0; b < a.nbox; b++) {
        const TemporalBox& x = a.box[b];
        float tn = -__builtin_inff(), tf = __builtin_inff();
        bool miss = false;
        const float dx = edit_axis(x.lo[0], x.hi[0], P.x, a.sun[0], a.inv_sun[0], tn, tf, miss);
        const float dy = edit_axis(x.lo[1], x.hi[1], P.y, a.sun[1], a.inv_sun[1], tn, tf, miss);
        const float dz = edit_axis(x.lo[2], x.hi[2], P.z, a.sun[2], a.inv_sun[2], tn, tf, miss);
        const float dist2 = (dx * dx + dy * dy) + dz * dz;
        touched = touched || dist2 <= a.r2 || (!miss && tn <= tf && tf > 0.0f);
    }
    return touched;
}

// TEMPORAL_MOVED_SLABS: the same test against the boxes in device memory
__device__ __forceinline__ bool slab_touches(const TemporalArgs& a, vec3 P) {
    const SlabBoxes* __restrict__ s = a.slab;
    const uint32_t nbox = s->count;
    bool touched = false;
    for (uint32_t b = 0; b < nbox; b++) {
        const TemporalBox x = s->box[b];
        float tn = -__builtin_inff(), tf = __builtin_inff();
        bool miss = false;
        const float dx = edit_axis(x.lo[0], x.hi[0], P.x, a.sun[0], a.inv_sun[0], tn, tf, miss);
        const float dy = edit_axis(x.lo[1], x.hi[1], P.y, a.sun[1], a.inv_sun[1], tn, tf, miss);
        const float dz = edit_axis(x.lo[2], x.hi[2], P.z, a.sun[2], a.inv_sun[2], tn, tf, miss);
        const float dist2 = (dx * dx + dy * dy) + dz * dz;
        touched = touched || dist2 <= a.r2 || (!miss && tn <= tf && tf > 0.0f);
    }
    return touched;
}

}  // namespace

template <int MODE>
__global__ __launch_bounds__(kTemporalWg) void k_temporal_frame(Frame f, Planes planes, TemporalArgs a) {
    const float4* __restrict__ lf = reinterpret_cast<const float4*>(planes.lighting_f32);
    const uint32_t W = (uint32_t)f.width, npix = W * (uint32_t)f.height;
    const float fw = (float)f.width, fh = (float)f.height;
    for (uint32_t i = blockIdx.x * kTemporalWg + threadIdx.x; i < npix; i += gridDim.x * kTemporalWg) {
        const float4 l = lf[i];
        const vec3 light = v3(l.x * RT_LIGHTING_SCALE, l.y * RT_LIGHTING_SCALE, l.z * RT_LIGHTING_SCALE);
        vec3 sum = v3(0.0f, 0.0f, 0.0f);
        uint32_t n = 1u, nrm;
        float dep;
        if (MODE == TEMPORAL_STILL) {
            // same camera, same world: the previous record holds this frame's depth and normal too
            const uint2 rec = a.prev_rec[i];
            const float4 p = a.prev_sum[i];
            dep = __uint_as_float(rec.x);
            nrm = rec.y >> 27;
            n = (rec.y & kCountMask) + 1u;
            sum = v3(p.x, p.y, p.z);
        } else {
            dep = planes.depth_f32[i];
            nrm = (uint32_t)planes.normal_r8[i];
        }
        if ((MODE == TEMPORAL_MOVED || MODE == TEMPORAL_MOVED_BOXES || MODE == TEMPORAL_MOVED_SLABS) && nrm < 6u && dep < 65535.0f) {
            const vec3 o = ld3(f.origin), o1 = ld3(a.origin), f1 = ld3(a.forward), r1 = ld3(a.right), u1 = ld3(a.up);
            const uint32_t px = i % W, py = i / W;
            const vec3 d = pixel_dir(ld3(f.forward), ld3(f.right), ld3(f.up), (float)px, (float)py, fw, fh);
            const vec3 P = vadd(o, vscale(d, dep / 32.0f));
            const bool touched = MODE == TEMPORAL_MOVED_BOXES ? edit_touches(a, P)
                                 : MODE == TEMPORAL_MOVED_SLABS ? (edit_touches(a, P) || slab_touches(a, P)) : false;
            if (!touched) {
                const vec3 v = vsub(P, o1);
                const float along = dotp(v, f1) / dotp(f1, f1);
                const float sx = (dotp(v, r1) / dotp(r1, r1)) / along;
                const float sy = (dotp(v, u1) / dotp(u1, u1)) / along;
                const float qx = rtm_floor(((sx + 1.0f) * 0.5f) * fw + 0.5f);
                const float qy = rtm_floor(((sy + 1.0f) * 0.5f) * fh + 0.5f);
                // (a NaN fails every comparison: rejected before the conversion to int)
                if (along > 0.0f && qx >= 0.0f && qx < fw && qy >= 0.0f && qy < fh) {
                    const uint32_t q = (uint32_t)qy * W + (uint32_t)qx;
                    const uint2 rec = a.prev_rec[q];
                    const uint32_t c = rec.y & kCountMask;
                    if ((rec.y >> 27) == nrm && c > 0u) {
                        const vec3 d1 = pixel_dir(f1, r1, u1, qx, qy, fw, fh);
                        const vec3 P1 = vadd(o1, vscale(d1, __uint_as_float(rec.x) / 32.0f));
                        const uint32_t k = nrm >> 1;
                        if (rtm_abs(axis_of(P, k) - axis_of(P1, k)) <= 0.25f) {
                            const float4 p = a.prev_sum[q];   // (only accepted pixels load the previous sum)
                            if (c <= a.cap) {
                                sum = v3(p.x, p.y, p.z);
                                n = c + 1u;
                            } else {
                                const float fc = (float)c, fcap = (float)a.cap;
                                sum = v3((p.x / fc) * fcap, (p.y / fc) * fcap, (p.z / fc) * fcap);
                                n = a.cap + 1u;
                            }
                        }
                    }
                }
            }
        }
        sum = vadd(sum, light);
        a.next_sum[i] = make_float4(sum.x, sum.y, sum.z, 0.0f);
        a.next_rec[i] = make_uint2(__float_as_uint(dep), n | (nrm << 27));
        store_lighting(planes, i, sum, (int)n);
    }
}

hipError_t launch_temporal_frame(const Frame& f, const Planes& planes, const TemporalArgs& a, int mode, hipStream_t st) {
    if (f.tile_world != 1 || a.cap < 1u || a.cap > 65535u) return hipErrorInvalidValue;
    const uint32_t npix = (uint32_t)f.width * (uint32_t)f.height;
    if (npix == 0u) return hipSuccess;
    const uint32_t blocks = (npix + kTemporalWg - 1u) / kTemporalWg;
    const dim3 grid(blocks < 4096u ? blocks : 4096u), block(kTemporalWg);
    if (mode == TEMPORAL_RESTART) hipLaunchKernelGGL((k_temporal_frame<TEMPORAL_RESTART>), grid, block, 0, st, f, planes, a);
    else if (mode == TEMPORAL_STILL) hipLaunchKernelGGL((k_temporal_frame<TEMPORAL_STILL>), grid, block, 0, st, f, planes, a);
    else if (mode == TEMPORAL_MOVED) hipLaunchKernelGGL((k_temporal_frame<TEMPORAL_MOVED>), grid, block, 0, st, f, planes, a);
    else if (mode == TEMPORAL_MOVED_BOXES) {
        if (a.nbox < 1u || a.nbox > kTemporalMaxBoxes) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_temporal_frame<TEMPORAL_MOVED_BOXES>), grid, block, 0, st, f, planes, a);
    }
    else if (mode == TEMPORAL_MOVED_SLABS) {
        if (a.nbox > kTemporalMaxBoxes || a.slab == nullptr) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_temporal_frame<TEMPORAL_MOVED_SLABS>), grid, block, 0, st, f, planes, a);
    }
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace rtd
