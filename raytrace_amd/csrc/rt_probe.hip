// rt_probe.hip — gfx950 kernels of rt_probe_light / rt_probe_light_async: the light loop of the shader's non-air branch
// (raytrace.comp:317-350, generalised to `depth` levels as k_mega's loop does) from surfaces the host hands over.
//
//   k_probe     : one lane per path = (probe, sample), probe-major, so that a probe's samples sit in neighbouring lanes and share
//                 their first fetches.  Rays are stepped with the shared DDA of rt_dda.hpp in its direct-fetch form (dda_arm /
//                 dda_advance with DIRECT = true, as k_query and k_frame step theirs; k_query's header says why a persistent
//                 LDS-map kernel lost for batches of this kind).  A path keeps its shadow bits and the terminal sky in registers
//                 and its albedo stack in LDS (a runtime-indexed register array would live in scratch memory), then calls
//                 unwind_light.  PAIR: the shadow and the diffuse ray of a level are independent, so the lane steps both in one
//                 loop — two fetch chains in flight per lane instead of one (measured against the plain form: DESIGN.md "Light
//                 probes").
//   the sum     : a probe's lights are added in sample order by ONE lane — no float atomics, no order that depends on the launch
//                 shape.  Each path leaves a 16-byte record (light rgb, its sun1.air bit).  When a workgroup holds whole probes
//                 (samples divides kProbeWg) the records stay in LDS and lane t of the workgroup adds those of its t-th probe;
//                 otherwise they go to a scratch array and k_probe_sum adds them, one lane per probe.
#include <hip/hip_runtime.h>

#include "rt_dda.hpp"
#include "rt_kernels.hpp"

namespace rtd {

namespace {

constexpr uint32_t kProbeWg = 256;
constexpr uint32_t kProbeStack = RT_MAX_DEPTH - 1;   // albedo words of the surfaces of levels 2..depth

// Head of trace_ray (:83-107) as k_query arms it: normalize (:83), 1/|d| (:88), the first texel, then dda_arm.
template <int LOGR, bool LRZ>
__device__ __forceinline__ void pr_arm(RaySlot2& r, vec3 o, vec3 dir, const Frame& f, const Scene& sc) {
    constexpr int R = 1 << LOGR, LB = LOGR - 2;
    const vec3 d = vnormalize(dir);
    r.lx = 1.0f / rtm_abs(d.x); r.ly = 1.0f / rtm_abs(d.y); r.lz = 1.0f / rtm_abs(d.z);
    int ix, iy, iz;
    const bool ok = wrap_texel(o, (float)R, &ix, &iy, &iz);
    unsigned long long unused = 0;
    dda_arm<LOGR, LRZ, false, true, false>(r, d.x, d.y, d.z, o.x, o.y, o.z, ok, swizzled_index(ix, iy, iz, LB), 0u, f, (float)(R / 2),
                                           nullptr, sc, unused, nullptr);
}

// What the light loop needs of an ended diffuse ray (trace_ray's HitResult, :163-182): the position after the 0.001 offset off the
// face, the face code and the material word; returns whether the ray left the region.
template <int LOGR, bool LRZ>
__device__ __forceinline__ bool pr_surface(const RaySlot2& r, const Scene& sc, vec3* pos, uint32_t* normal, uint32_t* material) {
    const uint32_t kind = r2_kind(r);
    const uint32_t nrm = r.axis == 0 ? (r.ndx < 0.0f ? 1u : 0u) : (r.axis == 1 ? (r.ndy < 0.0f ? 3u : 2u) : (r.ndz < 0.0f ? 5u : 4u));
    vec3 p = v3(r.px, r.py, r.pz);
    if (kind == PX_SPECIAL) p = v3(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));   // it never moved: mod(x, 0) (Q12)
    *material = (kind == PX_HIT && (LRZ || r.valid)) ? sc.mat[r.vox] : 0u;                          // :150-154 (limit, border: 0)
    const float off = 0.001f;                                                                       // :166-180
    if (nrm == 0) p.x += off; else if (nrm == 1) p.x -= off;
    else if (nrm == 2) p.y += off; else if (nrm == 3) p.y -= off;
    else if (nrm == 4) p.z += off; else p.z -= off;
    *pos = p;
    *normal = nrm;
    return kind == PX_AIR;
}

// The path of sample `s` from the surface {pos, normal}: k_mega's loop (rt_kernels.hip) with the probe's cell in place of the
// pixel's workgroup.  s_stack: this lane's column of the workgroup's albedo stack (stride kProbeWg).
template <int LOGR, bool LRZ, bool PAIR>
__device__ __forceinline__ float4 probe_path(const Scene& sc, const Frame& f, vec3 pos, uint32_t normal, uint32_t cell, uint32_t s,
                                             uint32_t* s_stack) {
    constexpr float half = (float)((1 << LOGR) / 2);
    const vec3 sunangle = ld3(f.sunangle), sunlight = ld3(f.sunlight);
    const uint32_t seed = (f.seed + s) % (uint32_t)RT_NOISE_BYTES;
    const uint32_t base = noise_texel(sc, (float)(seed % RT_NOISE_SIZE), (float)(seed / RT_NOISE_SIZE));   // :298-304
    NoiseOffset no;
    no.x = unorm8(base, 0) * 255.0f + (float)((cell & 0xFFFFu) * RT_SHADER_GROUP_SIZE);
    no.y = unorm8(base, 1) * 255.0f + (float)((cell >> 16) * RT_SHADER_GROUP_SIZE);
    uint32_t sunbits = 0;
    int K = 0;
    bool terminal_sky = false;
    vec3 sky = v3(0.0f, 0.0f, 0.0f);
    unsigned long long unused = 0;
    for (int level = 1; level <= f.depth; level++) {
        const uint32_t nv = noise_value_texel(sc, no, level);
        const float nr = unorm8(nv, 0), ng = unorm8(nv, 1);
        const vec3 ddir = diffuse_direction(normal, nr, ng);
        RaySlot2 sun, dif;
        pr_arm<LOGR, LRZ>(sun, pos, sun_ray_direction(sunangle, nr, ng), f, sc);
        pr_arm<LOGR, LRZ>(dif, pos, ddir, f, sc);
        if (PAIR) {
            while (sun.tracing || dif.tracing) {
                // both bytes are asked for before either ray moves; an ended ray's index stays inside the array
                const uint32_t vs = sc.mine[sun.vox], vd = sc.mine[dif.vox];
                if (sun.tracing) dda_advance<LOGR, LRZ, false, false, false>(sun, vs, f, half, unused, nullptr);
                if (dif.tracing) dda_advance<LOGR, LRZ, false, false, false>(dif, vd, f, half, unused, nullptr);
            }
        } else {
            while (sun.tracing) dda_advance<LOGR, LRZ, false, false, false>(sun, (uint32_t)sc.mine[sun.vox], f, half, unused, nullptr);
            while (dif.tracing) dda_advance<LOGR, LRZ, false, false, false>(dif, (uint32_t)sc.mine[dif.vox], f, half, unused, nullptr);
        }
        if (r2_kind(sun) == PX_AIR) sunbits |= 1u << (level - 1);
        uint32_t material;
        const bool air = pr_surface<LOGR, LRZ>(dif, sc, &pos, &normal, &material);
        K = level;
        if (air) { terminal_sky = true; sky = sample_sky(ddir, sunangle, sunlight, true); break; }   // :331-332 / :343-345
        if (level == f.depth) break;
        s_stack[(uint32_t)(level - 1) * kProbeWg] = material;   // albedo of surface level + 1
    }
    const vec3 L1 = unwind_light(K, sunbits, terminal_sky, sky, sunlight, [&](int j) { return s_stack[(uint32_t)(j - 1) * kProbeWg]; });
    const vec3 light = vadd(v3(0.0f, 0.0f, 0.0f), L1);   // vec3 light = vec3(0); ... light += light1
    return make_float4(light.x, light.y, light.z, __uint_as_float(sunbits & 1u));
}

// records[0 .. n) of one probe added in order -> its RtProbeLight
template <typename Rec>
__device__ __forceinline__ uint4 probe_sum(Rec rec, uint32_t n) {
    vec3 sum = v3(0.0f, 0.0f, 0.0f);
    uint32_t sun = 0;
    for (uint32_t s = 0; s < n; s++) {
        const float4 r = rec(s);
        sum = vadd(sum, v3(r.x, r.y, r.z));
        sun += __float_as_uint(r.w);
    }
    const float fn = (float)n;
    return make_uint4(__float_as_uint(sum.x / fn), __float_as_uint(sum.y / fn), __float_as_uint(sum.z / fn), sun);
}

template <int LOGR, bool LRZ, bool PAIR, bool IN_LDS>
__global__ __launch_bounds__(kProbeWg) void k_probe(Scene sc, Frame f, ProbeArgs a) {
    __shared__ uint32_t s_stack[kProbeStack * kProbeWg];
    __shared__ float4 s_rec[IN_LDS ? kProbeWg : 1];
    const uint32_t p = blockIdx.x * kProbeWg + threadIdx.x, npaths = a.count * a.samples;   // (at most 2^26: checked by the host)
    if (p < npaths) {
        const uint32_t probe = p / a.samples, s = p - probe * a.samples;
        const uint4 r0 = a.probes[2u * probe];
        const uint32_t cell = a.probes[2u * probe + 1u].x;
        const uint32_t normal = r0.w > (uint32_t)RT_PROBE_SPHERE ? (uint32_t)RT_PROBE_SPHERE : r0.w;   // (the async call cannot reject it)
        const float4 rec = probe_path<LOGR, LRZ, PAIR>(sc, f, v3(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z)),
                                                       normal, cell, s, s_stack + threadIdx.x);
        if (IN_LDS) s_rec[threadIdx.x] = rec; else a.scratch[p] = rec;
    }
    if (IN_LDS) {
        __syncthreads();
        // samples divides kProbeWg: the workgroup's paths are those of kProbeWg / samples whole probes
        const uint32_t per_wg = kProbeWg / a.samples, probe = blockIdx.x * per_wg + threadIdx.x;
        if (threadIdx.x < per_wg && probe < a.count) {
            const float4* rec = s_rec + threadIdx.x * a.samples;
            a.out[probe] = probe_sum([&](uint32_t s) { return rec[s]; }, a.samples);
        }
    }
}

__global__ __launch_bounds__(kProbeWg) void k_probe_sum(ProbeArgs a) {
    const uint32_t probe = blockIdx.x * kProbeWg + threadIdx.x;
    if (probe >= a.count) return;
    const float4* rec = a.scratch + (size_t)probe * a.samples;
    a.out[probe] = probe_sum([&](uint32_t s) { return rec[s]; }, a.samples);
}

template <int LOGR, bool LRZ>
void probe_launch(const Scene& sc, const Frame& f, const ProbeArgs& a, bool pair, bool in_lds, dim3 grid, hipStream_t st) {
    const dim3 block(kProbeWg);
    if (pair) {
        if (in_lds) hipLaunchKernelGGL((k_probe<LOGR, LRZ, true, true>), grid, block, 0, st, sc, f, a);
        else hipLaunchKernelGGL((k_probe<LOGR, LRZ, true, false>), grid, block, 0, st, sc, f, a);
    } else {
        if (in_lds) hipLaunchKernelGGL((k_probe<LOGR, LRZ, false, true>), grid, block, 0, st, sc, f, a);
        else hipLaunchKernelGGL((k_probe<LOGR, LRZ, false, false>), grid, block, 0, st, sc, f, a);
    }
}

}  // namespace

bool probe_sums_in_lds(uint32_t samples) { return samples <= kProbeWg && kProbeWg % samples == 0u; }

hipError_t launch_probe(const Scene& sc, const Frame& f, const ProbeArgs& a, bool pair, hipStream_t st) {
    if (f.logr < 8 || f.logr > 10 || f.depth < 1 || f.depth > RT_MAX_DEPTH || a.samples == 0u) return hipErrorInvalidValue;
    if (a.count == 0u) return hipSuccess;
    if ((uint64_t)a.count * a.samples > kProbeMaxPaths) return hipErrorInvalidValue;
    const bool in_lds = probe_sums_in_lds(a.samples);
    if (!in_lds && !a.scratch) return hipErrorInvalidValue;
    const uint32_t npaths = a.count * a.samples;
    const dim3 grid((npaths + kProbeWg - 1u) / kProbeWg);
    launch_for_region(f, [&](auto L, auto Z) { probe_launch<decltype(L)::value, decltype(Z)::value>(sc, f, a, pair, in_lds, grid, st); });
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && !in_lds) {
        hipLaunchKernelGGL(k_probe_sum, dim3((a.count + kProbeWg - 1u) / kProbeWg), dim3(kProbeWg), 0, st, a);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace rtd
