// rt_emit.hip — gfx950 kernels of rt_emit_particles / rt_emit_particles_async: debris from the occupied voxels of shapes, written in
// a fixed order into a ring of RtParticleState (include/rt_abi.h "Particle emitters"; the rules are restated in
// tests/emit_particles_ref.py).
//
// An ITEM is one (emitter, 4^3 brick) of the host's plan (api/emit_check.hpp): the bricks of an emitter's clipped bounding box,
// z-major, emitter after emitter — which is the order of the rules, because a brick's 64 voxels lie in the swizzled arrays in the
// order (z & 3, y & 3, x & 3).  One wave per item, lane l = voxel l of the brick:
//
//   k_emit_count : the brick's 64 minefield bytes in one coalesced load; a lane tests membership (shape_row, rt_shape_rows.hpp:
//                  rt_edit_shapes' own rule), occupancy and the hash; the ballot is the item's mask, stored for the other two.
//   k_emit_scan  : one workgroup: the exclusive scan of the masks' popcounts — 4096 items per round — which numbers every item's
//                  first particle and gives N; its thread 0 then reads the cursor, decides n and the first slot, leaves both for
//                  k_emit_write and stores the cursor's new value.
//   k_emit_write : lane l of a set bit takes particle base + popcount(mask below l), loads its material word, computes the state
//                  and stores four 16-byte words.  Waves with an empty mask or wholly beyond n leave at once.
//
// No atomic decides a slot.  All float arithmetic is fp32 with one rounding per operation (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "rt_kernels.hpp"
#include "rt_shape_rows.hpp"
#include "rt_world.hpp"

namespace rtd {

namespace {

constexpr uint32_t kEmitWg = 256;        // four waves, one item each
constexpr uint32_t kEmitScanWg = 1024;   // the scan's one workgroup
constexpr uint32_t kEmitScanPer = 4;     // items per thread and round (16 measured slower: a lane's loads follow each other)

__device__ __forceinline__ uint32_t emit_mix(uint32_t h) {
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    return h;
}

// What a wave knows about its item: the emitter's record index and, per lane, the texel and the index into the swizzled arrays.
struct EmitItem {
    uint32_t rec;      // index of the EmitRecord (uniform)
    int bx4;           // the brick's first texel x (uniform)
    int x, y, z;       // the lane's texel
    uint32_t index;    // the lane's entry of the swizzled arrays
};

// Item `item` (uniform across the wave, < a.items) of the plan: the last record whose `first` is not above it, then the brick of
// the record's box.  The brick's coordinates are masked to the region, so that no record can lead a load out of the arrays.
template <int LOGR>
__device__ __forceinline__ EmitItem emit_item(const EmitParticlesArgs& a, uint32_t item, uint32_t lane) {
    uint32_t lo = 0u, hi = a.nrecs - 1u;
    while (lo < hi) {   // (scalar: item and the records are uniform)
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (a.recs[8u * mid + 7u].z <= item) lo = mid; else hi = mid - 1u;
    }
    const uint4 q6 = a.recs[8u * lo + 6u], q7 = a.recs[8u * lo + 7u];
    const uint32_t rel = item - q7.z;
    const uint32_t nbx = q6.w ? q6.w : 1u, nby = q7.x ? q7.x : 1u;
    constexpr int lb = LOGR - 2;
    constexpr uint32_t bmask = (1u << lb) - 1u;
    const uint32_t bx = (q6.x + rel % nbx) & bmask, by = (q6.y + (rel / nbx) % nby) & bmask, bz = (q6.z + rel / (nbx * nby)) & bmask;
    EmitItem it;
    it.rec = lo;
    it.bx4 = (int)(4u * bx);
    it.x = it.bx4 + (int)(lane & 3u);
    it.y = (int)(4u * by + ((lane >> 2) & 3u));
    it.z = (int)(4u * bz + (lane >> 4));
    it.index = (brick_index(bx, by, bz, lb) << 6) | lane;
    return it;
}

// The world voxel of texel x under window centre lr: the one integer in [lr - R/2, lr + R/2) congruent to x - R/2 mod R.
template <int LOGR>
__device__ __forceinline__ int emit_world(int x, int lr) {
    constexpr int R = 1 << LOGR;
    return lr - R / 2 + (int)((uint32_t)(x - lr) & (uint32_t)(R - 1));
}

__device__ __forceinline__ uint32_t emit_hash(uint32_t seed, int vx, int vy, int vz) {
    return emit_mix(seed ^ emit_mix((uint32_t)vx ^ emit_mix((uint32_t)vy ^ emit_mix((uint32_t)vz))));
}

__device__ __forceinline__ uint64_t* emit_masks(uint32_t* scratch) { return reinterpret_cast<uint64_t*>(scratch + 4); }
__device__ __forceinline__ uint32_t* emit_bases(uint32_t* scratch, uint32_t items) { return scratch + 4 + 2u * (size_t)items; }

template <int LOGR>
__global__ __launch_bounds__(kEmitWg) void k_emit_count(Scene sc, EmitParticlesArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t item = __builtin_amdgcn_readfirstlane(blockIdx.x * (kEmitWg / 64u) + (threadIdx.x >> 6));
    if (item >= a.items) return;
    const EmitItem it = emit_item<LOGR>(a, item, lane);
    const uint32_t byte = sc.mine[it.index];
    const uint4 q0 = a.recs[8u * it.rec], q1 = a.recs[8u * it.rec + 1u];
    const uint32_t density = a.recs[8u * it.rec + 4u].w;
    const int4 p = make_int4((int)q0.x, (int)q0.y, (int)q0.z, 0), q = make_int4((int)q1.x, (int)q1.y, (int)q1.z, 0);
    const bool member = ((shape_row(q1.w & 0xFFu, p, q, it.bx4, it.y, it.z) >> (lane & 3u)) & 1ull) != 0ull;
    const uint32_t h = emit_hash(q0.w, emit_world<LOGR>(it.x, a.lr[0]), emit_world<LOGR>(it.y, a.lr[1]), emit_world<LOGR>(it.z, a.lr[2]));
    const uint64_t mask = __ballot(member && byte == 0u && (h & 255u) < density);
    if (lane == 0u) emit_masks(a.scratch)[item] = mask;
}

__global__ __launch_bounds__(kEmitScanWg) void k_emit_scan(EmitParticlesArgs a) {
    __shared__ uint32_t wave_sum[kEmitScanWg / 64u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t* masks = emit_masks(a.scratch);
    uint32_t* bases = emit_bases(a.scratch, a.items);
    uint32_t carry = 0u;   // particles of the rounds before (the same in every thread)
    for (uint32_t t0 = 0u; t0 < a.items; t0 += kEmitScanWg * kEmitScanPer) {
        const uint32_t i0 = t0 + kEmitScanPer * tid;
        uint32_t c[kEmitScanPer], s = 0u;
#pragma unroll
        for (uint32_t k = 0; k < kEmitScanPer; k++) {
            c[k] = i0 + k < a.items ? (uint32_t)__popcll(masks[i0 + k]) : 0u;
            s += c[k];
        }
        uint32_t incl = s;
#pragma unroll
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const uint32_t v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        if (lane == 63u) wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = 0u, total = 0u;
#pragma unroll
        for (uint32_t w = 0; w < kEmitScanWg / 64u; w++) {
            const uint32_t v = wave_sum[w];
            before += w < wave ? v : 0u;
            total += v;
        }
        uint32_t run = carry + before + incl - s;
#pragma unroll
        for (uint32_t k = 0; k < kEmitScanPer; k++) {
            if (i0 + k < a.items) bases[i0 + k] = run;
            run += c[k];
        }
        carry += total;
        __syncthreads();   // wave_sum is written again in the next round
    }
    if (tid == 0u) {
        const uint4 cur = *a.cursor;
        const uint32_t start = cur.x % a.capacity;
        const uint32_t N = carry, n = N < a.max_emit ? N : a.max_emit;
        uint32_t next = start + n;   // both below 2^20 + 1
        if (next >= a.capacity) next -= a.capacity;
        *reinterpret_cast<uint4*>(a.scratch) = make_uint4(start, n, 0u, 0u);
        *a.cursor = make_uint4(next, cur.y + n, cur.z + (N - n), cur.w);
    }
}

template <int LOGR>
__global__ __launch_bounds__(kEmitWg) void k_emit_write(Scene sc, EmitParticlesArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t item = __builtin_amdgcn_readfirstlane(blockIdx.x * (kEmitWg / 64u) + (threadIdx.x >> 6));
    if (item >= a.items) return;
    const uint64_t mask = emit_masks(a.scratch)[item];
    const uint32_t base = emit_bases(a.scratch, a.items)[item];
    const uint32_t start = a.scratch[0], n = a.scratch[1];
    if (mask == 0ull || base >= n) return;
    const uint32_t j = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (((mask >> lane) & 1ull) == 0ull || j >= n) return;
    const EmitItem it = emit_item<LOGR>(a, item, lane);
    uint32_t slot = start + j;   // start < capacity and j < n <= capacity
    if (slot >= a.capacity) slot -= a.capacity;

    const uint4 q0 = a.recs[8u * it.rec], q1 = a.recs[8u * it.rec + 1u], q2 = a.recs[8u * it.rec + 2u], q3 = a.recs[8u * it.rec + 3u];
    const uint4 q4 = a.recs[8u * it.rec + 4u], q5 = a.recs[8u * it.rec + 5u];
    const int v[3] = {emit_world<LOGR>(it.x, a.lr[0]), emit_world<LOGR>(it.y, a.lr[1]), emit_world<LOGR>(it.z, a.lr[2])};
    const uint32_t h = emit_hash(q0.w, v[0], v[1], v[2]);
    float u[4];
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) u[i] = (float)(emit_mix(h + i + 1u) >> 8) * 5.9604644775390625e-08f;   // 2^-24
    const float origin[3] = {__uint_as_float(q2.x), __uint_as_float(q2.y), __uint_as_float(q2.z)}, speed = __uint_as_float(q2.w);
    const float drift[3] = {__uint_as_float(q3.x), __uint_as_float(q3.y), __uint_as_float(q3.z)}, spread = __uint_as_float(q3.w);
    const float half = __uint_as_float(q4.x), life_min = __uint_as_float(q4.y), life_span = __uint_as_float(q4.z);
    float lo[3], hi[3], r[3], vel[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float c = (float)v[k] + 0.5f;
        lo[k] = c - half;
        hi[k] = c + half;
        r[k] = c - origin[k];
    }
    const float len = rtm_length3({r[0], r[1], r[2]});
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float dir = len > 0.0f ? r[k] / len : 0.0f;
        vel[k] = (dir * speed + (u[k] * 2.0f - 1.0f) * spread) + drift[k];
    }
    const float life = life_min + u[3] * life_span;
    const uint32_t material = sc.mat[it.index];

    uint4* out = a.states + 4u * (size_t)slot;
    out[0] = make_uint4(__float_as_uint(lo[0]), __float_as_uint(lo[1]), __float_as_uint(lo[2]), __float_as_uint(life));
    out[1] = make_uint4(__float_as_uint(hi[0]), __float_as_uint(hi[1]), __float_as_uint(hi[2]), (q1.w >> 8) & 0xFFu);
    out[2] = make_uint4(__float_as_uint(vel[0]), __float_as_uint(vel[1]), __float_as_uint(vel[2]), q5.x);
    out[3] = make_uint4(material, q5.y, q4.x, 0u);
}

}  // namespace

hipError_t launch_emit_particles(const Scene& sc, int logr, const EmitParticlesArgs& a, hipStream_t st) {
    if (logr < 8 || logr > 10 || a.nrecs < 1u || a.nrecs > kMaxEmitRecords || a.items < 1u || a.items > kMaxEmitItems || a.capacity < 1u ||
        a.capacity > kMaxParticles || a.max_emit < 1u || a.max_emit > a.capacity)
        return hipErrorInvalidValue;
    const dim3 grid((a.items + kEmitWg / 64u - 1u) / (kEmitWg / 64u)), block(kEmitWg);
    if (logr == 8) hipLaunchKernelGGL((k_emit_count<8>), grid, block, 0, st, sc, a);
    else if (logr == 9) hipLaunchKernelGGL((k_emit_count<9>), grid, block, 0, st, sc, a);
    else hipLaunchKernelGGL((k_emit_count<10>), grid, block, 0, st, sc, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_emit_scan, dim3(1), dim3(kEmitScanWg), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (logr == 8) hipLaunchKernelGGL((k_emit_write<8>), grid, block, 0, st, sc, a);
    else if (logr == 9) hipLaunchKernelGGL((k_emit_write<9>), grid, block, 0, st, sc, a);
    else hipLaunchKernelGGL((k_emit_write<10>), grid, block, 0, st, sc, a);
    return hipGetLastError();
}

}  // namespace rtd
