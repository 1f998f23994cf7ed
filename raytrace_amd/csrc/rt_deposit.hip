// rt_deposit.hip — gfx950 kernels of rt_deposit_particles / rt_deposit_particles_async: particles that have come to rest become
// voxels of the resident region (include/rt_abi.h "Particle deposits"; the rules are restated in tests/deposit_particles_ref.py).
//
//   k_deposit_claim  : one lane per particle.  Three 16-byte loads (box, flags, velocity), the candidate test, the target texel, one
//             minefield byte.  A depositing lane claims its texel with atomicMin(claim, i) — the lowest index wins whatever the
//             arrival order — stores 0 to its chunk's flag word (every writer stores the same value), ORs DEAD into its flags word
//             and clears draw[i].half.  The three counters are summed per wave by ballot and added with one atomic per wave.
//   k_deposit_chunks : one workgroup per chunk of the box.  A workgroup whose flag word was never written returns before the first
//             barrier; the others run the chunk rebuild (rt_rebuild_chunk.hpp) with DepositStage: a wave reads the claims of its
//             rows one row per load (lane = x), the ballot of "claimed" is the row's bits, and a claimed lane stores the winner's
//             material word.
//   (k_rebuild_chunk_maps, rt_edit.hip, follows over the same chunk list.)
//
// The claims and flags are one block that the host fills with 0xFF bytes in front of the claim pass: an unclaimed texel and an
// untouched chunk both read 0xFFFFFFFF, no particle index.
#include <hip/hip_runtime.h>

#include "rt_kernels.hpp"
#include "rt_rebuild_chunk.hpp"

namespace rtd {

namespace {

constexpr uint32_t kClaimWg = 256;
constexpr uint32_t kNoClaim = 0xFFFFFFFFu;
constexpr uint32_t kInactive = RT_PSTATE_DEAD | RT_PSTATE_INVALID;
constexpr float kDomain = 4194304.0f;   // rt_sweep_boxes' |lo|, |hi| <= 2^22

// one atomic per wave: the lanes that pass `p` counted by ballot, added by the wave's first active lane
__device__ __forceinline__ void wave_count(uint32_t* counter, bool p) {
    const uint64_t b = __ballot(p);
    if (b == 0ull) return;
    const uint64_t active = __ballot(true);
    if ((uint32_t)(threadIdx.x & 63u) == (uint32_t)(__ffsll((unsigned long long)active) - 1)) atomicAdd(counter, (uint32_t)__popcll(b));
}

template <int LOGR>
__global__ __launch_bounds__(kClaimWg) void k_deposit_claim(const uint8_t* __restrict__ mine_sw, DepositArgs a) {
    constexpr int R = 1 << LOGR, H = R / 2;
    const uint32_t i = blockIdx.x * kClaimWg + threadIdx.x;
    const bool have = i < a.count;
    bool candidate = false;
    int v[3] = {0, 0, 0};
    uint32_t state_flags = 0u;
    if (have) {
        const uint4* in = a.states + 4u * (size_t)i;
        const uint4 r0 = in[0], r1 = in[1], r2 = in[2];
        state_flags = r1.w;
        const float lo[3] = {__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z)};
        const float hi[3] = {__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z)};
        const float vel[3] = {__uint_as_float(r2.x), __uint_as_float(r2.y), __uint_as_float(r2.z)};
        candidate = (r1.w & kInactive) == 0u && (r1.w & RT_PSTATE_CONTACT) != 0u;
#pragma unroll
        for (int k = 0; k < 3; k++) {   // (every comparison is false for a NaN)
            candidate = candidate && __builtin_fabsf(vel[k]) <= a.max_speed && __builtin_fabsf(lo[k]) <= kDomain && __builtin_fabsf(hi[k]) <= kDomain;
            const float c = (lo[k] + hi[k]) * 0.5f;
            v[k] = candidate ? (int)__builtin_floorf(c) : 0;
        }
    }
    // the target: inside the window, then inside the clipped box
    bool inside = candidate;
    int x[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        inside = inside && v[k] >= a.lr[k] - H && v[k] < a.lr[k] + H;
        x[k] = (int)(((uint32_t)v[k] + (uint32_t)H) & (uint32_t)(R - 1));
        inside = inside && x[k] >= a.lo[k] && x[k] <= a.hi[k];
    }
    bool deposits = false;
    if (inside) deposits = mine_sw[swizzled_index(x[0], x[1], x[2], LOGR - 2)] != 0u;
    const uint64_t depositing = __ballot(deposits);
    if (deposits) {
        const uint32_t ex = (uint32_t)(a.hi[0] - a.lo[0] + 1), ey = (uint32_t)(a.hi[1] - a.lo[1] + 1);
        const uint32_t t = ((uint32_t)(x[2] - a.lo[2]) * ey + (uint32_t)(x[1] - a.lo[1])) * ex + (uint32_t)(x[0] - a.lo[0]);
        atomicMin(&a.claims[t], i);
        const uint32_t ncx = (uint32_t)((a.hi[0] >> 6) - (a.lo[0] >> 6) + 1), ncy = (uint32_t)((a.hi[1] >> 6) - (a.lo[1] >> 6) + 1);
        const uint32_t ci = ((uint32_t)((x[2] >> 6) - (a.lo[2] >> 6)) * ncy + (uint32_t)((x[1] >> 6) - (a.lo[1] >> 6))) * ncx +
                            (uint32_t)((x[0] >> 6) - (a.lo[0] >> 6));
        // the chunk's flag: one store for the lanes that share the first depositing lane's chunk (most waves land in one chunk)
        const int first = __ffsll((unsigned long long)depositing) - 1;
        const uint32_t ci0 = (uint32_t)__shfl((int)ci, first);
        if (ci != ci0 || (int)(threadIdx.x & 63u) == first) a.flags[ci] = 0u;
        reinterpret_cast<uint32_t*>(a.states)[16u * (size_t)i + 7u] = state_flags | RT_PSTATE_DEAD;   // RtParticleState.flags, this lane's own
        if (a.draw) reinterpret_cast<uint32_t*>(a.draw)[8u * (size_t)i + 3u] = 0u;   // RtParticle.half = +0.0f
    }
    wave_count(a.counts + 0, deposits);
    wave_count(a.counts + 2, inside && !deposits);
    wave_count(a.counts + 3, candidate && !inside);
}

// rt_deposit_particles' edit stage.  WAVE w owns the rows ShapeStage gives its 64 threads — (z, y) with z = w + 16 j, j = 0..3, and
// every y — and walks them one row per step with lane = x: the row's claims are 256 contiguous bytes, one coalesced load; the ballot of
// "claimed" is the row's bits, ORed into the bitmap by lane 0 (no other wave has rows with this z); a lane whose texel is claimed
// stores the winner's material word.  Eight rows' loads are issued before the first is used.
struct DepositStage {
    uint32_t* __restrict__ mat_sw;
    const uint32_t* __restrict__ claims;
    const uint32_t* __restrict__ states;   // RtParticleState as 16 words each; word 12 = material
    uint32_t* __restrict__ voxels;         // RtDepositCount.voxels
    int lo[3], hi[3];
    __device__ __forceinline__ void operator()(uint32_t* occ0, uint32_t cx, uint32_t cy, uint32_t cz, int lb, int tid) const {
        __shared__ uint32_t wsum[16];
        constexpr int kBatch = 8;
        const int x0 = (int)(cx * 64u), y0 = (int)(cy * 64u), z0 = (int)(cz * 64u);
        const int lane = tid & 63, wave = tid >> 6, x = x0 + lane;
        const bool in_x = x >= lo[0] && x <= hi[0];
        const int ya = (lo[1] > y0 ? lo[1] : y0), yb = (hi[1] < y0 + 63 ? hi[1] : y0 + 63);   // the box's rows of a layer
        const uint32_t ex = (uint32_t)(hi[0] - lo[0] + 1), ey = (uint32_t)(hi[1] - lo[1] + 1);
        uint32_t n = 0;   // (the same in every lane of the wave)
        for (int j = 0; j < 4; j++) {
            const int z = z0 + wave + 16 * j;
            if (z < lo[2] || z > hi[2]) continue;
            const uint32_t* layer = claims + (size_t)(uint32_t)(z - lo[2]) * ey * ex;
            for (int yy = ya; yy <= yb; yy += kBatch) {
                uint32_t c[kBatch];
#pragma unroll
                for (int u = 0; u < kBatch; u++)
                    c[u] = (in_x && yy + u <= yb) ? layer[(size_t)(uint32_t)(yy + u - lo[1]) * ex + (uint32_t)(x - lo[0])] : kNoClaim;
#pragma unroll
                for (int u = 0; u < kBatch; u++) {
                    const uint64_t sel = __ballot(c[u] != kNoClaim);
                    if (sel == 0ull) continue;
                    const int y = yy + u;
                    if (c[u] != kNoClaim) mat_sw[swizzled_index(x, y, z, lb)] = states[16u * (size_t)c[u] + 12u];
                    if (lane == 0) {
                        const int w = 2 * ((wave + 16 * j) * kRow0Stride + (y - y0));
                        occ0[w] |= (uint32_t)sel;
                        occ0[w + 1] |= (uint32_t)(sel >> 32);
                    }
                    n += (uint32_t)__popcll(sel);
                }
            }
        }
        // voxels: a sum per wave, then one atomic per workgroup
        if (lane == 0) wsum[wave] = n;
        __syncthreads();
        if (tid == 0) {
            uint32_t s = 0;
            for (int k = 0; k < 16; k++) s += wsum[k];
            if (s) atomicAdd(voxels, s);
        }
    }
};

// One workgroup per chunk of the box, in the order of the chunk list (ascending ids = z-major over the box's chunks, as the claim
// pass numbers the flags).  The flag word is read by every thread (one address: a uniform value), so the exit is the workgroup's.
__global__ __launch_bounds__(1024) void k_deposit_chunks(uint8_t* __restrict__ mine_sw, uint32_t* __restrict__ mat_sw,
                                                         const uint32_t* __restrict__ chunks, DepositArgs a, int logr) {
    if (a.flags[blockIdx.x] != 0u) return;   // nothing deposited in this chunk: its bytes stay as they are
    DepositStage stage{mat_sw, a.claims, reinterpret_cast<const uint32_t*>(a.states), a.counts + 1, {a.lo[0], a.lo[1], a.lo[2]}, {a.hi[0], a.hi[1], a.hi[2]}};
    rebuild_chunk(mine_sw, chunks, logr, stage);
}

}  // namespace

hipError_t launch_deposit_particles(uint8_t* mine_sw, uint32_t* mat_sw, const uint32_t* chunks, uint32_t nchunks, int logr, const DepositArgs& a,
                                    hipStream_t st) {
    if (logr < 8 || logr > 10 || a.count < 1u || a.count > kMaxParticles || nchunks < 1u) return hipErrorInvalidValue;
    uint64_t texels = 1, boxchunks = 1;
    for (int k = 0; k < 3; k++) {
        if (a.lo[k] < 0 || a.hi[k] >= (1 << logr) || a.lo[k] > a.hi[k]) return hipErrorInvalidValue;
        texels *= (uint64_t)(a.hi[k] - a.lo[k] + 1);
        boxchunks *= (uint64_t)((a.hi[k] >> 6) - (a.lo[k] >> 6) + 1);
    }
    if (texels > kMaxDepositTexels || boxchunks != nchunks) return hipErrorInvalidValue;
    const dim3 grid((a.count + kClaimWg - 1u) / kClaimWg), block(kClaimWg);
    if (logr == 8) hipLaunchKernelGGL((k_deposit_claim<8>), grid, block, 0, st, mine_sw, a);
    else if (logr == 9) hipLaunchKernelGGL((k_deposit_claim<9>), grid, block, 0, st, mine_sw, a);
    else hipLaunchKernelGGL((k_deposit_claim<10>), grid, block, 0, st, mine_sw, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_deposit_chunks, dim3(nchunks), dim3(1024), 0, st, mine_sw, mat_sw, chunks, a, logr);
    return hipGetLastError();
}

}  // namespace rtd
