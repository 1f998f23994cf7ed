// rt_detach.hip — gfx950 kernels of rt_detach_voxels / rt_detach_voxels_async: the occupied voxels of a box of texels that no path
// of face-adjacent occupied voxels joins to an anchor are found, carved and captured into a stamp (include/rt_abi.h "Voxel
// detachment"; the rules are restated twice in tests/detach_voxels_ref.py).  Every launch has one workgroup per chunk of the box,
// numbered z-major over the box's chunks, and the sets are bitmaps: per chunk 64 x 64 rows of 64 bits along x, row z * 64 + y.
//
//   k_detach_seed   : a lane per row.  The row's occupancy (minefield byte == 0, masked to the clipped box) is built from sixteen
//             dwords, one per brick along x — a wave's lanes cover four whole bricks per load — and stored; the anchors S_0 (the box's
//             faces named in anchor_faces, and with RT_DETACH_ANCHOR_MATERIAL the occupied cells whose word passes the mask test) go
//             into reach buffer 0.  The launch also sets the chunk's flag word and clears the head, so the scratch needs no fill.
//   k_detach_reach  : pass p of the contract.  A workgroup whose pass comes after the end (pass p - 1 changed nothing) returns at
//             once.  Otherwise it loads its occupancy and its reach bits of pass p - 1 into LDS (2 x 32 KiB), ORs in the adjacent
//             layer of its six neighbours' reach bits of pass p - 1, and closes the set inside the chunk: every thread ORs the four
//             rows beside each of its rows into it, masks by occupancy and floods along x (a Kogge-Stone fill, six steps each way),
//             until a pass over all rows changes none.  The closure is monotone — bits are only set, and a torn read of a
//             neighbour's row sees a subset of a later state — so it has one fixed point whatever the order; an iteration that is not
//             the last completes at least one more run of occupied cells along x, of which a chunk has at most 64 * 64 * 32, and that
//             is the loop's explicit bound.  The result goes to reach buffer p & 1, and head word p is set if any row differs from
//             pass p - 1's: a pass reads only the previous pass's state, which is what makes `passes` exact.
//   k_detach_apply  : finds the first pass that changed nothing (a scan of at most 256 head words) — none means unconverged, and
//             every row then counts as holding no detached voxel.  Every thread takes four rows: occupied and not reached are the
//             detached bits, kept in LDS (32 KiB), with the rows' counts and bounds, which are summed per wave and added with one
//             atomic per wave and field; a chunk with a detached voxel counts into `chunks` and, with RT_DETACH_CARVE, stores 0 to
//             its flag word.  Then a wave walks rows, lane = x, reading the row's bits from LDS so that no global load stands between
//             two rows: with RT_DETACH_CAPTURE every cell of the box writes its stamp voxel (SOLID and the word for a detached
//             voxel, ABSENT and 0 otherwise, so the stamp needs no clear), then with RT_DETACH_CARVE a detached cell gets a non-zero
//             minefield byte (the chunk pass gives the final value) and air_material — the same lane reads the word before it
//             writes it.
//   k_detach_chunks : one workgroup per chunk of the box.  A workgroup whose flag word was never cleared returns before the first
//             barrier; the others run the chunk rebuild (rt_rebuild_chunk.hpp) with a stage that does nothing.
//   (k_rebuild_chunk_maps, rt_edit.hip, follows over the same chunk list.)
#include <hip/hip_runtime.h>

#include "rt_kernels.hpp"
#include "rt_rebuild_chunk.hpp"

namespace rtd {

namespace {

constexpr uint32_t kDetachWg = 1024;                  // sixteen waves
constexpr int kRows = 64 * 64;                        // rows of a chunk
constexpr int kClosureCap = 64 * 64 * 32;             // runs of occupied cells along x in a chunk: the closure's bound

// where a workgroup's chunk lies and where its bitmaps are
struct DetachChunk {
    int ncx, ncy, ncz, bx, by, bz;   // the box's chunks per axis, this chunk among them
    int cx, cy, cz;                  // this chunk in the region
    uint32_t n;                      // chunks of the box
};
__device__ __forceinline__ DetachChunk detach_chunk(const DetachArgs& a, uint32_t b) {
    DetachChunk c;
    c.ncx = (a.hi[0] >> 6) - (a.lo[0] >> 6) + 1;
    c.ncy = (a.hi[1] >> 6) - (a.lo[1] >> 6) + 1;
    c.ncz = (a.hi[2] >> 6) - (a.lo[2] >> 6) + 1;
    c.bx = (int)(b % (uint32_t)c.ncx);
    c.by = (int)((b / (uint32_t)c.ncx) % (uint32_t)c.ncy);
    c.bz = (int)(b / (uint32_t)(c.ncx * c.ncy));
    c.cx = (a.lo[0] >> 6) + c.bx;
    c.cy = (a.lo[1] >> 6) + c.by;
    c.cz = (a.lo[2] >> 6) + c.bz;
    c.n = (uint32_t)(c.ncx * c.ncy * c.ncz);
    return c;
}
__device__ __forceinline__ uint32_t* detach_flags(const DetachArgs& a) { return a.scratch + kDetachHeadWords; }
// bitmap `which` (0 occupancy, 1 + k reach buffer k) of box chunk b
__device__ __forceinline__ uint64_t* detach_bits(const DetachArgs& a, uint32_t n, uint32_t which, uint32_t b) {
    return reinterpret_cast<uint64_t*>(a.scratch + kDetachHeadWords + detach_flag_words(n) + kDetachChunkWords * ((size_t)which * n + b));
}

// the bits of `o` that a path of set bits of `o` joins to a bit of `s` (s within o): Kogge-Stone fills towards both ends
__device__ __forceinline__ uint64_t fill_x(uint64_t s, uint64_t o) {
    uint64_t f = s, p = o;
    f |= p & (f << 1);  p &= p << 1;
    f |= p & (f << 2);  p &= p << 2;
    f |= p & (f << 4);  p &= p << 4;
    f |= p & (f << 8);  p &= p << 8;
    f |= p & (f << 16); p &= p << 16;
    f |= p & (f << 32);
    p = o;
    f |= p & (f >> 1);  p &= p >> 1;
    f |= p & (f >> 2);  p &= p >> 2;
    f |= p & (f >> 4);  p &= p >> 4;
    f |= p & (f >> 8);  p &= p >> 8;
    f |= p & (f >> 16); p &= p >> 16;
    f |= p & (f >> 32);
    return f;
}

__global__ __launch_bounds__(kDetachWg) void k_detach_seed(const uint8_t* __restrict__ mine_sw, const uint32_t* __restrict__ mat_sw, DetachArgs a, int logr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lb = logr - 2;
    const DetachChunk c = detach_chunk(a, blockIdx.x);
    if (tid == 0) detach_flags(a)[blockIdx.x] = 0xFFFFFFFFu;
    if (blockIdx.x == 0 && tid < (int)kDetachHeadWords) a.scratch[tid] = 0u;   // the pass record and the spare result
    uint64_t* occ = detach_bits(a, c.n, 0u, blockIdx.x);
    uint64_t* seed = detach_bits(a, c.n, 1u, blockIdx.x);
    // the chunk's part of the box along x, as bits and as bricks
    const int xa = a.lo[0] - 64 * c.cx > 0 ? a.lo[0] - 64 * c.cx : 0, xb = a.hi[0] - 64 * c.cx < 63 ? a.hi[0] - 64 * c.cx : 63;
    const uint64_t xmask = (~0ull >> (63 - xb)) & (~0ull << xa);
    for (int k = 0; k < 4; k++) {
        // sixteen lanes (y & 3, z & 3) cover a brick's 64 bytes, a wave four bricks along y; the loop below walks sixteen bricks along x
        const int q = wave + 16 * k, zb = q >> 2, yb = 4 * (q & 3) + (lane >> 4), zl = (lane >> 2) & 3, yl = lane & 3;
        const int y = 4 * yb + yl, z = 4 * zb + zl, Y = 64 * c.cy + y, Z = 64 * c.cz + z;
        const bool inside = Y >= a.lo[1] && Y <= a.hi[1] && Z >= a.lo[2] && Z <= a.hi[2];
        uint64_t o = 0;
        if (inside) {
            uint32_t dw[16];
#pragma unroll
            for (int i = 0; i < 16; i++) {   // (a dword that lies outside the box along x is not read)
                const size_t brick = brick_index((uint32_t)(16 * c.cx + i), (uint32_t)(16 * c.cy + yb), (uint32_t)(16 * c.cz + zb), lb);
                dw[i] = (4 * i + 3 >= xa && 4 * i <= xb) ? *reinterpret_cast<const uint32_t*>(mine_sw + (brick << 6) + 16 * zl + 4 * yl) : 0xFFFFFFFFu;
            }
#pragma unroll
            for (int i = 0; i < 16; i++) {
#pragma unroll
                for (int j = 0; j < 4; j++) o |= (uint64_t)(((dw[i] >> (8 * j)) & 0xFFu) == 0u) << (4 * i + j);
            }
            o &= xmask;
        }
        uint64_t anc = 0;
        if (o != 0ull) {
            if ((a.anchor_faces & 1u) && (a.lo[0] >> 6) == c.cx) anc |= 1ull << (a.lo[0] & 63);
            if ((a.anchor_faces & 2u) && (a.hi[0] >> 6) == c.cx) anc |= 1ull << (a.hi[0] & 63);
            if (((a.anchor_faces & 4u) && Y == a.lo[1]) || ((a.anchor_faces & 8u) && Y == a.hi[1]) || ((a.anchor_faces & 16u) && Z == a.lo[2]) ||
                ((a.anchor_faces & 32u) && Z == a.hi[2]))
                anc = ~0ull;
            anc &= o;
            if (a.flags & RT_DETACH_ANCHOR_MATERIAL) {
                uint64_t m = o & ~anc;
                for (int i = 0; i < 64 && m != 0ull; i++) {   // at most 64 set bits
                    const int x = __builtin_ctzll(m);
                    m &= m - 1ull;
                    if ((mat_sw[swizzled_index(64 * c.cx + x, Y, Z, lb)] & a.anchor_mask) == a.anchor_value) anc |= 1ull << x;
                }
            }
        }
        occ[z * 64 + y] = o;
        seed[z * 64 + y] = anc;
    }
}

__global__ __launch_bounds__(kDetachWg) void k_detach_reach(DetachArgs a, uint32_t pass) {
    __shared__ uint64_t occ_s[kRows];     // 32 KiB
    __shared__ uint64_t reach_s[kRows];   // 32 KiB
    if (pass >= 2u && a.scratch[pass - 1u] == 0u) return;   // the process has ended (one address: the exit is the workgroup's)
    const int tid = threadIdx.x, y = tid & 63, wave = tid >> 6;
    const DetachChunk c = detach_chunk(a, blockIdx.x);
    const uint32_t b = blockIdx.x, from = 1u + ((pass - 1u) & 1u), to = 1u + (pass & 1u);
    const uint64_t* occ = detach_bits(a, c.n, 0u, b);
    const uint64_t* prev = detach_bits(a, c.n, from, b);
    // the neighbours' buffers of the previous pass, as dwords (low half of row r at 2 r); null at the box's faces
    const uint32_t sy = (uint32_t)c.ncx, sz = (uint32_t)(c.ncx * c.ncy);
    const uint32_t* nxm = c.bx > 0 ? reinterpret_cast<const uint32_t*>(detach_bits(a, c.n, from, b - 1u)) : nullptr;
    const uint32_t* nxp = c.bx + 1 < c.ncx ? reinterpret_cast<const uint32_t*>(detach_bits(a, c.n, from, b + 1u)) : nullptr;
    const uint64_t* nym = c.by > 0 ? detach_bits(a, c.n, from, b - sy) : nullptr;
    const uint64_t* nyp = c.by + 1 < c.ncy ? detach_bits(a, c.n, from, b + sy) : nullptr;
    const uint64_t* nzm = c.bz > 0 ? detach_bits(a, c.n, from, b - sz) : nullptr;
    const uint64_t* nzp = c.bz + 1 < c.ncz ? detach_bits(a, c.n, from, b + sz) : nullptr;

    uint64_t init[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int z = wave + 16 * k, r = z * 64 + y;
        const uint64_t o = occ[r];
        uint64_t s = prev[r];
        init[k] = s;
        if (nxm) s |= (uint64_t)(nxm[2 * r + 1] >> 31);
        if (nxp) s |= (uint64_t)(nxp[2 * r] & 1u) << 63;
        if (nym && y == 0) s |= nym[z * 64 + 63];
        if (nyp && y == 63) s |= nyp[z * 64];
        if (nzm && z == 0) s |= nzm[63 * 64 + y];
        if (nzp && z == 63) s |= nzp[y];
        occ_s[r] = o;
        reach_s[r] = s & o;
    }
    __syncthreads();

    for (int it = 0; it < kClosureCap; it++) {
        int changed = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int z = wave + 16 * k, r = z * 64 + y;
            const uint64_t o = occ_s[r];
            if (o == 0ull) continue;
            const uint64_t have = reach_s[r];
            uint64_t n = have;
            if (y > 0) n |= reach_s[r - 1];
            if (y < 63) n |= reach_s[r + 1];
            if (z > 0) n |= reach_s[r - 64];
            if (z < 63) n |= reach_s[r + 64];
            n = fill_x(n & o, o);
            if (n != have) { reach_s[r] = n; changed = 1; }
        }
        if (!__syncthreads_or(changed)) break;
    }

    uint64_t* out = detach_bits(a, c.n, to, b);
    int differs = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int r = (wave + 16 * k) * 64 + y;
        const uint64_t v = reach_s[r];   // (the thread's own rows: nobody else writes them)
        out[r] = v;
        differs |= v != init[k];
    }
    if (__syncthreads_or(differs) && tid == 0) a.scratch[pass] = 1u;   // (every writer stores the same value)
}

__global__ __launch_bounds__(kDetachWg) void k_detach_apply(uint8_t* mine_sw, uint32_t* mat_sw, DetachArgs a, int logr) {
    __shared__ uint64_t det_s[kRows];   // 32 KiB: the rows' detached bits
    __shared__ uint32_t s_end;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lb = logr - 2;
    const DetachChunk c = detach_chunk(a, blockIdx.x);
    if (tid == 0) s_end = 0xFFFFFFFFu;
    __syncthreads();
    if (tid < (int)a.max_passes && a.scratch[tid + 1] == 0u) atomicMin(&s_end, (uint32_t)tid + 1u);   // the first pass that changed nothing
    __syncthreads();
    const uint32_t end = s_end;
    const bool converged = end <= a.max_passes;
    if (blockIdx.x == 0 && tid == 0) {
        atomicAdd(a.result + 2, converged ? end : a.max_passes);
        if (!converged) atomicAdd(a.result + 3, 1u);
    }
    const uint64_t* occ = detach_bits(a, c.n, 0u, blockIdx.x);
    const uint64_t* reach = detach_bits(a, c.n, 1u + (end & 1u), blockIdx.x);
    const bool capture = (a.flags & RT_DETACH_CAPTURE) != 0u, carve = (a.flags & RT_DETACH_CARVE) != 0u;

    // ---- the rows' detached bits into LDS, a thread four rows (lane = y), with the sums and bounds of those rows ----------------------
    uint32_t ndet = 0, nsup = 0;
    int lo_x = INT32_MAX, lo_y = INT32_MAX, lo_z = INT32_MAX, hi_x = INT32_MIN, hi_y = INT32_MIN, hi_z = INT32_MIN;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int z = wave + 16 * k, r = z * 64 + lane, Y = 64 * c.cy + lane, Z = 64 * c.cz + z;
        uint64_t det = 0;
        if (converged) {   // (rows outside the box hold no occupied cell)
            const uint64_t o = occ[r], v = reach[r];
            det = o & ~v;
            nsup += (uint32_t)__popcll(o & v);
        }
        det_s[r] = det;
        if (det != 0ull) {
            ndet += (uint32_t)__popcll(det);
            const int x0 = 64 * c.cx + __builtin_ctzll(det), x1 = 64 * c.cx + 63 - __builtin_clzll(det);
            lo_x = x0 < lo_x ? x0 : lo_x; hi_x = x1 > hi_x ? x1 : hi_x;
            lo_y = Y < lo_y ? Y : lo_y;   hi_y = Y > hi_y ? Y : hi_y;
            lo_z = Z < lo_z ? Z : lo_z;   hi_z = Z > hi_z ? Z : hi_z;
        }
    }
    // sums and bounds per wave, one atomic per wave and field
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ndet += __shfl_xor(ndet, off);
        nsup += __shfl_xor(nsup, off);
        int t;
        t = __shfl_xor(lo_x, off); lo_x = t < lo_x ? t : lo_x;   t = __shfl_xor(hi_x, off); hi_x = t > hi_x ? t : hi_x;
        t = __shfl_xor(lo_y, off); lo_y = t < lo_y ? t : lo_y;   t = __shfl_xor(hi_y, off); hi_y = t > hi_y ? t : hi_y;
        t = __shfl_xor(lo_z, off); lo_z = t < lo_z ? t : lo_z;   t = __shfl_xor(hi_z, off); hi_z = t > hi_z ? t : hi_z;
    }
    if (lane == 0) {
        if (nsup) atomicAdd(a.result + 1, nsup);
        if (ndet) {
            atomicAdd(a.result + 0, ndet);
            int* bounds = reinterpret_cast<int*>(a.result);
            atomicMin(bounds + 4, lo_x); atomicMin(bounds + 5, lo_y); atomicMin(bounds + 6, lo_z);
            atomicMax(bounds + 8, hi_x); atomicMax(bounds + 9, hi_y); atomicMax(bounds + 10, hi_z);
        }
    }
    const int dirty = __syncthreads_or(ndet != 0u);   // (also the barrier between the rows' writers and their readers)
    if (dirty && tid == 0) {
        atomicAdd(a.result + 7, 1u);
        if (carve) detach_flags(a)[blockIdx.x] = 0u;
    }
    if (!capture && !(carve && dirty)) return;

    // ---- the cells: a wave a row at a time, lane = x; nothing here waits for a store ------------------------------------------------
    const int X = 64 * c.cx + lane;
    if (X < a.lo[0] || X > a.hi[0]) return;
    const int ex = a.hi[0] - a.lo[0] + 1, ey = a.hi[1] - a.lo[1] + 1;
    // the chunk's rows inside the box
    const int y0 = a.lo[1] - 64 * c.cy > 0 ? a.lo[1] - 64 * c.cy : 0, y1 = a.hi[1] - 64 * c.cy < 63 ? a.hi[1] - 64 * c.cy : 63;
    const int z0 = a.lo[2] - 64 * c.cz > 0 ? a.lo[2] - 64 * c.cz : 0, z1 = a.hi[2] - 64 * c.cz < 63 ? a.hi[2] - 64 * c.cz : 63;
    for (int z = z0 + wave; z <= z1; z += 16) {
        const int Z = 64 * c.cz + z;
#pragma unroll 4
        for (int y = y0; y <= y1; y++) {
            const uint64_t det = det_s[z * 64 + y];
            if (det == 0ull && !capture) continue;
            const int Y = 64 * c.cy + y;
            const bool mine = ((det >> lane) & 1ull) != 0ull;
            const uint32_t idx = swizzled_index(X, Y, Z, lb);
            if (capture) {
                const size_t d = ((size_t)(Z - a.lo[2]) * (size_t)ey + (size_t)(Y - a.lo[1])) * (size_t)ex + (size_t)(X - a.lo[0]);
                a.stamp_mats[d] = mine ? mat_sw[idx] : 0u;
                a.stamp_state[d] = mine ? (uint8_t)RT_STAMP_SOLID : (uint8_t)RT_STAMP_ABSENT;
            }
            if (carve && mine) {
                mine_sw[idx] = 1u;
                mat_sw[idx] = a.air_material;
            }
        }
    }
}

// the chunk rebuild's edit stage of a call whose edits the apply pass has already written
struct NoStage {
    __device__ __forceinline__ void operator()(uint32_t*, uint32_t, uint32_t, uint32_t, int, int) const {}
};

// One workgroup per chunk of the box, in the order of the chunk list.  The flag word is read by every thread (one address: a uniform
// value), so the exit is the workgroup's.
__global__ __launch_bounds__(1024) void k_detach_chunks(uint8_t* __restrict__ mine_sw, const uint32_t* __restrict__ chunks, DetachArgs a, int logr) {
    if (detach_flags(a)[blockIdx.x] != 0u) return;   // no detached voxel in this chunk: its bytes stay as they are
    rebuild_chunk(mine_sw, chunks, logr, NoStage{});
}

}  // namespace

hipError_t launch_detach_voxels(uint8_t* mine_sw, uint32_t* mat_sw, const uint32_t* chunks, uint32_t nchunks, int logr, const DetachArgs& a,
                                hipStream_t st) {
    if (logr < 8 || logr > 10 || nchunks < 1u || !a.scratch || !a.result || a.max_passes < 1u || a.max_passes > kDetachMaxPasses ||
        a.anchor_faces > 63u || (a.flags & ~(RT_DETACH_CARVE | RT_DETACH_CAPTURE | RT_DETACH_ANCHOR_MATERIAL)) != 0u)
        return hipErrorInvalidValue;
    const bool capture = (a.flags & RT_DETACH_CAPTURE) != 0u, carve = (a.flags & RT_DETACH_CARVE) != 0u;
    if (capture != (a.stamp_mats != nullptr) || capture != (a.stamp_state != nullptr) || (carve && !chunks)) return hipErrorInvalidValue;
    uint64_t boxchunks = 1;
    for (int k = 0; k < 3; k++) {
        if (a.lo[k] < 0 || a.hi[k] >= (1 << logr) || a.lo[k] > a.hi[k] || a.hi[k] - a.lo[k] >= 256) return hipErrorInvalidValue;
        boxchunks *= (uint64_t)((a.hi[k] >> 6) - (a.lo[k] >> 6) + 1);
    }
    if (boxchunks != nchunks) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_detach_seed, dim3(nchunks), dim3(kDetachWg), 0, st, mine_sw, mat_sw, a, logr);
    hipError_t e = hipGetLastError();
    for (uint32_t p = 1; p <= a.max_passes && e == hipSuccess; p++) {
        hipLaunchKernelGGL(k_detach_reach, dim3(nchunks), dim3(kDetachWg), 0, st, a, p);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_detach_apply, dim3(nchunks), dim3(kDetachWg), 0, st, mine_sw, mat_sw, a, logr);
    e = hipGetLastError();
    if (e != hipSuccess || !carve) return e;
    hipLaunchKernelGGL(k_detach_chunks, dim3(nchunks), dim3(1024), 0, st, mine_sw, chunks, a, logr);
    return hipGetLastError();
}

}  // namespace rtd
