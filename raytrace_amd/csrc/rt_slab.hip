// rt_slab.hip — gfx950 kernels of RtConfig.stream_history: what a streamed slab can have changed of the light, found on the device.
//
//   k_slab_occupancy<LOGR> : the 16-thick slab at texel `offset` of `axis` is 4 (R/4)^2 bricks of the brick-swizzled minefield, 64
//                            bytes each.  One lane per brick, grid-stride: four 16-byte loads (a layer of 4 x 4 voxels each), a
//                            zero-byte test per word (a voxel is occupied when its byte is 0: the shader's hit test), and the
//                            brick's three nibbles — which of its 4 x, y and z coordinates hold an occupied voxel.  A workgroup ORs
//                            them into three rows of R bits in LDS — it looks at the word first and skips the atomic where the
//                            bits are set already, which after a workgroup's first bricks is nearly always — and flushes the
//                            non-zero words with one device-scope atomicOr each.  Launched twice per slab, round the launch that
//                            writes it: the masks of what left and of what arrived.  Reads 1 byte per voxel.
//   k_place_slab_boxes     : one workgroup in front of the frame's temporal pass.  For each pending slot, in call order, the old
//                            masks are placed with the previous frame's lr and the new ones with this frame's: per set bit
//                            w(t) = lr - R/2 + (t - lr) mod R in 64-bit integers, so that a content on both sides of the window's
//                            seam gets its tight box, the box being [min w, max w + 1] per axis (two runs per mask word at most:
//                            w rises with t but for the seam).  A set without a bit gives no box; the others are compacted, at
//                            most kSlabMaxBoxes, behind their count.
#include <hip/hip_runtime.h>

#include "rt_kernels.hpp"
#include "rt_world.hpp"

namespace rtd {

namespace {

constexpr uint32_t kSlabWg = 256;

// 0x80 in every byte of v that is 0, nothing else (no borrow between bytes)
__device__ __forceinline__ uint32_t zero_bytes(uint32_t v) {
    return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu);
}

// rows[w] |= bits, without the atomic where a look shows them set (bits only ever appear: a stale look costs one atomic)
__device__ __forceinline__ void lds_or(uint32_t* rows, uint32_t w, uint32_t bits) {
    if (bits != 0u && (*(volatile uint32_t*)&rows[w] & bits) != bits) atomicOr(&rows[w], bits);
}

}  // namespace

template <int LOGR>
__global__ __launch_bounds__(kSlabWg) void k_slab_occupancy(const uint8_t* __restrict__ mine_sw, int axis, int offset,
                                                            uint32_t* __restrict__ masks) {
    constexpr int LB = LOGR - 2;
    constexpr uint32_t kBricks = 4u << (2 * LB);
    __shared__ uint32_t rows[kSlabSetWords];
    if (threadIdx.x < kSlabSetWords) rows[threadIdx.x] = 0u;
    __syncthreads();
    // the slab's bricks in memory order: x fastest, 4 of them along the slab's own axis
    const int sx = axis == 0 ? 2 : LB, sy = axis == 1 ? 2 : LB;
    const uint32_t first = (uint32_t)offset >> 2;
    for (uint32_t b = blockIdx.x * kSlabWg + threadIdx.x; b < kBricks; b += gridDim.x * kSlabWg) {
        const uint32_t bx = (b & ((1u << sx) - 1u)) + (axis == 0 ? first : 0u);
        const uint32_t by = ((b >> sx) & ((1u << sy) - 1u)) + (axis == 1 ? first : 0u);
        const uint32_t bz = (b >> (sx + sy)) + (axis == 2 ? first : 0u);
        const Brick k = load_brick(mine_sw, brick_index(bx, by, bz, LB));
        // a layer (iz & 3) is one uint4, its component iy & 3, the byte in it ix & 3 (swizzled_index)
        const uint4 za = make_uint4(zero_bytes(k.a.x), zero_bytes(k.a.y), zero_bytes(k.a.z), zero_bytes(k.a.w));
        const uint4 zq = make_uint4(zero_bytes(k.q.x), zero_bytes(k.q.y), zero_bytes(k.q.z), zero_bytes(k.q.w));
        const uint4 zd = make_uint4(zero_bytes(k.d.x), zero_bytes(k.d.y), zero_bytes(k.d.z), zero_bytes(k.d.w));
        const uint4 ze = make_uint4(zero_bytes(k.e.x), zero_bytes(k.e.y), zero_bytes(k.e.z), zero_bytes(k.e.w));
        const uint32_t y0 = za.x | zq.x | zd.x | ze.x, y1 = za.y | zq.y | zd.y | ze.y;
        const uint32_t y2 = za.z | zq.z | zd.z | ze.z, y3 = za.w | zq.w | zd.w | ze.w;
        const uint32_t z0 = za.x | za.y | za.z | za.w, z1 = zq.x | zq.y | zq.z | zq.w;
        const uint32_t z2 = zd.x | zd.y | zd.z | zd.w, z3 = ze.x | ze.y | ze.z | ze.w;
        const uint32_t xs = y0 | y1 | y2 | y3;   // 0x80 << 8 j: some voxel with ix & 3 == j
        const uint32_t xn = ((xs >> 7) & 1u) | ((xs >> 14) & 2u) | ((xs >> 21) & 4u) | ((xs >> 28) & 8u);
        const uint32_t yn = (y0 ? 1u : 0u) | (y1 ? 2u : 0u) | (y2 ? 4u : 0u) | (y3 ? 8u : 0u);
        const uint32_t zn = (z0 ? 1u : 0u) | (z1 ? 2u : 0u) | (z2 ? 4u : 0u) | (z3 ? 8u : 0u);
        // texel 4 bx + j is bit (bx & 7) * 4 + j of word bx >> 3: a nibble never crosses a word
        lds_or(rows + 0 * kSlabMaskWords, bx >> 3, xn << ((bx & 7u) * 4u));
        lds_or(rows + 1 * kSlabMaskWords, by >> 3, yn << ((by & 7u) * 4u));
        lds_or(rows + 2 * kSlabMaskWords, bz >> 3, zn << ((bz & 7u) * 4u));
    }
    __syncthreads();
    if (threadIdx.x < kSlabSetWords) {
        const uint32_t v = rows[threadIdx.x];
        if (v != 0u) atomicOr(&masks[threadIdx.x], v);
    }
}

hipError_t launch_slab_occupancy(const uint8_t* mine_sw, int logr, int axis, int offset, uint32_t* masks, hipStream_t st) {
    const int R = 1 << logr;
    if (logr < 8 || logr > 10 || axis < 0 || axis > 2 || offset < 0 || offset % RT_SLICE_SIZE != 0 || offset + RT_SLICE_SIZE > R)
        return hipErrorInvalidValue;
    const uint32_t bricks = 4u << (2 * (logr - 2));
    const uint32_t blocks = bricks / kSlabWg < 512u ? bricks / kSlabWg : 512u;
    const dim3 grid(blocks), block(kSlabWg);
    if (logr == 8) hipLaunchKernelGGL((k_slab_occupancy<8>), grid, block, 0, st, mine_sw, axis, offset, masks);
    else if (logr == 9) hipLaunchKernelGGL((k_slab_occupancy<9>), grid, block, 0, st, mine_sw, axis, offset, masks);
    else hipLaunchKernelGGL((k_slab_occupancy<10>), grid, block, 0, st, mine_sw, axis, offset, masks);
    return hipGetLastError();
}

// Thread (c, j) = (tid / 32, tid % 32) takes word j of the three rows of candidate c = 2 slot + set.  w(t) rises with t except
// across the seam (texel lr mod R, where it is lowest), so a word is at most two runs — the texels below the seam and those from
// it on — and the lowest and highest set bit of each run give the word's extremes.  The 32 lanes of a candidate (half a wave) fold
// each axis with shuffles; thread 0 compacts.
__global__ __launch_bounds__(kSlabWg) void k_place_slab_boxes(const uint32_t* __restrict__ masks, uint32_t nslots, int3 lr_prev,
                                                              int3 lr_cur, int logr, SlabBoxes* __restrict__ out) {
    __shared__ long long blo[kSlabMaxBoxes][3], bhi[kSlabMaxBoxes][3];
    const uint32_t c = threadIdx.x / kSlabMaskWords, j = threadIdx.x % kSlabMaskWords;
    const long long R = 1ll << logr;
    const int3 lr3 = (c & 1u) ? lr_cur : lr_prev;
    const int lr[3] = {lr3.x, lr3.y, lr3.z};
    const bool live = c < 2u * nslots && j < (uint32_t)(R >> 5);
    for (int a = 0; a < 3; a++) {
        long long l = LLONG_MAX, h = LLONG_MIN;
        const uint32_t word = live ? masks[c * kSlabSetWords + (uint32_t)a * kSlabMaskWords + j] : 0u;
        const long long base = (long long)lr[a] - R / 2, t0 = (long long)(j * 32u);
        const long long seam = (long long)lr[a] & (R - 1);                       // (R a power of two: the non-negative mod)
        const long long cut = seam - t0 < 0 ? 0 : (seam - t0 > 32 ? 32 : seam - t0);   // bits of the word below the seam
        const uint32_t below = cut >= 32 ? 0xFFFFFFFFu : ((1u << (uint32_t)cut) - 1u);
        const uint32_t runs[2] = {word & below, word & ~below};
        for (int r = 0; r < 2; r++) {
            if (runs[r] == 0u) continue;
            const long long first = t0 + (long long)__builtin_ctz(runs[r]), last = t0 + 31 - (long long)__builtin_clz(runs[r]);
            const long long wl = base + ((first - (long long)lr[a]) & (R - 1)), wh = base + ((last - (long long)lr[a]) & (R - 1));
            l = wl < l ? wl : l;
            h = wh > h ? wh : h;
        }
        for (int off = (int)kSlabMaskWords / 2; off > 0; off >>= 1) {
            const long long ol = __shfl_xor(l, off, (int)kSlabMaskWords), oh = __shfl_xor(h, off, (int)kSlabMaskWords);
            l = ol < l ? ol : l;
            h = oh > h ? oh : h;
        }
        if (j == 0u) { blo[c][a] = l; bhi[c][a] = h; }
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t n = 0;
        for (uint32_t k = 0; k < 2u * nslots; k++) {
            if (blo[k][0] > bhi[k][0]) continue;   // (no occupied voxel: no bit on any axis)
            TemporalBox& x = out->box[n++];
            for (int a = 0; a < 3; a++) { x.lo[a] = (float)blo[k][a]; x.hi[a] = (float)(bhi[k][a] + 1); }
        }
        out->count = n;
    }
}

hipError_t launch_place_slab_boxes(const uint32_t* masks, uint32_t nslots, const int32_t lr_prev[3], const int32_t lr_cur[3], int logr,
                                   SlabBoxes* out, hipStream_t st) {
    static_assert(kSlabWg == kSlabMaxBoxes * kSlabMaskWords, "one thread per candidate and mask word");
    if (nslots < 1u || nslots > kSlabSlots || logr < 8 || logr > 10) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_place_slab_boxes, dim3(1), dim3(kSlabWg), 0, st, masks, nslots, make_int3(lr_prev[0], lr_prev[1], lr_prev[2]),
                       make_int3(lr_cur[0], lr_cur[1], lr_cur[2]), logr, out);
    return hipGetLastError();
}

}  // namespace rtd
