// rt_rebuild_chunk.hpp — the rebuild of one 64^3 chunk's minefield by one workgroup, shared by the kernels that edit the resident
// world: rt_edit.hip (rt_edit_voxels, rt_edit_shapes, rt_edit_stamps) and rt_deposit.hip (rt_deposit_particles).  The chunk's
// occupancy (minefield == 0) is loaded into an LDS bitmap, an edit stage changes it, the OR pyramid of levels 1..6 is built and the
// chunk's whole minefield is written back with pack_into's rule (src/world/chunk.rs:125-184).  One definition: every kind of edit
// leaves the bytes rt_edit_voxels would.
#pragma once

#include <hip/hip_runtime.h>

#include "rt_device.hpp"
#include "rt_world.hpp"

namespace rtd {

// Occupancy rows of level 0: row (z, y) of the chunk is 64 bits (x = bit), two dwords at 2 * (z * 65 + y).  The pad of one row per
// z keeps the four z-layers a wave reads in the write-back pass (rows 65 * 2 dwords apart) on different banks.
constexpr int kRow0Stride = 65;
// Level 1 (32^3 cells of 2^3 voxels): row (Z, Y) is 32 bits at Z * 33 + Y.
constexpr int kRow1Stride = 33;

__device__ __forceinline__ uint64_t occ_row0(const uint32_t* occ0, int z, int y) {
    const int w = 2 * (z * kRow0Stride + y);
    return (uint64_t)occ0[w] | ((uint64_t)occ0[w + 1] << 32);
}

// bit X of the result = bit 2X | bit 2X + 1 of v (64 -> 32 bits)
__device__ __forceinline__ uint32_t or_pairs64(uint64_t v) {
    uint64_t t = (v | (v >> 1)) & 0x5555555555555555ull;
    t = (t | (t >> 1)) & 0x3333333333333333ull;
    t = (t | (t >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    t = (t | (t >> 4)) & 0x00FF00FF00FF00FFull;
    t = (t | (t >> 8)) & 0x0000FFFF0000FFFFull;
    t = (t | (t >> 16)) & 0x00000000FFFFFFFFull;
    return (uint32_t)t;
}

// The rebuild of one chunk by one workgroup of 1024 threads (16 waves): chunks[blockIdx.x] = (cz * n + cy) * n + cx with n = R / 64
// chunks per axis.  `stage(occ0, cx, cy, cz, lb, tid)` is the edit stage: it runs between two barriers on the loaded level 0
// bitmap, changes its bits and stores the material words of what it changes.  Chunks are distinct, so workgroups never touch the
// same bytes.
template <typename Stage>
__device__ __forceinline__ void rebuild_chunk(uint8_t* __restrict__ mine_sw, const uint32_t* __restrict__ chunks, int logr, const Stage& stage) {
    __shared__ uint32_t occ0[2 * 64 * kRow0Stride];   // 33280 B: level 0 bitmap
    __shared__ uint32_t occ1[32 * kRow1Stride];       //  4224 B: level 1 rows
    __shared__ uint8_t occ2[16 * 16 * 16];            //  4096 B: levels 2..5, one byte per cell
    __shared__ uint8_t occ3[8 * 8 * 8];
    __shared__ uint8_t occ4[4 * 4 * 4];
    __shared__ uint8_t occ5[2 * 2 * 2];
    __shared__ uint8_t bval[16 * 16 * 16];            //  4096 B: per 4^3 brick (= level 2 cell): first level 2..6 that is occupied

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lb = logr - 2, nl = logr - 6;
    const uint32_t cid = chunks[blockIdx.x], cmask = (1u << nl) - 1u;
    const uint32_t cx = cid & cmask, cy = (cid >> nl) & cmask, cz = cid >> (2 * nl);
    // a wave covers one row of 16 x-adjacent bricks (1 KiB contiguous): lane = brick bx * 4 + z-layer zl, 16 bytes each
    const int bx = lane >> 2, zl = lane & 3;

    // ---- load: occupancy of the resident minefield, 16 ballots per 1 KiB row ---------------------------------------------
    for (int q = wave; q < 256; q += 16) {
        const int bz = q >> 4, by = q & 15;
        const size_t brick = brick_index(cx * 16u + bx, cy * 16u + by, cz * 16u + bz, lb);
        const uint4 v = *reinterpret_cast<const uint4*>(mine_sw + (brick << 6) + zl * 16);
        const uint32_t dw[4] = {v.x, v.y, v.z, v.w};
        uint64_t ball[16];
#pragma unroll
        for (int k = 0; k < 16; k++) ball[k] = __ballot(((dw[k >> 2] >> (8 * (k & 3))) & 0xFFu) == 0u);
        // byte k = y&3 * 4 + x&3 of lane (bx, zl) -> bit 4 bx + x&3 of row (4 bz + zl, 4 by + y&3)
        if (lane < 16) {
            const int rz = lane >> 2, r = lane & 3;
            uint64_t row = 0;
#pragma unroll
            for (int xi = 0; xi < 4; xi++) {   // (selects with constant indices: a lane-dependent index would put ball[] in scratch)
                const uint64_t b = r == 0 ? ball[xi] : r == 1 ? ball[4 + xi] : r == 2 ? ball[8 + xi] : ball[12 + xi];
                row |= ((b >> rz) & 0x1111111111111111ull) << xi;
            }
            const int w = 2 * ((4 * bz + rz) * kRow0Stride + 4 * by + r);
            occ0[w] = (uint32_t)row;
            occ0[w + 1] = (uint32_t)(row >> 32);
        }
    }
    __syncthreads();

    // ---- edits: material words to the region, solid bits to the bitmap -------------------------------------------------
    stage(occ0, cx, cy, cz, lb, tid);
    __syncthreads();

    // ---- OR pyramid ----------------------------------------------------------------------------------------------------
    {   // level 1: 32 x 32 rows, one per thread
        const int Z = tid >> 5, Y = tid & 31;
        const uint64_t v = occ_row0(occ0, 2 * Z, 2 * Y) | occ_row0(occ0, 2 * Z, 2 * Y + 1) | occ_row0(occ0, 2 * Z + 1, 2 * Y) |
                           occ_row0(occ0, 2 * Z + 1, 2 * Y + 1);
        occ1[Z * kRow1Stride + Y] = or_pairs64(v);
    }
    __syncthreads();
    for (int c = tid; c < 4096; c += 1024) {   // level 2
        const int X = c & 15, Y = (c >> 4) & 15, Z = c >> 8;
        const uint32_t v = occ1[(2 * Z) * kRow1Stride + 2 * Y] | occ1[(2 * Z) * kRow1Stride + 2 * Y + 1] |
                           occ1[(2 * Z + 1) * kRow1Stride + 2 * Y] | occ1[(2 * Z + 1) * kRow1Stride + 2 * Y + 1];
        occ2[c] = ((v >> (2 * X)) & 3u) != 0u;
    }
    __syncthreads();
    if (tid < 512) {   // level 3
        const int X = tid & 7, Y = (tid >> 3) & 7, Z = tid >> 6;
        uint32_t any = 0;
        for (int k = 0; k < 8; k++) any |= occ2[((2 * Z + (k >> 2)) << 8) | ((2 * Y + ((k >> 1) & 1)) << 4) | (2 * X + (k & 1))];
        occ3[tid] = any != 0u;
    }
    __syncthreads();
    if (tid < 64) {    // level 4
        const int X = tid & 3, Y = (tid >> 2) & 3, Z = tid >> 4;
        uint32_t any = 0;
        for (int k = 0; k < 8; k++) any |= occ3[((2 * Z + (k >> 2)) << 6) | ((2 * Y + ((k >> 1) & 1)) << 3) | (2 * X + (k & 1))];
        occ4[tid] = any != 0u;
    }
    __syncthreads();
    if (tid < 8) {     // level 5 (level 6 needs no table: it is the fallback value below)
        const int X = tid & 1, Y = (tid >> 1) & 1, Z = tid >> 2;
        uint32_t any = 0;
        for (int k = 0; k < 8; k++) any |= occ4[((2 * Z + (k >> 2)) << 4) | ((2 * Y + ((k >> 1) & 1)) << 2) | (2 * X + (k & 1))];
        occ5[tid] = any != 0u;
    }
    __syncthreads();
    for (int c = tid; c < 4096; c += 1024) {   // a brick's voxels that are not within a level-1 cell of a solid one
        const int X = c & 15, Y = (c >> 4) & 15, Z = c >> 8;
        uint32_t v = 6;
        if (occ5[((Z >> 3) << 2) | ((Y >> 3) << 1) | (X >> 3)]) v = 5;
        if (occ4[((Z >> 2) << 4) | ((Y >> 2) << 2) | (X >> 2)]) v = 4;
        if (occ3[((Z >> 1) << 6) | ((Y >> 1) << 3) | (X >> 1)]) v = 3;
        if (occ2[c]) v = 2;
        bval[c] = (uint8_t)v;
    }
    __syncthreads();

    // ---- write-back: the whole chunk's minefield, one dword4 (a z-layer of a brick) per lane -----------------------------
    for (int q = wave; q < 256; q += 16) {
        const int bz = q >> 4, by = q & 15;
        const int z = 4 * bz + zl;
        const uint32_t bv = bval[(bz << 8) | (by << 4) | bx];
        uint32_t dw[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int y = 4 * by + r;
            const uint32_t l0 = (uint32_t)(occ_row0(occ0, z, y) >> (4 * bx)) & 0xFu;
            const uint32_t l1 = (occ1[(z >> 1) * kRow1Stride + (y >> 1)] >> (2 * bx)) & 3u;
            uint32_t d = 0;
#pragma unroll
            for (int xi = 0; xi < 4; xi++) {
                const uint32_t b = ((l0 >> xi) & 1u) ? 0u : (((l1 >> (xi >> 1)) & 1u) ? 1u : bv);
                d |= b << (8 * xi);
            }
            dw[r] = d;
        }
        const size_t brick = brick_index(cx * 16u + bx, cy * 16u + by, cz * 16u + bz, lb);
        *reinterpret_cast<uint4*>(mine_sw + (brick << 6) + zl * 16) = make_uint4(dw[0], dw[1], dw[2], dw[3]);
    }
}

}  // namespace rtd
