// rt_edit.hip — gfx950 kernels of rt_edit_voxels, rt_edit_shapes and the voxel stamps (rt_edit_stamps, rt_stamp_capture).
//
//   k_rebuild_chunks   : one workgroup per touched 64^3 chunk: scatters the chunk's edited material words, loads its occupancy
//                        (minefield == 0) into an LDS bitmap, applies the edits' solid bits, builds the OR pyramid of levels 1..6
//                        and writes the chunk's whole minefield back with pack_into's rule (src/world/chunk.rs:125-184)
//   k_shape_chunks     : the same chunk rebuild (rebuild_chunk, rt_rebuild_chunk.hpp) with another edit stage: the batch's boxes and spheres, applied in
//                        order to the bitmap rows a thread owns, their material words stored by that thread
//   k_stamp_chunks     : the chunk rebuild with a third edit stage: the batch's stamp placements, each a dense box of voxels read
//                        from the stamp's own arrays through three strides (any of the 48 axis orientations)
//   k_stamp_capture    : rt_stamp_capture: a box of the region un-tiled into a stamp's arrays, minefield bytes turned into states
//   k_stamp_clean      : rt_stamp_create: the material words of ABSENT voxels cleared
//   k_rebuild_chunk_maps: the coarse (and, above R = 256, brick) nibble-map words that cover the touched chunks (rt_world.hpp's rule)
#include <hip/hip_runtime.h>

#include "rt_device.hpp"
#include "rt_kernels.hpp"
#include "rt_rebuild_chunk.hpp"
#include "rt_shape_rows.hpp"
#include "rt_world.hpp"

namespace rtd {

namespace {

// rt_edit_voxels' edit stage.  The chunk's edits are recs[offs[i] .. offs[i + 1]): .x = local index (z << 12 | y << 6 | x) |
// solid << 18, .y = material word, each voxel at most once (the host keeps the last edit of a voxel).
struct RecordStage {
    uint32_t* __restrict__ mat_sw;
    const uint32_t* __restrict__ offs;
    const uint2* __restrict__ recs;
    __device__ __forceinline__ void operator()(uint32_t* occ0, uint32_t cx, uint32_t cy, uint32_t cz, int lb, int tid) const {
        const uint32_t e0 = offs[blockIdx.x], e1 = offs[blockIdx.x + 1];
        for (uint32_t e = e0 + tid; e < e1; e += 1024u) {
            const uint2 rec = recs[e];
            const int x = rec.x & 63u, y = (rec.x >> 6) & 63u, z = (rec.x >> 12) & 63u;
            const int w = 2 * (z * kRow0Stride + y) + (x >> 5);
            const uint32_t bit = 1u << (x & 31);
            if (rec.x & (1u << 18)) atomicOr(&occ0[w], bit);
            else atomicAnd(&occ0[w], ~bit);
            mat_sw[swizzled_index((int)(cx * 64u) + x, (int)(cy * 64u) + y, (int)(cz * 64u) + z, lb)] = rec.y;
        }
    }
};

// the least |2 x + 1 - a| over the 64 texels x0 .. x0 + 63
__device__ __forceinline__ int sphere_gap(int a, int x0) {
    const int lo = 2 * x0 + 1, hi = 2 * x0 + 127;
    return a < lo ? lo - a : a > hi ? a - hi : 1 - (a & 1);
}

// rt_edit_shapes' edit stage.  shapes[2 s], shapes[2 s + 1] = RtShapeEdit s as two dword4: (a, material), (b, kind | where << 8 |
// solid << 16).  Thread t owns the rows (z, y) = ((t >> 6) + 16 j, t & 63), j = 0..3, for EVERY shape: it keeps them in registers
// through the batch, so the bitmap needs no atomics, and every store to a voxel's material word comes from that one thread in
// program order — the last shape wins.  The loop and a shape's fields are uniform across the workgroup (scalar loads).
struct ShapeStage {
    uint32_t* __restrict__ mat_sw;
    const int4* __restrict__ shapes;
    uint32_t nshapes;
    __device__ __forceinline__ void operator()(uint32_t* occ0, uint32_t cx, uint32_t cy, uint32_t cz, int lb, int tid) const {
        const int x0 = (int)(cx * 64u), y0 = (int)(cy * 64u), z0 = (int)(cz * 64u);
        const int ly = tid & 63, lz = tid >> 6, y = y0 + ly;
        uint64_t row[4];
#pragma unroll
        for (int j = 0; j < 4; j++) row[j] = occ_row0(occ0, lz + 16 * j, ly);
        for (uint32_t s = 0; s < nshapes; s++) {
            const int4 p = shapes[2u * s], q = shapes[2u * s + 1u];
            const uint32_t kind = (uint32_t)q.w & 0xFFu, where = ((uint32_t)q.w >> 8) & 0xFFu;
            const bool solid = (((uint32_t)q.w >> 16) & 0xFFu) != 0u;
            const uint32_t material = (uint32_t)p.w;
            // a shape whose bounding box misses the chunk selects nothing in it
            if (kind == 0u) {
                if (p.x > x0 + 63 || q.x < x0 || p.y > y0 + 63 || q.y < y0 || p.z > z0 + 63 || q.z < z0) continue;
            } else {
                const int gx = sphere_gap(p.x, x0), gy = sphere_gap(p.y, y0), gz = sphere_gap(p.z, z0);
                if (gx * gx > q.x || gy * gy > q.x || gz * gz > q.x) continue;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int z = z0 + lz + 16 * j;
                const uint64_t m = shape_row(kind, p, q, x0, y, z);   // (rt_shape_rows.hpp: the one membership rule)
                uint64_t sel = where == 0u ? m : where == 1u ? (m & row[j]) : (m & ~row[j]);
                row[j] = solid ? (row[j] | sel) : (row[j] & ~sel);
                // material words: the four x of one brick are 16 contiguous bytes of the swizzled array
                while (sel) {
                    const int g = (int)(__ffsll((unsigned long long)sel) - 1) >> 2;
                    const uint32_t nib = (uint32_t)(sel >> (4 * g)) & 0xFu;
                    uint32_t* dst = mat_sw + swizzled_index(x0 + 4 * g, y, z, lb);
                    if (nib == 0xFu) {
                        *reinterpret_cast<uint4*>(dst) = make_uint4(material, material, material, material);
                    } else {
#pragma unroll
                        for (int xi = 0; xi < 4; xi++)
                            if ((nib >> xi) & 1u) dst[xi] = material;
                    }
                    sel &= ~(0xFull << (4 * g));
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int w = 2 * ((lz + 16 * j) * kRow0Stride + ly);
            occ0[w] = (uint32_t)row[j];
            occ0[w + 1] = (uint32_t)(row[j] >> 32);
        }
    }
};

// rt_edit_stamps' edit stage.  recs[4 s .. 4 s + 3] = the placement's 64-byte record as four dword4 (api/edit_stamps.hpp,
// StampRecord): (mats, state: two device addresses), (lo.x, lo.y, lo.z, hi.x), (hi.y, hi.z, stride.x, stride.y), (stride.z, base,
// where, -).  The box lo..hi is the placement's bounding box in world texels, inclusive; world texel w of it shows stamp voxel
// base + sum_k stride[k] * w[k] of the stamp's [ez][ey][ex] arrays (state 0 absent, 1 air, 2 solid).  Rows and ordering are
// ShapeStage's: thread t owns the rows (z, y) = ((t >> 6) + 16 j, t & 63) for EVERY placement and issues every material store of its
// rows in program order, so the bitmap needs no atomics and the last placement wins.  The loop over the placements that meet the
// chunk and a placement's fields are uniform across the workgroup (scalar loads); per row the source index advances by stride.x per voxel.  States are one
// byte per voxel, gathered with that stride whatever the orientation (DESIGN.md "Voxel stamps" on the bit planes that were not built).
struct StampStage {
    uint32_t* __restrict__ mat_sw;
    const int4* __restrict__ recs;
    uint32_t nrecs;
    __device__ __forceinline__ void operator()(uint32_t* occ0, uint32_t cx, uint32_t cy, uint32_t cz, int lb, int tid) const {
        const int x0 = (int)(cx * 64u), y0 = (int)(cy * 64u), z0 = (int)(cz * 64u);
        const int ly = tid & 63, lz = tid >> 6, y = y0 + ly;
        uint64_t row[4];
#pragma unroll
        for (int j = 0; j < 4; j++) row[j] = occ_row0(occ0, lz + 16 * j, ly);
        // Which placements meet the chunk: one placement per thread and pass, a bit each in LDS.  (Walking the records one after the
        // other instead costs every workgroup one scalar-cache miss per placement, most of them for a box that misses the chunk.)
        __shared__ uint32_t hit[4096 / 32];
        const uint32_t nwords = (nrecs + 31u) >> 5;
        for (uint32_t w = (uint32_t)tid; w < nwords; w += 1024u) hit[w] = 0u;
        __syncthreads();
        for (uint32_t s = (uint32_t)tid; s < nrecs; s += 1024u) {
            const int4 q1 = recs[4u * s + 1u], q2 = recs[4u * s + 2u];
            // a placement whose bounding box misses the chunk selects nothing in it
            if (!(q1.x > x0 + 63 || q1.w < x0 || q1.y > y0 + 63 || q2.x < y0 || q1.z > z0 + 63 || q2.y < z0)) atomicOr(&hit[s >> 5], 1u << (s & 31u));
        }
        __syncthreads();
        for (uint32_t w = 0; w < nwords; w++)
        for (uint32_t bits = __builtin_amdgcn_readfirstlane(hit[w]); bits; bits &= bits - 1u) {
            const uint32_t s = 32u * w + (uint32_t)__builtin_ctz(bits);   // in batch order
            const int4 q1 = recs[4u * s + 1u], q2 = recs[4u * s + 2u];
            const int4 q0 = recs[4u * s], q3 = recs[4u * s + 3u];
            const uint32_t* __restrict__ mats = reinterpret_cast<const uint32_t*>(((uint64_t)(uint32_t)q0.y << 32) | (uint64_t)(uint32_t)q0.x);
            const uint8_t* __restrict__ state = reinterpret_cast<const uint8_t*>(((uint64_t)(uint32_t)q0.w << 32) | (uint64_t)(uint32_t)q0.z);
            const int sx = q2.z, sy = q2.w, sz = q3.x;
            const uint32_t where = (uint32_t)q3.z;
            const int xa = (q1.x > x0 ? q1.x : x0) - x0, xb = (q1.w < x0 + 63 ? q1.w : x0 + 63) - x0;   // the box's bits of a row
            if (y < q1.y || y > q2.x) continue;
            const int row0 = q3.y + sy * y + sx * x0;   // the source index of bit 0 of the row, less stride.z * z
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int z = z0 + lz + 16 * j;
                if (z < q1.z || z > q2.y) continue;
                const int idx0 = row0 + sz * z;
                uint64_t present = 0ull, solid = 0ull;
                for (int b = xa; b <= xb; b++) {
                    const uint32_t st = state[idx0 + sx * b];
                    present |= (uint64_t)(st != 0u) << b;
                    solid |= (uint64_t)(st == 2u) << b;
                }
                uint64_t sel = where == 0u ? present : where == 1u ? (present & row[j]) : (present & ~row[j]);
                row[j] = (row[j] & ~sel) | (solid & sel);
                // material words: the four x of one brick are 16 contiguous bytes of the swizzled array
                while (sel) {
                    const int g = (int)(__ffsll((unsigned long long)sel) - 1) >> 2;
                    const uint32_t nib = (uint32_t)(sel >> (4 * g)) & 0xFu;
                    uint32_t* dst = mat_sw + swizzled_index(x0 + 4 * g, y, z, lb);
                    const int src = idx0 + sx * 4 * g;
                    if (nib == 0xFu) {
                        *reinterpret_cast<uint4*>(dst) = make_uint4(mats[src], mats[src + sx], mats[src + 2 * sx], mats[src + 3 * sx]);
                    } else {
#pragma unroll
                        for (int xi = 0; xi < 4; xi++)
                            if ((nib >> xi) & 1u) dst[xi] = mats[src + sx * xi];
                    }
                    sel &= ~(0xFull << (4 * g));
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int w = 2 * ((lz + 16 * j) * kRow0Stride + ly);
            occ0[w] = (uint32_t)row[j];
            occ0[w + 1] = (uint32_t)(row[j] >> 32);
        }
    }
};

}  // namespace

// One workgroup (16 waves) per touched chunk: chunks[blockIdx.x] is its id, recs[offs[i] .. offs[i + 1]) its edits (RecordStage).
__global__ __launch_bounds__(1024) void k_rebuild_chunks(uint8_t* __restrict__ mine_sw, uint32_t* __restrict__ mat_sw,
                                                         const uint32_t* __restrict__ chunks, const uint32_t* __restrict__ offs,
                                                         const uint2* __restrict__ recs, int logr) {
    rebuild_chunk(mine_sw, chunks, logr, RecordStage{mat_sw, offs, recs});
}

// One workgroup per chunk that meets a shape's bounding box; every workgroup walks the whole batch (ShapeStage).
__global__ __launch_bounds__(1024) void k_shape_chunks(uint8_t* __restrict__ mine_sw, uint32_t* __restrict__ mat_sw,
                                                       const uint32_t* __restrict__ chunks, const int4* __restrict__ shapes,
                                                       uint32_t nshapes, int logr) {
    rebuild_chunk(mine_sw, chunks, logr, ShapeStage{mat_sw, shapes, nshapes});
}

// One workgroup per chunk that meets a placement's bounding box; every workgroup walks the whole batch (StampStage).
__global__ __launch_bounds__(1024) void k_stamp_chunks(uint8_t* __restrict__ mine_sw, uint32_t* __restrict__ mat_sw,
                                                       const uint32_t* __restrict__ chunks, const int4* __restrict__ recs,
                                                       uint32_t nrecs, int logr) {
    rebuild_chunk(mine_sw, chunks, logr, StampStage{mat_sw, recs, nrecs});
}

// rt_stamp_capture: voxel i of the stamp (x fastest) is the region's texel (x0, y0, z0) + (i % ex, i / ex % ey, i / (ex ey)): SOLID
// (2) where the minefield byte is 0, else AIR (1), or ABSENT (0) with skip_air; the material word is the voxel's, 0 where ABSENT.
__global__ __launch_bounds__(256) void k_stamp_capture(const uint8_t* __restrict__ mine_sw, const uint32_t* __restrict__ mat_sw, int logr,
                                                       int x0, int y0, int z0, int ex, int ey, uint32_t n, uint32_t skip_air,
                                                       uint32_t* __restrict__ mats_out, uint8_t* __restrict__ state_out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int x = x0 + (int)(i % (uint32_t)ex), y = y0 + (int)((i / (uint32_t)ex) % (uint32_t)ey), z = z0 + (int)(i / ((uint32_t)ex * (uint32_t)ey));
    const uint32_t s = swizzled_index(x, y, z, logr - 2);
    const uint32_t st = mine_sw[s] == 0u ? 2u : skip_air ? 0u : 1u;
    state_out[i] = (uint8_t)st;
    mats_out[i] = st ? mat_sw[s] : 0u;
}

// rt_stamp_create: the material word of an ABSENT voxel is 0 (what rt_stamp_read returns).
__global__ __launch_bounds__(256) void k_stamp_clean(uint32_t* __restrict__ mats, const uint8_t* __restrict__ state, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n && state[i] == 0u) mats[i] = 0u;
}

// The nibble-map words over the touched chunks, after k_rebuild_chunks: one workgroup per chunk.  A coarse cube has edge R/64, so a
// chunk holds 4096/R cubes per axis (16, 8, 4); at R = 1024 a word's 8 cubes span two chunks along x and the other chunk's half is
// recomputed from its unchanged bytes (two touched neighbours both write the same value).  R > 256: the chunk's 16^3 bricks as well.
__global__ __launch_bounds__(512) void k_rebuild_chunk_maps(const uint8_t* __restrict__ mine_sw, uint32_t* __restrict__ coarse,
                                                            uint32_t* __restrict__ brick_words, const uint32_t* __restrict__ chunks,
                                                            int logr) {
    const int nl = logr - 6, lb = logr - 2;
    const uint32_t cid = chunks[blockIdx.x], cmask = (1u << nl) - 1u;
    const uint32_t cx = cid & cmask, cy = (cid >> nl) & cmask, cz = cid >> (2 * nl);
    const uint32_t cpa = 4096u >> logr;                   // coarse cubes per chunk edge
    const uint32_t nwx = cpa >= 8u ? cpa / 8u : 1u;        // words per cube row of the chunk
    const uint32_t wx0 = (cx * cpa) / 8u;
    const uint32_t ncw = nwx * cpa * cpa;
    const uint32_t nbw = brick_words ? 2u * 16u * 16u : 0u;
    for (uint32_t t = threadIdx.x; t < ncw + nbw; t += 512u) {
        if (t < ncw) {
            const uint32_t wx = wx0 + t % nwx, yy = cy * cpa + (t / nwx) % cpa, zz = cz * cpa + t / (nwx * cpa);
            const uint32_t w = (zz << 9) | (yy << 3) | wx;
            coarse[w] = coarse_word(mine_sw, w, logr);
        } else {
            const uint32_t u = t - ncw;
            const uint32_t wx = 2u * cx + (u & 1u), by = cy * 16u + ((u >> 1) & 15u), bz = cz * 16u + (u >> 5);
            const uint32_t w = brick_index(8u * wx, by, bz, lb) >> 3;
            brick_words[w] = brick_word(mine_sw, w);
        }
    }
}

hipError_t launch_rebuild_chunks(uint8_t* mine_sw, uint32_t* mat_sw, const uint32_t* chunks, const uint32_t* offs, const uint2* recs,
                                 uint32_t nchunks, int logr, hipStream_t st) {
    if (nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rebuild_chunks, dim3(nchunks), dim3(1024), 0, st, mine_sw, mat_sw, chunks, offs, recs, logr);
    return hipGetLastError();
}

hipError_t launch_shape_chunks(uint8_t* mine_sw, uint32_t* mat_sw, const uint32_t* chunks, const void* shapes, uint32_t nshapes,
                               uint32_t nchunks, int logr, hipStream_t st) {
    if (nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_shape_chunks, dim3(nchunks), dim3(1024), 0, st, mine_sw, mat_sw, chunks, static_cast<const int4*>(shapes), nshapes, logr);
    return hipGetLastError();
}

hipError_t launch_stamp_chunks(uint8_t* mine_sw, uint32_t* mat_sw, const uint32_t* chunks, const void* recs, uint32_t nrecs,
                               uint32_t nchunks, int logr, hipStream_t st) {
    if (nchunks == 0) return hipSuccess;
    if (nrecs > 4096u) return hipErrorInvalidValue;   // (StampStage's bit per placement; the host admits 4096 per call)
    hipLaunchKernelGGL(k_stamp_chunks, dim3(nchunks), dim3(1024), 0, st, mine_sw, mat_sw, chunks, static_cast<const int4*>(recs), nrecs, logr);
    return hipGetLastError();
}

hipError_t launch_stamp_capture(const uint8_t* mine_sw, const uint32_t* mat_sw, int logr, int x0, int y0, int z0, int ex, int ey, int ez,
                                bool skip_air, uint32_t* mats_out, uint8_t* state_out, hipStream_t st) {
    const uint32_t n = (uint32_t)ex * (uint32_t)ey * (uint32_t)ez;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_stamp_capture, dim3((n + 255u) / 256u), dim3(256), 0, st, mine_sw, mat_sw, logr, x0, y0, z0, ex, ey, n,
                       skip_air ? 1u : 0u, mats_out, state_out);
    return hipGetLastError();
}

hipError_t launch_stamp_clean(uint32_t* mats, const uint8_t* state, uint32_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_stamp_clean, dim3((n + 255u) / 256u), dim3(256), 0, st, mats, state, n);
    return hipGetLastError();
}

hipError_t launch_rebuild_chunk_maps(const uint8_t* mine_sw, uint32_t* coarse, uint32_t* brick, const uint32_t* chunks, uint32_t nchunks,
                                     int logr, hipStream_t st) {
    if (nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rebuild_chunk_maps, dim3(nchunks), dim3(512), 0, st, mine_sw, coarse, logr > 8 ? brick : nullptr, chunks, logr);
    return hipGetLastError();
}

}  // namespace rtd
