// rt_world.hip — gfx950 kernels of the resident world's layout: re-tiling into the 4^3-brick-swizzled arrays, the two nibble maps
// over them, and reading both back.
//
//   k_flatten_voxels : rt_upload_world: linear R^3 arrays -> brick-swizzled arrays
//   k_flatten_slab   : rt_upload_slice: the same for one 16-thick slab
//   k_build_maps     : the coarse (and, above R = 256, brick) nibble-map words of a box, by rt_world.hpp's rule — the whole maps
//                      after an upload or a generated region, the words a slab touches after an uploaded or generated slab
//   k_check_maps     : rt_selftest(RT_SELFTEST_SCENE_MAPS): every word of both maps against the rule restated voxel by voxel
//   k_read_box       : rt_read_box: un-tiles a box of the region into the caller's layout (x fastest)
#include <hip/hip_runtime.h>

#include "rt_kernels.hpp"
#include "rt_world.hpp"

namespace rtd {

// dst index i (swizzled) <- src linear index (x fastest, util.rs:104-106).  Writes are fully coalesced; reads come
// in 4-voxel runs.  Flags minefield values above kMaxStepValue (the reference writes 0..6, chunk.rs:163-183).
__global__ __launch_bounds__(256) void k_flatten_voxels(const uint8_t* __restrict__ mine_lin,
                                                        const uint32_t* __restrict__ mat_lin,
                                                        uint8_t* __restrict__ mine_sw, uint32_t* __restrict__ mat_sw,
                                                        uint32_t* __restrict__ bad_value_flag, int logr) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;   // grid covers exactly R^3 (< 2^31)
    const int lb = logr - 2;
    const uint32_t bmask = (1u << lb) - 1u;
    uint32_t brick = i >> 6, l = i & 63u;
    uint32_t ix = ((brick & bmask) << 2) | (l & 3u);
    uint32_t iy = (((brick >> lb) & bmask) << 2) | ((l >> 2) & 3u);
    uint32_t iz = ((brick >> (2 * lb)) << 2) | (l >> 4);
    size_t src = (((((size_t)iz << logr) + iy) << logr)) + ix;
    uint8_t v = mine_lin[src];
    if (v > kMaxStepValue) atomicOr(bad_value_flag, 1u);
    mine_sw[i] = v;
    mat_sw[i] = mat_lin[src];
}

// rt_upload_slice: the same re-tiling for ONE 16-thick slab (TerrainUploadManager::upload_slice, terrain_upload.rs:84-275 ->
// vkCmdCopyBufferToImage with an offset).  The slab arrives as a dense box of extent 16 along `axis` and R along the other
// two (x fastest); thread i handles swizzled voxel i of the slab's bricks — 4 brick layers along `axis`, whole bricks, so every
// thread writes inside one 64-byte line run.  (The slab's values were checked on the host before it got here: rt_upload_slice.)
__global__ __launch_bounds__(256) void k_flatten_slab(const uint8_t* __restrict__ mine_slab, const uint32_t* __restrict__ mat_slab,
                                                      uint8_t* __restrict__ mine_sw, uint32_t* __restrict__ mat_sw,
                                                      int logr, int axis, int offset) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;   // grid covers exactly 16 * R^2
    const int lb = logr - 2;
    const uint32_t bmask = (1u << lb) - 1u;
    const uint32_t l = i & 63u, sb = i >> 6;              // sb: brick within the slab, 4 layers along `axis`
    // brick coordinates: the two full axes take lb bits each, the slab axis 2 bits (layer) on top of offset/4
    uint32_t bc[3];
    uint32_t rest = sb;
    for (int a = 0; a < 3; a++) {
        if (a == axis) { bc[a] = (uint32_t)(offset >> 2) + (rest & 3u); rest >>= 2; }
        else { bc[a] = rest & bmask; rest >>= lb; }
    }
    const uint32_t ix = (bc[0] << 2) | (l & 3u), iy = (bc[1] << 2) | ((l >> 2) & 3u), iz = (bc[2] << 2) | (l >> 4);
    const uint32_t R = 1u << logr;
    const uint32_t sx = axis == 0 ? ix - (uint32_t)offset : ix, sy = axis == 1 ? iy - (uint32_t)offset : iy,
                   sz = axis == 2 ? iz - (uint32_t)offset : iz;
    const uint32_t ex = axis == 0 ? (uint32_t)RT_SLICE_SIZE : R, ey = axis == 1 ? (uint32_t)RT_SLICE_SIZE : R;
    const size_t src = ((size_t)sz * ey + sy) * ex + sx;
    const size_t dst = ((size_t)brick_index(bc[0], bc[1], bc[2], lb) << 6) | l;
    mine_sw[dst] = mine_slab[src];
    mat_sw[dst] = mat_slab[src];
}

// Thread t builds coarse word t of the box (cw0, cwn) or brick word t - ncw of the box (bw0, bwn); brick_words is null at R = 256.
__global__ __launch_bounds__(256) void k_build_maps(const uint8_t* __restrict__ mine_sw, uint32_t* __restrict__ coarse,
                                                    uint32_t* __restrict__ brick_words, int logr, MapBoxes box) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t ncw = box.cwn.x * box.cwn.y * box.cwn.z, nbw = brick_words ? box.bwn.x * box.bwn.y * box.bwn.z : 0u;
    const int lb = logr - 2;
    if (t < ncw) {
        const uint32_t wx = box.cw0.x + t % box.cwn.x, cy = box.cw0.y + (t / box.cwn.x) % box.cwn.y, cz = box.cw0.z + t / (box.cwn.x * box.cwn.y);
        const uint32_t w = (cz << 9) | (cy << 3) | wx;
        coarse[w] = coarse_word(mine_sw, w, logr);
    } else if (t - ncw < nbw) {
        const uint32_t u = t - ncw;
        const uint32_t wx = box.bw0.x + u % box.bwn.x, by = box.bw0.y + (u / box.bwn.x) % box.bwn.y, bz = box.bw0.z + u / (box.bwn.x * box.bwn.y);
        const uint32_t w = brick_index(8u * wx, by, bz, lb) >> 3;
        brick_words[w] = brick_word(mine_sw, w);
    }
}

// The rule as the maps' readers understand it, voxel by voxel: the nibble of the cube of edge e at voxel (x0, y0, z0).
__device__ uint32_t nibble_of_cube(const uint8_t* mine_sw, int x0, int y0, int z0, int e, int lb) {
    const uint8_t v = mine_sw[swizzled_index(x0, y0, z0, lb)];
    for (int z = z0; z < z0 + e; z++)
        for (int y = y0; y < y0 + e; y++)
            for (int x = x0; x < x0 + e; x++)
                if (mine_sw[swizzled_index(x, y, z, lb)] != v) return kNibMixed;
    return v < kNibMixed ? v : kNibMixed;
}

// rt_selftest(RT_SELFTEST_SCENE_MAPS): thread t recomputes coarse word t (t < 32768) or brick word t - 32768 from nibble_of_cube
// alone — nothing of rt_world.hpp — and counts a difference.
__global__ __launch_bounds__(256) void k_check_maps(const uint8_t* __restrict__ mine_sw, const uint32_t* __restrict__ coarse,
                                                    const uint32_t* __restrict__ brick_words, uint32_t nbrick_words, int logr,
                                                    unsigned long long* __restrict__ mismatches) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int lb = logr - 2, e = 1 << (logr - 6), nb = 1 << lb;
    bool differs = false;
    if (t < (uint32_t)kCoarseWords) {
        uint32_t word = 0;
        for (int b = 0; b < 8; b++) {
            const int c = (int)t * 8 + b;      // cube (cz, cy, cx), 6 bits each
            word |= nibble_of_cube(mine_sw, (c & 63) * e, ((c >> 6) & 63) * e, (c >> 12) * e, e, lb) << (4 * b);
        }
        differs = word != coarse[t];
    } else if (t - (uint32_t)kCoarseWords < nbrick_words) {
        const uint32_t u = t - (uint32_t)kCoarseWords;
        uint32_t word = 0;
        for (int b = 0; b < 8; b++) {
            const int k = (int)u * 8 + b;      // brick (bz, by, bx), lb bits each
            word |= nibble_of_cube(mine_sw, (k & (nb - 1)) * 4, ((k >> lb) & (nb - 1)) * 4, (k >> (2 * lb)) * 4, 4, lb) << (4 * b);
        }
        differs = word != brick_words[u];
    }
    const uint64_t m = __ballot(differs);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(mismatches, (unsigned long long)__popcll(m));
}

// rt_read_box: out[i] for i over the box (x0, y0, z0) + [0, ex) x [0, ey) x [0, nz), x fastest.  Either output may be null.
__global__ __launch_bounds__(256) void k_read_box(const uint8_t* __restrict__ mine_sw, const uint32_t* __restrict__ mat_sw, int logr,
                                                  int x0, int y0, int z0, int ex, int ey, uint64_t n, uint32_t* __restrict__ mat_out,
                                                  uint8_t* __restrict__ mine_out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int x = x0 + (int)(i % (uint64_t)ex), y = y0 + (int)((i / (uint64_t)ex) % (uint64_t)ey), z = z0 + (int)(i / ((uint64_t)ex * ey));
    const uint32_t s = swizzled_index(x, y, z, logr - 2);
    if (mat_out) mat_out[i] = mat_sw[s];
    if (mine_out) mine_out[i] = mine_sw[s];
}

// ---- which words a change touches ---------------------------------------------------------------------------------------------
MapBoxes map_boxes_region(int logr) {
    const uint32_t nb = 1u << (logr - 2);
    return MapBoxes{make_uint3(0, 0, 0), make_uint3(8, 64, 64), make_uint3(0, 0, 0), make_uint3(nb / 8u, nb, nb)};
}

// A slab of 16 voxels at `texel_offset` along `axis`: cubes have edge R/64, so 1024/R layers of them (4, 2, 1), and four layers of
// bricks — rounded out to whole words along x (a word's 8 x-adjacent nibbles are all recomputed from the bytes).
MapBoxes map_boxes_slab(int logr, int axis, int texel_offset) {
    MapBoxes b = map_boxes_region(logr);
    const uint32_t off = (uint32_t)texel_offset, e = (1u << logr) / 64u;
    const uint32_t c0 = off / e, c1 = (off + RT_SLICE_SIZE - 1u) / e;   // inclusive cube range along `axis`
    const uint32_t b0 = off / 4u;                                       // first of the four brick layers
    if (axis == 0) { b.cw0.x = c0 / 8u; b.cwn.x = c1 / 8u - b.cw0.x + 1u; b.bw0.x = b0 / 8u; b.bwn.x = (b0 + 3u) / 8u - b.bw0.x + 1u; }
    else if (axis == 1) { b.cw0.y = c0; b.cwn.y = c1 - c0 + 1u; b.bw0.y = b0; b.bwn.y = 4u; }
    else { b.cw0.z = c0; b.cwn.z = c1 - c0 + 1u; b.bw0.z = b0; b.bwn.z = 4u; }
    return b;
}

hipError_t launch_build_maps(const uint8_t* mine_sw, uint32_t* coarse, uint32_t* brick, int logr, const MapBoxes& b, hipStream_t st) {
    uint32_t* bmap = logr > 8 ? brick : nullptr;
    const uint32_t n = b.cwn.x * b.cwn.y * b.cwn.z + (bmap ? b.bwn.x * b.bwn.y * b.bwn.z : 0u);
    hipLaunchKernelGGL(k_build_maps, dim3((n + 255u) / 256u), dim3(256), 0, st, mine_sw, coarse, bmap, logr, b);
    return hipGetLastError();
}

hipError_t launch_flatten(const uint8_t* mine_lin, const uint32_t* mat_lin, uint8_t* mine_sw, uint32_t* mat_sw,
                          uint32_t* coarse, uint32_t* brick, uint32_t* bad_flag, int logr, hipStream_t st) {
    hipLaunchKernelGGL(k_flatten_voxels, dim3((1u << (3 * logr)) / 256u), dim3(256), 0, st, mine_lin, mat_lin, mine_sw, mat_sw,
                       bad_flag, logr);
    return launch_build_maps(mine_sw, coarse, brick, logr, map_boxes_region(logr), st);
}

hipError_t launch_flatten_slab(const uint8_t* mine_slab, const uint32_t* mat_slab, uint8_t* mine_sw, uint32_t* mat_sw, uint32_t* coarse,
                               uint32_t* brick, int logr, int axis, int offset, hipStream_t st) {
    const uint32_t R = 1u << logr;
    hipLaunchKernelGGL(k_flatten_slab, dim3(RT_SLICE_SIZE * R * R / 256u), dim3(256), 0, st, mine_slab, mat_slab, mine_sw, mat_sw,
                       logr, axis, offset);
    return launch_build_maps(mine_sw, coarse, brick, logr, map_boxes_slab(logr, axis, offset), st);
}

hipError_t launch_check_maps(const uint8_t* mine_sw, const uint32_t* coarse, const uint32_t* brick, int logr,
                             unsigned long long* mismatches, hipStream_t st) {
    const uint32_t nbw = (logr > 8 && brick) ? (1u << (3 * (logr - 2))) / 8u : 0u;
    const uint32_t n = (uint32_t)kCoarseWords + nbw;
    hipLaunchKernelGGL(k_check_maps, dim3((n + 255u) / 256u), dim3(256), 0, st, mine_sw, coarse, nbw ? brick : nullptr, nbw, logr,
                       mismatches);
    return hipGetLastError();
}

hipError_t launch_read_box(const uint8_t* mine_sw, const uint32_t* mat_sw, int logr, int x0, int y0, int z0, int ex, int ey, int nz,
                           uint32_t* mat_out, uint8_t* mine_out, hipStream_t st) {
    const uint64_t n = (uint64_t)ex * (uint64_t)ey * (uint64_t)nz;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_read_box, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, st, mine_sw, mat_sw, logr, x0, y0, z0, ex, ey, n,
                       mat_out, mine_out);
    return hipGetLastError();
}

}  // namespace rtd
