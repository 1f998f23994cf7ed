// rt_terrain.hip — gfx950 kernels of rt_generate_world and rt_generate_slice: the project's deterministic terrain
// (raytrace_amd/host/world.cpp: terrain_height, material_for_height, generate_chunk, pack_into) generated straight into the
// brick-swizzled region, byte for byte what the host generator assembles and rt_upload_world / rt_upload_slice re-tile.
//
//   k_terrain_heights: one thread per column of the window, widened to whole world chunks: the FP64 height, the same operations
//                      in the same order as world.cpp (both sides compile with -ffp-contract=off -fno-fast-math)
//   k_terrain_fill   : one workgroup per world chunk that overlaps the window: the chunk column's 64^2 heights and their max
//                      pyramid in LDS, then every voxel of the chunk inside the window from them — pack_into's minefield of a
//                      generated chunk is a function of the heights alone (DESIGN.md "Terrain on the device")
// The nibble-map words over the written box follow from the bytes (launch_build_maps, rt_world.hip).
#include <hip/hip_runtime.h>

#include "rt_device.hpp"
#include "rt_kernels.hpp"
#include "rt_world.hpp"

namespace rtd {

namespace {

// ---- world.cpp restated for the device ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t tg_mix64(uint64_t x) {   // splitmix64 finaliser
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
constexpr uint64_t kHashSalt = 0xA5A5A5A5DEADBEEFull, kHashY = 0x9E3779B97F4A7C15ull, kHashZ = 0xC2B2AE3D27D4EB4Full;
constexpr uint64_t kMaterialSalt = 0x51ED270B7F4A7C15ull, kOctaveStep = 0x632BE59BD9B4E019ull;

// hash3(seed, a, b, c) up to (and including) the b step: the part a column shares
__device__ __forceinline__ uint64_t tg_hash_ab(uint64_t seed, int64_t a, int64_t b) {
    uint64_t h = tg_mix64(seed ^ kHashSalt);
    h = tg_mix64(h ^ (uint64_t)a);
    return tg_mix64(h ^ (uint64_t)b * kHashY);
}

__constant__ double kTgDir[16][2] = {
    {1.0, 0.0}, {0.9238795325, 0.3826834324}, {0.7071067812, 0.7071067812}, {0.3826834324, 0.9238795325},
    {0.0, 1.0}, {-0.3826834324, 0.9238795325}, {-0.7071067812, 0.7071067812}, {-0.9238795325, 0.3826834324},
    {-1.0, 0.0}, {-0.9238795325, -0.3826834324}, {-0.7071067812, -0.7071067812}, {-0.3826834324, -0.9238795325},
    {0.0, -1.0}, {0.3826834324, -0.9238795325}, {0.7071067812, -0.7071067812}, {0.9238795325, -0.3826834324}};

__device__ __forceinline__ double tg_corner(uint64_t seed, int64_t cx, int64_t cy, double dx, double dy) {
    const uint32_t g = (uint32_t)tg_mix64(tg_hash_ab(seed, cx, cy)) & 15u;   // hash3(seed, cx, cy, 0): c * K = 0
    return kTgDir[g][0] * dx + kTgDir[g][1] * dy;
}
__device__ __forceinline__ double tg_fade(double t) { return t * t * t * (t * (t * 6.0 - 15.0) + 10.0); }

__device__ double tg_gradient_noise(double x, double y, uint64_t seed) {
    const double fx = floor(x), fy = floor(y);
    const int64_t ix = (int64_t)fx, iy = (int64_t)fy;
    const double tx = x - fx, ty = y - fy;
    const double n00 = tg_corner(seed, ix, iy, tx, ty), n10 = tg_corner(seed, ix + 1, iy, tx - 1.0, ty);
    const double n01 = tg_corner(seed, ix, iy + 1, tx, ty - 1.0), n11 = tg_corner(seed, ix + 1, iy + 1, tx - 1.0, ty - 1.0);
    const double u = tg_fade(tx), v = tg_fade(ty);
    const double a = n00 + (n10 - n00) * u, b = n01 + (n11 - n01) * u;
    return (a + (b - a) * v) * 1.4142135623730951;
}

__device__ double tg_get_noise(double x, double y, uint64_t seed) {   // basic_multi(x, y, seed) * 0.5 + 0.5
    double px = x * 2.0, py = y * 2.0, amp = 1.0, sum = 0.0;
    for (int o = 0; o < 6; o++) {
        sum += tg_gradient_noise(px, py, seed + (uint64_t)o * kOctaveStep) * amp;
        px *= 2.0; py *= 2.0; amp *= 0.5;
    }
    return sum * 0.5 * 0.5 + 0.5;
}

__device__ int32_t tg_terrain_height(int64_t x, int64_t y, uint64_t seed) {
    const double kScale = 600.0;
    const double mx = (double)x / kScale, my = (double)y / kScale;
    const double d = 0.2;
    const double left = tg_get_noise(mx - d, my, seed), right = tg_get_noise(mx + d, my, seed);
    const double up = tg_get_noise(mx, my - d, seed), down = tg_get_noise(mx, my + d, seed);
    const double dx = (right - left) / (d * 2.0), dy = (down - up) / (d * 2.0);
    const double slope = sqrt(dx * dx + dy * dy);
    const double base = tg_get_noise(mx, my, seed);
    double eroded = base + (1.0 - slope) * 0.7;
    if (eroded < 0.0) eroded = 0.0;
    const double m = pow(eroded / 1.5, 2.6);
    return (int32_t)(int64_t)(m * kScale * 0.2 + 10.0);
}

// MATERIALS[id].pack() of the ids generate_chunk writes (world.cpp: albedo << 14 | << 7 | solid << 15)
constexpr uint32_t pack_material(uint32_t r, uint32_t g, uint32_t b) { return (r << 14 | g << 7 | b) | (1u << 15); }
constexpr uint32_t kGrass = pack_material(39, 110, 61), kDirt = pack_material(62, 27, 22), kRock = pack_material(110, 116, 115);

// material_for_height for a solid voxel at height z of the column whose hash3 prefix is `col`
__device__ __forceinline__ uint32_t tg_material(uint64_t col, int z) {
    if (z < 20) return kGrass;
    if (z >= 160) return kRock;
    const uint32_t r = (uint32_t)(tg_mix64(col ^ (uint64_t)(int64_t)z * kHashZ) >> 16);
    if (z < 80) return r % 60u < (uint32_t)(z - 20) ? kDirt : kGrass;
    return r % 80u < (uint32_t)(z - 80) ? kRock : kDirt;
}

}  // namespace

// Heights of the columns [x0, x0 + w) x [y0, y0 + n / w), x fastest.
__global__ __launch_bounds__(256) void k_terrain_heights(int32_t* __restrict__ heights, int64_t x0, int64_t y0, uint32_t w, uint32_t n,
                                                         uint64_t seed) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    heights[t] = tg_terrain_height(x0 + (int64_t)(t % w), y0 + (int64_t)(t / w), seed);
}

// One workgroup per world chunk (c0 + blockIdx) that overlaps the window [lo, lo + ext).  heights: the columns of every chunk of the
// grid, row stride hw, starting at world (c0.x * 64, c0.y * 64).  Per voxel (world.cpp generate_chunk + pack_into):
//   solid  = deep chunk (cz < 0) || z < h(x, y)
//   mine   = 0 if solid, else the first L in 1..6 whose aligned 2^L cube is occupied — deep || max h over its footprint > its z0 —
//            and 6 when none is (pack_into's all-air chunk gets 6 everywhere)
//   mat    = grass in a deep chunk, material_for_height of a solid voxel, 0 for air
// A lane writes one z-layer of a 4^3 brick: 16 minefield bytes and 16 material words, dword4 stores; a wave covers 16 x-adjacent
// bricks' four layers, 1 KiB of minefield and 4 KiB of materials.  Every texel is (v + R/2) mod R, so no store leaves the region.
__global__ __launch_bounds__(256) void k_terrain_fill(uint8_t* __restrict__ mine_sw, uint32_t* __restrict__ mat_sw,
                                                      const int32_t* __restrict__ heights, uint32_t hw, int3 c0, int3 lo, int3 ext,
                                                      uint64_t seed, int logr) {
    __shared__ int32_t hgt[64 * 64];           // 16 KiB: the chunk column's heights, [y][x]
    __shared__ uint64_t colh[64 * 64];         // 32 KiB: hash3 prefix of each column (only chunks with 20 <= z < 160 use it)
    __shared__ int32_t m2[16 * 16], m3[8 * 8], m4[4 * 4], m5[2 * 2];   // max height over each 2^L footprint, L = 2..5 (level 6
                                                                        // needs none: 6 is the fallback value)

    const int tid = threadIdx.x;
    const int cx = c0.x + (int)blockIdx.x, cy = c0.y + (int)blockIdx.y, cz = c0.z + (int)blockIdx.z;
    const int ox = cx * 64, oy = cy * 64, oz = cz * 64;   // (inside the window's chunks: int32, as every voxel of the window)
    // the part of the chunk inside the window (16-aligned on every axis; int64: a window may end at 2^31)
    auto part = [](int o, int l, int e, int& b0, int& b1) {
        b0 = (int)(max((int64_t)o, (int64_t)l) - o);
        b1 = (int)(min((int64_t)o + 64, (int64_t)l + e) - o);
    };
    int bx0, bx1, by0, by1, lz0, lz1;
    part(ox, lo.x, ext.x, bx0, bx1);
    part(oy, lo.y, ext.y, by0, by1);
    part(oz, lo.z, ext.z, lz0, lz1);
    if (bx1 <= bx0 || by1 <= by0 || lz1 <= lz0) return;   // (whole workgroup: the box is uniform)
    const bool deep = cz < 0;                             // generate.rs:63-64: oz + 64 < 12
    const bool hashed = !deep && oz < 160;                // material_for_height rolls only for 20 <= z < 160

    if (!deep) {
        const int32_t* src = heights + (size_t)(oy - c0.y * 64) * hw + (size_t)(ox - c0.x * 64);
        for (int i = tid; i < 64 * 64; i += 256) {
            const int x = i & 63, y = i >> 6;
            hgt[i] = src[(size_t)y * hw + x];
            if (hashed) colh[i] = tg_hash_ab(seed ^ kMaterialSalt, (int64_t)ox + x, (int64_t)oy + y);
        }
        __syncthreads();
        {   // level 2: one thread per 4x4 footprint
            const int X = tid & 15, Y = tid >> 4;
            int32_t m = INT32_MIN;
            for (int k = 0; k < 16; k++) m = max(m, hgt[(4 * Y + (k >> 2)) * 64 + 4 * X + (k & 3)]);
            m2[tid] = m;
        }
        __syncthreads();
        if (tid < 64) { const int X = tid & 7, Y = tid >> 3;
            m3[tid] = max(max(m2[(2 * Y) * 16 + 2 * X], m2[(2 * Y) * 16 + 2 * X + 1]), max(m2[(2 * Y + 1) * 16 + 2 * X], m2[(2 * Y + 1) * 16 + 2 * X + 1])); }
        __syncthreads();
        if (tid < 16) { const int X = tid & 3, Y = tid >> 2;
            m4[tid] = max(max(m3[(2 * Y) * 8 + 2 * X], m3[(2 * Y) * 8 + 2 * X + 1]), max(m3[(2 * Y + 1) * 8 + 2 * X], m3[(2 * Y + 1) * 8 + 2 * X + 1])); }
        __syncthreads();
        if (tid < 4) { const int X = tid & 1, Y = tid >> 1;
            m5[tid] = max(max(m4[(2 * Y) * 4 + 2 * X], m4[(2 * Y) * 4 + 2 * X + 1]), max(m4[(2 * Y + 1) * 4 + 2 * X], m4[(2 * Y + 1) * 4 + 2 * X + 1])); }
        __syncthreads();
    }

    const int R = 1 << logr, lb = logr - 2;
    const uint32_t rmask = (uint32_t)R - 1u;
    // texel of the chunk's first voxel: world chunks map onto whole 64-texel blocks (R/2 is a multiple of 64)
    const uint32_t tx0 = (uint32_t)((int64_t)ox + R / 2) & rmask, ty0 = (uint32_t)((int64_t)oy + R / 2) & rmask,
                   tz0 = (uint32_t)((int64_t)oz + R / 2) & rmask;
    const int nbx = (bx1 - bx0) >> 2, nby = (by1 - by0) >> 2, nz = lz1 - lz0;
    const int items = nbx * nby * nz;
    for (int it = tid; it < items; it += 256) {
        const int zl = it & 3, j = it >> 2;
        const int bxl = j % nbx, j2 = j / nbx;
        const int byl = j2 % nby, zq = j2 / nby;
        const int lx = bx0 + 4 * bxl, ly = by0 + 4 * byl, lz = lz0 + 4 * zq + zl;
        const int z = oz + lz;
        uint32_t mine[4], mats[16];
        if (deep) {
#pragma unroll
            for (int r = 0; r < 4; r++) mine[r] = 0u;
#pragma unroll
            for (int k = 0; k < 16; k++) mats[k] = kGrass;
        } else {
            const int X = lx >> 2, Y = ly >> 2;
            // brick-level value: the first of levels 2..6 whose cube is occupied (6 when none is)
            uint32_t bv = 6u;
            if (m5[((Y >> 3) << 1) | (X >> 3)] > (z & ~31)) bv = 5u;
            if (m4[((Y >> 2) << 2) | (X >> 2)] > (z & ~15)) bv = 4u;
            if (m3[((Y >> 1) << 3) | (X >> 1)] > (z & ~7)) bv = 3u;
            if (m2[(Y << 4) | X] > (z & ~3)) bv = 2u;
            int32_t h[16];
#pragma unroll
            for (int k = 0; k < 16; k++) h[k] = hgt[(ly + (k >> 2)) * 64 + lx + (k & 3)];
            const int z1 = z & ~1;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                uint32_t d = 0;
#pragma unroll
                for (int xi = 0; xi < 4; xi++) {
                    const int k = r * 4 + xi;
                    const int kb = (r & 2) * 4 + (xi & 2);   // the 2x2 footprint's first column
                    const int32_t m1 = max(max(h[kb], h[kb + 1]), max(h[kb + 4], h[kb + 5]));
                    const bool solid = z < h[k];
                    const uint32_t v = solid ? 0u : (m1 > z1 ? 1u : bv);
                    d |= v << (8 * xi);
                    mats[k] = solid ? (hashed ? tg_material(colh[(ly + r) * 64 + lx + xi], z) : (z < 20 ? kGrass : kRock)) : 0u;
                }
                mine[r] = d;
            }
        }
        const uint32_t tx = tx0 + (uint32_t)lx, ty = ty0 + (uint32_t)ly, tz = (tz0 + (uint32_t)lz) & rmask;
        const size_t brick = brick_index(tx >> 2, ty >> 2, tz >> 2, lb);
        const size_t at = (brick << 6) | ((size_t)(tz & 3u) << 4);
        *reinterpret_cast<uint4*>(mine_sw + at) = make_uint4(mine[0], mine[1], mine[2], mine[3]);
        uint4* mdst = reinterpret_cast<uint4*>(mat_sw + at);
#pragma unroll
        for (int r = 0; r < 4; r++) mdst[r] = make_uint4(mats[4 * r], mats[4 * r + 1], mats[4 * r + 2], mats[4 * r + 3]);
    }
}

hipError_t launch_terrain(uint8_t* mine_sw, uint32_t* mat_sw, uint32_t* coarse, uint32_t* brick, int32_t* heights, int logr,
                          uint64_t seed, const int64_t lo[3], int axis, hipStream_t st) {
    const int64_t R = (int64_t)1 << logr;
    int64_t ext[3], c0[3], nc[3];
    for (int a = 0; a < 3; a++) {
        ext[a] = a == axis ? RT_SLICE_SIZE : R;
        const int64_t f0 = lo[a] >> 6, f1 = (lo[a] + ext[a] - 1) >> 6;   // (arithmetic shifts: floor division)
        c0[a] = f0;
        nc[a] = f1 - f0 + 1;
    }
    // heights of every column of the overlapped chunk columns (at most (R/64 + 1)^2 chunks: the buffer rt_api.hip allocates)
    const uint32_t hw = (uint32_t)(nc[0] * 64), hn = (uint32_t)(nc[0] * 64 * nc[1] * 64);
    hipLaunchKernelGGL(k_terrain_heights, dim3((hn + 255u) / 256u), dim3(256), 0, st, heights, c0[0] * 64, c0[1] * 64, hw, hn, seed);
    const int3 ic0 = make_int3((int)c0[0], (int)c0[1], (int)c0[2]);
    const int3 ilo = make_int3((int)lo[0], (int)lo[1], (int)lo[2]), iext = make_int3((int)ext[0], (int)ext[1], (int)ext[2]);
    hipLaunchKernelGGL(k_terrain_fill, dim3((unsigned)nc[0], (unsigned)nc[1], (unsigned)nc[2]), dim3(256), 0, st, mine_sw, mat_sw,
                       (const int32_t*)heights, hw, ic0, ilo, iext, seed, logr);
    // nibble-map words: everything for a whole region, the words a slab at its texel offset touches for one slab
    const MapBoxes boxes = axis < 0 ? map_boxes_region(logr) : map_boxes_slab(logr, axis, (int)((lo[axis] + R / 2) & (R - 1)));
    return launch_build_maps(mine_sw, coarse, brick, logr, boxes, st);
}

}  // namespace rtd
