// rt_world.hpp — the rule of the two nibble maps over the brick-swizzled minefield, stated once for every kernel that changes the
// resident world (rt_world.hip, rt_edit.hip, rt_terrain.hip).  The kernels that draw a frame only read the maps and do not
// include this.
//
// A nibble is the common value of a cube's bytes if they are all equal and below kNibMixed, else kNibMixed ("read the byte").
// Scene::coarse holds one per cube of edge R/64, Scene::brick (R > 256) one per 4^3 brick; a word holds 8 x-adjacent nibbles.
// k_check_maps (rt_world.hip) restates the rule voxel by voxel and calls nothing in here.
#pragma once
#include "rt_device.hpp"

namespace rtd {

// Brick (bx, by, bz) of the swizzled arrays: its 64 entries start at brick_index << 6 (swizzled_index, rt_device.hpp).
__device__ __forceinline__ uint32_t brick_index(uint32_t bx, uint32_t by, uint32_t bz, int lb) {
    return (((bz << lb) + by) << lb) + bx;
}

// One brick's 64 consecutive bytes, and the one test on them: brick_diff is 0 iff every byte equals v.
struct Brick { uint4 a, q, d, e; };
__device__ __forceinline__ Brick load_brick(const uint8_t* mine_sw, uint32_t brick) {
    const uint4* src = reinterpret_cast<const uint4*>(mine_sw + ((size_t)brick << 6));
    return Brick{src[0], src[1], src[2], src[3]};
}
__device__ __forceinline__ uint32_t brick_first(const Brick& k) { return k.a.x & 0xFFu; }
__device__ __forceinline__ uint32_t brick_diff(const Brick& k, uint32_t v) {
    const uint32_t splat = v * 0x01010101u;
    return (k.a.x ^ splat) | (k.a.y ^ splat) | (k.a.z ^ splat) | (k.a.w ^ splat) | (k.q.x ^ splat) | (k.q.y ^ splat) |
           (k.q.z ^ splat) | (k.q.w ^ splat) | (k.d.x ^ splat) | (k.d.y ^ splat) | (k.d.z ^ splat) | (k.d.w ^ splat) |
           (k.e.x ^ splat) | (k.e.y ^ splat) | (k.e.z ^ splat) | (k.e.w ^ splat);
}
__device__ __forceinline__ uint32_t nibble_of(uint32_t diff, uint32_t first) { return (diff == 0u && first < kNibMixed) ? first : kNibMixed; }

__device__ __forceinline__ uint32_t brick_nibble(const uint8_t* mine_sw, uint32_t brick) {
    const Brick k = load_brick(mine_sw, brick);
    return nibble_of(brick_diff(k, brick_first(k)), brick_first(k));
}

// Coarse word w = (cz << 9) | (cy << 3) | wx: cubes cx = 8 wx .. 8 wx + 7, each (R/256)^3 bricks, every one of them tested against
// the first byte of the cube's first brick (one running OR, no exit: the loads of a cube are independent of each other).
__device__ inline uint32_t coarse_word(const uint8_t* mine_sw, uint32_t w, int logr) {
    const int lb = logr - 2, sub = logr - 8;               // sub: log2(bricks per cube edge)
    const uint32_t nsub = 1u << sub;
    uint32_t word = 0;
    for (uint32_t b = 0; b < 8u; b++) {
        const uint32_t c = w * 8u + b;                     // cube (cz, cy, cx), 6 bits each
        const uint32_t cx = c & 63u, cy = (c >> 6) & 63u, cz = c >> 12;
        uint32_t first = 0, diff = 0;
        for (uint32_t bz = 0; bz < nsub; bz++)
            for (uint32_t by = 0; by < nsub; by++)
                for (uint32_t bx = 0; bx < nsub; bx++) {
                    const Brick k = load_brick(mine_sw, brick_index((cx << sub) + bx, (cy << sub) + by, (cz << sub) + bz, lb));
                    if ((bz | by | bx) == 0u) first = brick_first(k);
                    diff |= brick_diff(k, first);
                }
        word |= nibble_of(diff, first) << (4 * b);
    }
    return word;
}

// Brick word w: bricks 8 w .. 8 w + 7 (x-adjacent: bricks per row are a multiple of 8).
__device__ __forceinline__ uint32_t brick_word(const uint8_t* mine_sw, uint32_t w) {
    uint32_t word = 0;
    for (uint32_t b = 0; b < 8u; b++) word |= brick_nibble(mine_sw, w * 8u + b) << (4 * b);
    return word;
}

}  // namespace rtd
