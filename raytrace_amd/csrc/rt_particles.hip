// rt_particles.hip — gfx950 kernels of rt_draw_particles / rt_draw_particles_async: up to 2^20 small cubes composited into the planes of
// the frame drawn last, by depth (include/rt_abi.h "Particles"; tests/draw_particles_ref.py expands them to rt_draw_boxes' records).
// Particle i is the box center -+ half; every pixel ends with the bits k_draw_boxes would leave for those boxes in index order, but a
// tile reads only the particles that may touch it (DESIGN.md "Particles" carries the argument and the worst case).
//
//   k_particles_bin     : a thread per particle.  It derives the box, tests the record, and narrows the rectangle of 8x8 tiles the box
//                         may touch by bisecting each of its four edges with rt_tile_pass.hpp's cull — tile_dirs of a rectangle of
//                         many tiles, box_may_touch_tile with no depth — which only ever drops tiles the exact test rejects for
//                         every pixel.  At most kParticleBinTiles tiles: one count per tile's list.  More: the rectangle is widened
//                         to blocks of 8x8 tiles, and at most kParticleBinTiles blocks: one count per block's list.  More still: the
//                         particle joins the wide list.
//   k_particles_offsets : a thread per list.  A wave adds its lists' counts and claims that many pairs with one atomic; which
//                         segment a list gets depends on the order of the atomics, what it holds does not.
//   k_particles_fill    : a thread per particle writes its index into its lists' segments.
//   k_draw_particles    : a tile pass (rt_tile_pass.hpp).  A tile whose list, whose block's list and the wide list are all empty ends
//                         at once.  Else the wave walks the three 64 indices at a time: lane l loads particle ids[base + l] (16 bytes),
//                         culls it against the tile with the tile's depths, and every lane runs the exact slab test of its own ray on
//                         each candidate.  The winner is the smallest (t_in, index), compared explicitly: the order in which the
//                         atomics filled a list plays no part, and two runs give the same planes.
// Only vector atomics (atomicAdd on global words); no LDS, no inline assembly.
#include <hip/hip_runtime.h>

#include "rt_tile_pass.hpp"

namespace rtd {

namespace {

constexpr uint32_t kBinWg = 256;
// A particle's rectangle word: x0 | block << 11 | y0 << 12 | (w - 1) << 24 | (h - 1) << 28, in tiles, or with `block` set in blocks of
// 8x8 tiles; or one of
constexpr uint32_t kRectNone = 0xFFFFFFFFu, kRectWide = 0xFFFFFFFEu;
constexpr uint32_t kRectBlock = 1u << 11;
constexpr int kRectMaxTile = 2048;                                     // a rectangle that starts beyond it is not packed: wide

// the parts of the scratch (particle_scratch_words)
struct Scratch {
    uint32_t *wide_count, *pairs_used, *list_count, *list_cursor, *rect, *wide, *pairs;
    uint32_t tiles_x, tiles_y, blocks_x, tiles, lists;   // list t < tiles is tile t's, list tiles + b block b's
    __host__ __device__ Scratch(const ParticleArgs& a) {
        tiles_x = ((uint32_t)a.width + 7u) / 8u; tiles_y = ((uint32_t)a.height + 7u) / 8u;
        blocks_x = (tiles_x + 7u) / 8u;
        tiles = tiles_x * tiles_y;
        lists = (uint32_t)particle_lists(a.width, a.height);
        wide_count = a.scratch; pairs_used = a.scratch + 1;
        list_count = a.scratch + 2; list_cursor = list_count + lists;
        rect = list_cursor + lists; wide = rect + a.count; pairs = wide + a.count;
    }
    // the first list of the rectangle word's rectangle and the step from one of its rows to the next
    __device__ __forceinline__ uint32_t first_list(uint32_t rect, uint32_t* row) const {
        const uint32_t x0 = rect & 0x7FFu, y0 = rect >> 12 & 0x7FFu;
        if (rect & kRectBlock) { *row = blocks_x; return tiles + y0 * blocks_x + x0; }
        *row = tiles_x;
        return y0 * tiles_x + x0;
    }
};

// The box of the particle in words w0 (center, half) and w1 (material, emission, light, reserved), one rounding per corner, and
// whether the record is valid: the derived box is rt_draw_boxes' valid box (which a NaN, an infinity and a half that is not positive
// or vanishes in the rounding all fail), the light exists and the reserved word is 0.
__device__ __forceinline__ void particle_box(uint4 w0, float lo[3], float hi[3]) {
    float c[3];
    rec_xyz(w0, c);
    const float half = __uint_as_float(w0.w);
    for (int k = 0; k < 3; k++) { lo[k] = c[k] - half; hi[k] = c[k] + half; }
}
__device__ __forceinline__ bool particle_valid(uint4 w0, uint4 w1, uint32_t nlights, const float lo[3], const float hi[3]) {
    return __uint_as_float(w0.w) > 0.0f && box_valid(lo, hi) && w1.z < nlights && w1.w == 0u;
}

// May the box touch a pixel of the tiles x0 .. x1 - 1, y0 .. y1 - 1?  (False only where the exact test rejects it for all of them.)
__device__ __forceinline__ bool rect_may_touch(const ParticleArgs& a, const float lo[3], const float hi[3], const float o[3], float omax, int x0, int x1,
                                               int y0, int y1) {
    const TileDirs td = tile_dirs(a, x0 * 8, y0 * 8, omax, (x1 - x0) * 8 - 1, (y1 - y0) * 8 - 1);
    return box_may_touch_tile(lo, hi, o, td, omax, INFINITY);
}

// The rectangle word of a valid box.  Each bisection keeps the invariant "no tile outside the rectangle may be touched": an edge
// moves inwards only past tiles a test has just rejected.  The test need not be monotone for that; a looser answer only leaves the
// rectangle larger.  Two rounds: the second bisects x against the rows the first found, and y against those columns.
__device__ uint32_t particle_rect(const ParticleArgs& a, const float lo[3], const float hi[3]) {
    const float o[3] = {a.origin[0], a.origin[1], a.origin[2]};
    const float omax = rtm_max(rtm_max(rtm_abs(o[0]), rtm_abs(o[1])), rtm_abs(o[2]));
    int x0 = 0, x1 = (a.width + 7) / 8, y0 = 0, y1 = (a.height + 7) / 8;
    if (!rect_may_touch(a, lo, hi, o, omax, x0, x1, y0, y1)) return kRectNone;
    for (int round = 0; round < 2 && (x1 - x0) * (y1 - y0) > 1; round++) {
        for (int l = x0, h = x1; ; ) {            // the low x edge: nothing in x0 .. l - 1
            if (h - l <= 1) { x0 = l; break; }
            const int m = (l + h) >> 1;
            if (!rect_may_touch(a, lo, hi, o, omax, l, m, y0, y1)) l = m; else h = m;
        }
        for (int l = x0, h = x1; ; ) {            // the high x edge: nothing in h .. x1 - 1
            if (h - l <= 1) { x1 = h; break; }
            const int m = (l + h) >> 1;
            if (!rect_may_touch(a, lo, hi, o, omax, m, h, y0, y1)) h = m; else l = m;
        }
        for (int l = y0, h = y1; ; ) {
            if (h - l <= 1) { y0 = l; break; }
            const int m = (l + h) >> 1;
            if (!rect_may_touch(a, lo, hi, o, omax, x0, x1, l, m)) l = m; else h = m;
        }
        for (int l = y0, h = y1; ; ) {
            if (h - l <= 1) { y1 = h; break; }
            const int m = (l + h) >> 1;
            if (!rect_may_touch(a, lo, hi, o, omax, x0, x1, m, h)) h = m; else l = m;
        }
    }
    if (!rect_may_touch(a, lo, hi, o, omax, x0, x1, y0, y1)) return kRectNone;
    uint32_t block = 0u;
    if ((int64_t)(x1 - x0) * (y1 - y0) > (int64_t)kParticleBinTiles) {   // too many tiles: the blocks of 8x8 tiles that hold them
        x0 >>= 3; y0 >>= 3; x1 = (x1 + 7) >> 3; y1 = (y1 + 7) >> 3;
        block = kRectBlock;
    }
    const int w = x1 - x0, h = y1 - y0;
    if ((int64_t)w * h > (int64_t)kParticleBinTiles || x0 >= kRectMaxTile || y0 >= kRectMaxTile) return kRectWide;
    return (uint32_t)x0 | block | (uint32_t)y0 << 12 | (uint32_t)(w - 1) << 24 | (uint32_t)(h - 1) << 28;
}

__global__ __launch_bounds__(kBinWg) void k_particles_bin(ParticleArgs a) {
    const uint32_t i = blockIdx.x * kBinWg + threadIdx.x;
    if (i >= a.count) return;
    const Scratch s(a);
    const uint4 w0 = a.particles[2u * (size_t)i], w1 = a.particles[2u * (size_t)i + 1u];
    float lo[3], hi[3];
    particle_box(w0, lo, hi);
    const uint32_t rect = particle_valid(w0, w1, a.nlights, lo, hi) ? particle_rect(a, lo, hi) : kRectNone;
    s.rect[i] = rect;
    if (rect == kRectNone) return;
    if (rect == kRectWide) {
        s.wide[atomicAdd(s.wide_count, 1u)] = i;      // at most count of them
        return;
    }
    uint32_t row;
    const uint32_t first = s.first_list(rect, &row), w = (rect >> 24 & 0xFu) + 1u, h = (rect >> 28) + 1u;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) atomicAdd(&s.list_count[first + y * row + x], 1u);
}

__global__ __launch_bounds__(kBinWg) void k_particles_offsets(ParticleArgs a) {
    const Scratch s(a);
    const uint32_t t = blockIdx.x * kBinWg + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t n = t < s.lists ? s.list_count[t] : 0u;
    uint32_t upto = n;                                 // the wave's counts up to and with this lane's
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t below = __shfl_up(upto, d, 64);
        if (lane >= (uint32_t)d) upto += below;
    }
    uint32_t first = 0u;
    if (lane == 63u && upto > 0u) first = atomicAdd(s.pairs_used, upto);
    first = __shfl(first, 63, 64);
    if (t < s.lists) s.list_cursor[t] = first + upto - n;
}

__global__ __launch_bounds__(kBinWg) void k_particles_fill(ParticleArgs a) {
    const uint32_t i = blockIdx.x * kBinWg + threadIdx.x;
    if (i >= a.count) return;
    const Scratch s(a);
    const uint32_t rect = s.rect[i];
    if (rect == kRectNone || rect == kRectWide) return;
    uint32_t row;
    const uint32_t first = s.first_list(rect, &row), w = (rect >> 24 & 0xFu) + 1u, h = (rect >> 28) + 1u;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) s.pairs[atomicAdd(&s.list_cursor[first + y * row + x], 1u)] = i;   // the list's own segment
}

__global__ __launch_bounds__(kTileWg) void k_draw_particles(Planes pl, ParticleArgs a) {
    const TileLane tl(a.width, a.height);
    if (!tl.live) return;
    const Scratch s(a);
    const uint32_t tile = (uint32_t)(tl.py0 >> 3) * s.tiles_x + (uint32_t)(tl.px0 >> 3);
    const uint32_t block = s.tiles + (uint32_t)(tl.py0 >> 6) * s.blocks_x + (uint32_t)(tl.px0 >> 6);
    const uint32_t nwide = *s.wide_count, nown = s.list_count[tile], nblock = s.list_count[block];
    if (nwide + nown + nblock == 0u) return;           // (the whole wave)
    // the fill left each cursor at its segment's end
    const uint32_t *own = s.pairs + (s.list_cursor[tile] - nown), *of_block = s.pairs + (s.list_cursor[block] - nblock);
    const size_t pix = tl.pix;

    const float o[3] = {a.origin[0], a.origin[1], a.origin[2]};
    float d[3], inv[3];
    primary_dir(a, tl.px, tl.py, d, inv);
    const float depth = tl.inside ? pl.depth_f32[pix] : -INFINITY;
    const float omax = rtm_max(rtm_max(rtm_abs(o[0]), rtm_abs(o[1])), rtm_abs(o[2]));
    const TileDirs td = tile_dirs(a, tl.px0, tl.py0, omax);
    const float tile_depth = wave_max(depth);

    float best_t = INFINITY;
    uint32_t best = kNoRecord, best_axis = 0u;
    for (int list = 0; list < 3; list++) {
        const uint32_t* ids = list == 0 ? own : (list == 1 ? of_block : s.wide);
        const uint32_t n = list == 0 ? nown : (list == 1 ? nblock : nwide);
        for (uint32_t base = 0; base < n; base += 64u) {
            const uint32_t mine = base + tl.lane;
            uint32_t id = kNoRecord;
            float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f};
            bool keep = false;
            if (mine < n) {
                id = ids[mine];
                particle_box(a.particles[2u * (size_t)id], lo, hi);     // (valid: the bin pass listed it)
                keep = box_may_touch_tile(lo, hi, o, td, omax, tile_depth);
            }
            unsigned long long cand = __ballot(keep);
            while (cand) {
                const int j = __builtin_ctzll(cand);
                cand &= cand - 1ull;
                float blo[3], bhi[3];
                for (int k = 0; k < 3; k++) {
                    blo[k] = __uint_as_float(bcast(__float_as_uint(lo[k]), j));
                    bhi[k] = __uint_as_float(bcast(__float_as_uint(hi[k]), j));
                }
                const uint32_t bid = bcast(id, j);
                float t_in, t_out;
                uint32_t axis;
                const bool hit = ray_box_slab(blo, bhi, o, d, inv, &t_in, &t_out, &axis);
                // the smallest t_in, the lowest index on equal t_in — whatever the order of the list
                if (hit && (t_in < best_t || (t_in == best_t && bid < best))) { best_t = t_in; best = bid; best_axis = axis; }
            }
        }
    }

    if (!tl.inside || best == kNoRecord) return;
    float depth_f;
    uint32_t normal;
    if (!entity_hit_shows(o, d, best_t, best_axis, depth, &depth_f, &normal)) return;
    const uint4 w1 = a.particles[2u * (size_t)best + 1u];    // material, emission, light (< nlights: valid), reserved
    store_entity_pixel(pl, pix, depth_f, normal, w1.x, w1.y, a.lights[w1.z]);
}

}  // namespace

hipError_t launch_draw_particles(const Planes& pl, const ParticleArgs& a, hipStream_t st) {
    if (a.count == 0u || a.width <= 0 || a.height <= 0) return hipSuccess;
    const uint32_t lists = (uint32_t)particle_lists(a.width, a.height);
    hipError_t e = hipMemsetAsync(a.scratch, 0, (2u + (size_t)lists) * sizeof(uint32_t), st);   // the two totals and the lists' counts
    if (e != hipSuccess) return e;
    const dim3 per_particle((a.count + kBinWg - 1u) / kBinWg), per_list((lists + kBinWg - 1u) / kBinWg);
    hipLaunchKernelGGL(k_particles_bin, per_particle, dim3(kBinWg), 0, st, a);
    hipLaunchKernelGGL(k_particles_offsets, per_list, dim3(kBinWg), 0, st, a);
    hipLaunchKernelGGL(k_particles_fill, per_particle, dim3(kBinWg), 0, st, a);
    hipLaunchKernelGGL(k_draw_particles, TileLane::grid(a.width, a.height), dim3(kTileWg), 0, st, pl, a);
    return hipGetLastError();
}

}  // namespace rtd
