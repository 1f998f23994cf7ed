// rt_nav.hip — gfx950 kernels of the navigation fields (rt_nav_build, rt_nav_sample; include/rt_abi.h "Navigation fields", restated
// twice in tests/nav_field_ref.py).  The sets of the search are bitmaps: per (y, z) of the box a row of bits along x, stored in 16-bit
// pieces — piece t holds x = 16 t .. 16 t + 15, the columns one tile owns — nav_row_halves(ex) of them per row, row z * ey + y.
//
//   k_nav_seed     : a thread per piece.  The piece's unoccupied bits (minefield byte != 0) come from at most five aligned dwords of
//             the brick-swizzled minefield — the dwords that meet the piece's texels, none outside the box along x beyond its own
//             dword — and frontier buffer 0 is cleared.  The launch also fills the field (dist 0xFFFF, move 0xFF: a build overwrites
//             every cell) and clears the head, so the scratch needs no fill.
//   k_nav_stand    : a thread per piece.  Standable = unoccupied for `height` cells going up (above the box everything is) and
//             occupied below (under the box a floor is): into unreached buffer 0, counted into RtNavResult.standable.
//   k_nav_goals    : a lane per goal.  The first standable candidate becomes a frontier bit (an atomic OR: duplicates meet) with
//             dist 0; used and dropped goals are counted per wave.
//   k_nav_levels<G>: level launch j runs levels j G + 1 .. (j + 1) G, at most max_dist + 1.  A workgroup owns a tile of 16 x 16
//             columns over the whole z extent, so there is no vertical halo; it loads the tile and a halo of G columns on every side
//             (a row of 16 + 2 G bits is one dword) of the unoccupied, unreached and frontier bits into LDS and runs the levels
//             there: a thread takes rows, and for a row with unreached cells ORs, over the moves that lead from it to a frontier
//             cell, frontier rows shifted by the move and masked by the clearance, which is a running AND of unoccupied rows —
//             going up in the cell's own column for a climb, going down in the neighbour's column for a drop.  A move changes x
//             or y by exactly one, so after g levels every cell at least g columns inside the loaded area is exact, and the owned
//             tile is after G; the box's own border is a true border.  Only owned cells are written: the dist of each newly
//             reached cell, and the unreached and frontier bits into the OTHER buffers, so that a launch reads only what the launch
//             before it wrote.  Head word j + 1 is set if any owned frontier bit is left; a launch whose word is 0 returns at once.
//             Level max_dist + 1 writes no dist: an owned cell reached there sets the truncation word.
//   k_nav_moves    : a thread per cell.  A reached cell that is no goal gets the code of its first move in ORDER to a cell one
//             nearer; the launch also adds the truncation word to the result.
//   k_nav_sample   : a lane per agent: one 16-byte load, at most eleven lookups, two 16-byte stores.
#include <hip/hip_runtime.h>

#include "rt_kernels.hpp"

namespace rtd {

namespace {

constexpr uint32_t kNavWg = 1024;   // sixteen waves

struct NavBits {
    uint16_t *free, *unreached[2], *frontier[2];
};
__device__ __forceinline__ NavBits nav_bits(const NavArgs& a) {
    const size_t bw = 2u * nav_bitmap_words(a.ext);   // pieces per bitmap
    uint16_t* base = reinterpret_cast<uint16_t*>(a.scratch + kNavHeadWords);
    NavBits b;
    b.free = base;
    b.unreached[0] = base + bw; b.unreached[1] = base + 2u * bw;
    b.frontier[0] = base + 3u * bw; b.frontier[1] = base + 4u * bw;
    return b;
}
// the bits of piece t that lie in the box
__device__ __forceinline__ uint32_t nav_piece_mask(int ex, int t) {
    const int n = ex - 16 * t;
    return n >= 16 ? 0xFFFFu : (1u << n) - 1u;
}

__global__ __launch_bounds__(256) void k_nav_seed(const uint8_t* __restrict__ mine_sw, NavArgs a, int logr) {
    const NavBits b = nav_bits(a);
    const int ex = a.ext[0], ey = a.ext[1], ez = a.ext[2], lb = logr - 2;
    const uint32_t rs = nav_row_halves(ex), ntx = ((uint32_t)ex + 15u) >> 4;
    const size_t pieces = (size_t)ey * (size_t)ez * rs, gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t threads = (size_t)gridDim.x * blockDim.x;
    if (gid < kNavSpareResult) a.scratch[gid] = 0u;   // the launch record and the truncation word
    if (gid < pieces) {
        const uint32_t t = (uint32_t)(gid % rs);
        uint32_t f = 0;
        if (t < ntx) {
            const int y = (int)((gid / rs) % (size_t)ey), z = (int)(gid / ((size_t)rs * (size_t)ey));
            const int X0 = a.lo[0] + 16 * (int)t, Y = a.lo[1] + y, Z = a.lo[2] + z;
            const int n = ex - 16 * (int)t < 16 ? ex - 16 * (int)t : 16, xb = X0 & ~3;
            uint32_t bits = 0;
#pragma unroll
            for (int q = 0; q < 5; q++) {
                const int Xq = xb + 4 * q;
                if (Xq + 3 < X0 || Xq > X0 + n - 1) continue;   // (a dword that meets no texel of the piece is not read)
                const uint32_t dw = *reinterpret_cast<const uint32_t*>(mine_sw + swizzled_index(Xq, Y, Z, lb));
#pragma unroll
                for (int j = 0; j < 4; j++) bits |= (uint32_t)(((dw >> (8 * j)) & 0xFFu) != 0u) << (4 * q + j);
            }
            f = (bits >> (X0 & 3)) & ((1u << n) - 1u);
        }
        b.free[gid] = (uint16_t)f;
        b.frontier[0][gid] = 0;
    }
    const size_t cells = (size_t)ex * (size_t)ey * (size_t)ez;
    for (size_t c = gid; c < cells; c += threads) {
        a.dist[c] = 0xFFFFu;
        a.move[c] = 0xFFu;
    }
}

__global__ __launch_bounds__(256) void k_nav_stand(NavArgs a) {
    const NavBits b = nav_bits(a);
    const int ex = a.ext[0], ey = a.ext[1], ez = a.ext[2];
    const uint32_t rs = nav_row_halves(ex), ntx = ((uint32_t)ex + 15u) >> 4;
    const size_t pieces = (size_t)ey * (size_t)ez * rs, gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, up = (size_t)rs * (size_t)ey;
    uint32_t s = 0;
    if (gid < pieces) {
        const uint32_t t = (uint32_t)(gid % rs);
        if (t < ntx) {
            const int z = (int)(gid / up);
            s = b.free[gid];
            for (int j = 1; j < a.height; j++)
                if (z + j < ez) s &= b.free[gid + (size_t)j * up];
            if (z > 0) s &= ~(uint32_t)b.free[gid - up];
        }
        b.unreached[0][gid] = (uint16_t)s;
    }
    uint32_t n = (uint32_t)__popc(s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if ((threadIdx.x & 63u) == 0u && n) atomicAdd(a.result + 0, n);
}

__global__ __launch_bounds__(256) void k_nav_goals(NavArgs a) {
    const NavBits b = nav_bits(a);
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    const int ex = a.ext[0], ey = a.ext[1], ez = a.ext[2];
    const uint32_t rs = nav_row_halves(ex);
    bool have = g < a.goal_count, used = false;
    if (have) {
        const int4 c = a.goals[g];
        const int x = c.x - a.lo[0], y = c.y - a.lo[1], z0 = c.z - a.lo[2];
        if (x >= 0 && x < ex && y >= 0 && y < ey) {
            for (int s = 0; s <= a.goal_snap && !used; s++) {
                const int z = z0 - s;
                if (z < 0) break;
                if (z >= ez) continue;
                const size_t piece = ((size_t)z * (size_t)ey + (size_t)y) * rs + (size_t)(x >> 4);
                if (((b.unreached[0][piece] >> (x & 15)) & 1u) == 0u) continue;
                atomicOr(reinterpret_cast<uint32_t*>(b.frontier[0]) + (piece >> 1), 1u << (16u * (uint32_t)(piece & 1u) + (uint32_t)(x & 15)));
                a.dist[((size_t)z * (size_t)ey + (size_t)y) * (size_t)ex + (size_t)x] = 0u;   // (every writer stores the same value)
                used = true;
            }
        }
    }
    const uint32_t nu = (uint32_t)__popcll(__ballot(have && used)), nd = (uint32_t)__popcll(__ballot(have && !used));
    if ((threadIdx.x & 63u) == 0u) {
        if (nu) atomicAdd(a.result + 4, nu);
        if (nd) atomicAdd(a.result + 5, nd);
    }
}

// the 16 + 2 G bits of a row from x = 16 t - G on (pieces outside the row count as empty)
template <int G>
__device__ __forceinline__ uint32_t nav_window(const uint16_t* row, int t, int ntx) {
    const uint64_t v = (t > 0 ? (uint64_t)row[t - 1] : 0ull) | ((uint64_t)row[t] << 16) | (t + 1 < ntx ? (uint64_t)row[t + 1] << 32 : 0ull);
    return (uint32_t)(v >> (16 - G)) & (uint32_t)((1ull << (16 + 2 * G)) - 1ull);
}

template <int G>
__global__ __launch_bounds__(kNavWg) void k_nav_levels(NavArgs a, uint32_t j) {
    constexpr int W = 16 + 2 * G;                // rows of the loaded area along y, and bits of a row
    constexpr int kRows = W * 256;               // rows of the loaded area at the largest z extent
    constexpr int kPer = (kRows + (int)kNavWg - 1) / (int)kNavWg;   // rows per thread
    __shared__ uint32_t free_s[kRows], unre_s[kRows], fron_s[kRows];
    if (j > 0u && a.scratch[j] == 0u) return;    // the frontier has died (one address: the exit is the workgroup's)
    const int tid = threadIdx.x, lane = tid & 63;
    const int ex = a.ext[0], ey = a.ext[1], ez = a.ext[2], ntx = (ex + 15) >> 4;
    const uint32_t rs = nav_row_halves(ex);
    const int tx = (int)(blockIdx.x % (uint32_t)ntx), ty = (int)(blockIdx.x / (uint32_t)ntx);
    const NavBits b = nav_bits(a);
    const uint16_t *uin = b.unreached[j & 1u], *fin = b.frontier[j & 1u];
    uint16_t *uout = b.unreached[(j + 1u) & 1u], *fout = b.frontier[(j + 1u) & 1u];
    const int n = W * ez;
    const int height = a.height, max_climb = a.max_climb, max_drop = a.max_drop;

    // ---- the tile and its halo into LDS; at launch 0 the goal cells are what is reached so far -----------------------------------
    int any = 0;
    uint32_t count = 0, maxlvl = 0;
#pragma unroll
    for (int i = 0; i < kPer; i++) {
        const int r = tid + (int)kNavWg * i;
        if (r >= n) continue;
        const int z = r / W, yl = r - z * W, y = 16 * ty - G + yl;
        uint32_t f = 0, u = 0, fr = 0;
        if (y >= 0 && y < ey) {
            const size_t base = ((size_t)z * (size_t)ey + (size_t)y) * rs;
            f = nav_window<G>(b.free + base, tx, ntx);
            fr = nav_window<G>(fin + base, tx, ntx);
            u = nav_window<G>(uin + base, tx, ntx) & ~fr;
        }
        free_s[r] = f; unre_s[r] = u; fron_s[r] = fr;
        any |= fr != 0u;
        if (j == 0u && yl >= G && yl < G + 16) count += (uint32_t)__popc((fr >> G) & 0xFFFFu);
    }
    any = __syncthreads_or(any);

    const uint32_t first = j * (uint32_t)G + 1u;
    const uint32_t last = first + (uint32_t)G - 1u < a.max_dist + 1u ? first + (uint32_t)G - 1u : a.max_dist + 1u;
    int trunc = 0;
    for (uint32_t lvl = first; any && lvl <= last; lvl++) {
        uint32_t nw[kPer];
#pragma unroll
        for (int i = 0; i < kPer; i++) {
            nw[i] = 0u;
            const int r = tid + (int)kNavWg * i;
            if (r >= n) continue;
            const uint32_t u = unre_s[r];
            if (u == 0u) continue;
            const int z = r / W, yl = r - z * W;
            const bool ym = yl > 0, yp = yl + 1 < W;
            uint32_t got = 0;
            // level and climbing moves (k = 0 .. max_climb): this cell is the lower one, its own column must be free further up
            uint32_t cu = u;
            for (int k = 0; k <= max_climb && z + k < ez; k++) {
                if (k > 0 && z + k + height - 1 < ez) cu &= free_s[r + (k + height - 1) * W];
                const int rb = r + k * W;
                const uint32_t c = fron_s[rb];
                uint32_t m = (c >> 1) | (c << 1);
                if (ym) m |= fron_s[rb - 1];
                if (yp) m |= fron_s[rb + 1];
                got |= cu & m;
            }
            // dropping moves (k = -1 .. -max_drop): the target is the lower one, ITS column must be free from its level up to this
            // cell's head: a running AND per direction, going down
            if (max_drop > 0 && z > 0) {
                uint32_t t0 = ~0u, t1 = ~0u, t2 = ym ? ~0u : 0u, t3 = yp ? ~0u : 0u;
                for (int q = 0; q < height && z + q < ez; q++) {
                    const int rq = r + q * W;
                    const uint32_t fc = free_s[rq];
                    t0 &= fc >> 1; t1 &= fc << 1;
                    if (ym) t2 &= free_s[rq - 1];
                    if (yp) t3 &= free_s[rq + 1];
                }
                for (int k = 1; k <= max_drop && z - k >= 0; k++) {
                    const int rb = r - k * W;
                    const uint32_t fc = free_s[rb], c = fron_s[rb];
                    t0 &= fc >> 1; t1 &= fc << 1;
                    got |= (t0 & (c >> 1)) | (t1 & (c << 1));
                    if (ym) { t2 &= free_s[rb - 1]; got |= t2 & fron_s[rb - 1]; }
                    if (yp) { t3 &= free_s[rb + 1]; got |= t3 & fron_s[rb + 1]; }
                }
            }
            nw[i] = got & u;
        }
        __syncthreads();   // every row of this level's frontier has been read
        int more = 0;
#pragma unroll
        for (int i = 0; i < kPer; i++) {
            const int r = tid + (int)kNavWg * i;
            if (r >= n) continue;
            const uint32_t v = nw[i];
            fron_s[r] = v;
            if (v == 0u) continue;
            unre_s[r] &= ~v;
            more = 1;
            const int z = r / W, yl = r - z * W;
            uint32_t own = yl >= G && yl < G + 16 ? (v >> G) & 0xFFFFu : 0u;
            if (own == 0u) continue;
            if (lvl > a.max_dist) { trunc = 1; continue; }
            count += (uint32_t)__popc(own);
            maxlvl = lvl;
            const size_t cell = ((size_t)z * (size_t)ey + (size_t)(16 * ty + yl - G)) * (size_t)ex + (size_t)(16 * tx);
            while (own) {   // at most sixteen bits
                const int x = __builtin_ctz(own);
                own &= own - 1u;
                a.dist[cell + x] = (uint16_t)lvl;
            }
        }
        any = __syncthreads_or(more);
    }

    // ---- the owned rows back, into the other buffers (a thread's own rows: nobody else wrote them) ------------------------------
    int left = 0;
#pragma unroll
    for (int i = 0; i < kPer; i++) {
        const int r = tid + (int)kNavWg * i;
        if (r >= n) continue;
        const int z = r / W, yl = r - z * W, y = 16 * ty - G + yl;
        if (yl < G || yl >= G + 16 || y >= ey) continue;
        const size_t piece = ((size_t)z * (size_t)ey + (size_t)y) * rs + (size_t)tx;
        const uint32_t fo = (fron_s[r] >> G) & 0xFFFFu;
        uout[piece] = (uint16_t)((unre_s[r] >> G) & 0xFFFFu);
        fout[piece] = (uint16_t)fo;
        left |= fo != 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        count += __shfl_xor(count, off);
        const uint32_t o = __shfl_xor(maxlvl, off);
        maxlvl = o > maxlvl ? o : maxlvl;
    }
    if (lane == 0) {
        if (count) atomicAdd(a.result + 1, count);
        if (maxlvl) atomicMax(a.result + 2, maxlvl);
    }
    left = __syncthreads_or(left);
    trunc = __syncthreads_or(trunc);
    if (tid == 0) {   // (every writer stores the same value)
        if (left && last <= a.max_dist) a.scratch[j + 1u] = 1u;
        if (trunc) a.scratch[kNavTruncWord] = 1u;
    }
}

__device__ __forceinline__ bool nav_free_at(const uint16_t* freeb, uint32_t rs, int ey, int ez, int x, int y, int z) {
    if (z >= ez) return true;
    return ((freeb[((size_t)z * (size_t)ey + (size_t)y) * rs + (size_t)(x >> 4)] >> (x & 15)) & 1u) != 0u;
}

__global__ __launch_bounds__(256) void k_nav_moves(NavArgs a) {
    const int ex = a.ext[0], ey = a.ext[1], ez = a.ext[2];
    const size_t cells = (size_t)ex * (size_t)ey * (size_t)ez, c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && a.scratch[kNavTruncWord] != 0u) atomicAdd(a.result + 3, 1u);
    if (c >= cells) return;
    const uint32_t d = a.dist[c];
    if (d == 0u || d == 0xFFFFu) return;   // (the seed launch wrote 0xFF)
    const uint16_t* freeb = nav_bits(a).free;
    const uint32_t rs = nav_row_halves(ex);
    const int x = (int)(c % (size_t)ex), y = (int)((c / (size_t)ex) % (size_t)ey), z = (int)(c / ((size_t)ex * (size_t)ey));
    const int height = a.height, max_climb = a.max_climb, max_drop = a.max_drop;
    // CLEAR of this cell, as far as a climb asks
    int clear = height;
    while (clear < height + max_climb && nav_free_at(freeb, rs, ey, ez, x, y, z + clear)) clear++;
    for (int h = 0; h < 4; h++) {
        const int nx = x + (h == 0) - (h == 1), ny = y + (h == 2) - (h == 3);
        if (nx < 0 || nx >= ex || ny < 0 || ny >= ey) continue;
        // the neighbour column's free cells going down from this cell's head, as far as a drop asks
        int down = 0;
        while (down < height + max_drop && z + height - 1 - down >= 0 && nav_free_at(freeb, rs, ey, ez, nx, ny, z + height - 1 - down)) down++;
        for (int k = max_climb; k >= -max_drop; k--) {
            const int zb = z + k;
            if (zb < 0 || zb >= ez) continue;
            if ((uint32_t)a.dist[((size_t)zb * (size_t)ey + (size_t)ny) * (size_t)ex + (size_t)nx] != d - 1u) continue;
            if (k > 0 ? clear < k + height : down < height - k) continue;
            a.move[c] = (uint8_t)(h | ((k + 8) << 2));
            return;
        }
    }
}

__global__ __launch_bounds__(256) void k_nav_sample(NavSampleArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    const uint4 ag = a.agents[i];
    const float px = __uint_as_float(ag.x), py = __uint_as_float(ag.y), pz = __uint_as_float(ag.z);
    const int snap_down = (int)(ag.w & 0xFFu), snap_up = (int)((ag.w >> 8) & 0xFFu);
    const float lim = 1048576.0f;
    // (a NaN fails every comparison)
    const bool valid = (ag.w >> 16) == 0u && snap_down <= 8 && snap_up <= 2 && px > -lim && px < lim && py > -lim && py < lim && pz > -lim && pz < lim;
    int cx = -1, cy = -1, cz = -1, nx = -1, ny = -1, nz = -1;
    uint32_t dist = 0xFFFFFFFFu, move = 0xFFu;
    if (valid) {
        cx = (int)floorf(px); cy = (int)floorf(py); cz = (int)floorf(pz);
        nx = cx; ny = cy; nz = cz;
        const int x = cx - a.lo[0], y = cy - a.lo[1], z0 = cz - a.lo[2];
        if (x >= 0 && x < a.ext[0] && y >= 0 && y < a.ext[1]) {
            for (int s = 0; s <= snap_down + snap_up; s++) {
                const int z = s <= snap_down ? z0 - s : z0 + (s - snap_down);
                if (z < 0 || z >= a.ext[2]) continue;
                const size_t c = ((size_t)z * (size_t)a.ext[1] + (size_t)y) * (size_t)a.ext[0] + (size_t)x;
                const uint32_t d = a.dist[c];
                if (d == 0xFFFFu) continue;
                dist = d;
                cz = z + a.lo[2];
                nz = cz;
                if (d > 0u) {
                    move = a.move[c];
                    const uint32_t h = move & 3u;
                    nx = cx + (h == 0u) - (h == 1u);
                    ny = cy + (h == 2u) - (h == 3u);
                    nz = cz + (int)(move >> 2) - 8;
                }
                break;
            }
        }
    }
    a.steps[2u * i] = make_uint4((uint32_t)cx, (uint32_t)cy, (uint32_t)cz, dist);
    a.steps[2u * i + 1u] = make_uint4((uint32_t)nx, (uint32_t)ny, (uint32_t)nz, move);
}

template <int G>
void launch_nav_levels(const NavArgs& a, uint32_t tiles, hipStream_t st, hipError_t* e) {
    const uint32_t launches = (a.max_dist + 1u + (uint32_t)G - 1u) / (uint32_t)G;
    for (uint32_t j = 0; j < launches && *e == hipSuccess; j++) {
        hipLaunchKernelGGL(k_nav_levels<G>, dim3(tiles), dim3(kNavWg), 0, st, a, j);
        *e = hipGetLastError();
    }
}

}  // namespace

hipError_t launch_nav_build(const uint8_t* mine_sw, int logr, const NavArgs& a, uint32_t levels, hipStream_t st) {
    if (logr < 8 || logr > 10 || !mine_sw || !a.scratch || !a.dist || !a.move || !a.result || a.max_dist < 1u || a.max_dist > kNavMaxDist ||
        a.goal_count > kNavMaxGoals || (a.goal_count > 0u && !a.goals) || a.height < 1 || a.height > 4 || a.max_climb < 0 || a.max_climb > 2 ||
        a.max_drop < 0 || a.max_drop > 8 || a.goal_snap < 0 || a.goal_snap > 8 || (levels != 1u && levels != 4u && levels != 8u))
        return hipErrorInvalidValue;
    for (int k = 0; k < 3; k++)
        if (a.ext[k] < 1 || a.ext[k] > 256 || a.lo[k] < 0 || a.ext[k] > (1 << logr) - a.lo[k]) return hipErrorInvalidValue;
    const size_t pieces = 2u * nav_bitmap_words(a.ext), cells = (size_t)a.ext[0] * (size_t)a.ext[1] * (size_t)a.ext[2];
    const size_t seed_threads = pieces > kNavSpareResult ? pieces : kNavSpareResult;
    const uint32_t tiles = (((uint32_t)a.ext[0] + 15u) >> 4) * (((uint32_t)a.ext[1] + 15u) >> 4);
    hipLaunchKernelGGL(k_nav_seed, dim3((uint32_t)((seed_threads + 255u) / 256u)), dim3(256), 0, st, mine_sw, a, logr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_nav_stand, dim3((uint32_t)((pieces + 255u) / 256u)), dim3(256), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.goal_count > 0u) {
        hipLaunchKernelGGL(k_nav_goals, dim3((a.goal_count + 255u) / 256u), dim3(256), 0, st, a);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (levels == 1u) launch_nav_levels<1>(a, tiles, st, &e);
        else if (levels == 4u) launch_nav_levels<4>(a, tiles, st, &e);
        else launch_nav_levels<8>(a, tiles, st, &e);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_nav_moves, dim3((uint32_t)((cells + 255u) / 256u)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_nav_sample(const NavSampleArgs& a, hipStream_t st) {
    if (!a.dist || !a.move || !a.agents || !a.steps || a.count < 1u || a.count > kNavMaxAgents) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_nav_sample, dim3((a.count + 255u) / 256u), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace rtd
