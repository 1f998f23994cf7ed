// rt_flow.hip — gfx950 kernels of rt_flow_voxels / rt_flow_voxels_async: a level-based fluid spreads, falls and dries inside a box of
// texels (include/rt_abi.h "Fluid flow"; the rules are restated twice in tests/flow_voxels_ref.py).
//
//   k_flow_seed    : one lane per cell of the clipped box.  The cell's state from its minefield byte and, where that is 0, its
//             material word: 0 empty (a fluid cell of strength 0 too: it gives nothing and holds nothing up), 1..13 flowing with that
//             strength, 14 source, 15 fixed.  The first workgroup clears the launch words of the scratch's head and sets the chunk flags.
//   k_flow_ticks<G>: tick launch j runs ticks j G + 1 .. min((j + 1) G, ticks).  A workgroup owns a tile of 32 x 16 x 16 cells and loads
//             it with a halo of G cells into LDS (a cell outside the box loads as FIXED: it gives nothing, takes nothing and is the floor
//             under the low z face).  A tick's dependencies lie within Chebyshev distance 1 — the farthest are c + z and n - z —, so
//             tick t is exact on the cells at least t away from the loaded area's faces: it reads one LDS buffer over [t - 1, D - t + 1)
//             and writes the other over [t, D - t), and after n <= G ticks the interior is exact.  Every tick ORs whether an interior
//             cell changed into the launch's word; the workgroups of a launch whose predecessor's word is still 0 return at once (the
//             state is a fixed point and both arrays hold it).  A tile with no fluid in the loaded area is copied through.
//   k_flow_apply   : one lane per cell.  The final byte and word from the final state and the world as it stands: a flowing cell is
//             occupied with its strength in the level field, a cell that was fluid and is empty holds air_material and a non-zero byte
//             (the chunk pass gives the final value); only what differs is written, and a cell whose occupancy changed stores 0 to its
//             chunk's flag word.  One more tick from the global states counts `active`.  The counts are summed per wave and added with
//             one atomic per wave and counter.
//   k_flow_chunks  : one workgroup per chunk of the box, as k_settle_chunks: behind the flag word's early exit, the chunk rebuild
//             (rt_rebuild_chunk.hpp) with a stage that does nothing.
//   (k_rebuild_chunk_maps, rt_edit.hip, follows over the same chunk list.)
#include <hip/hip_runtime.h>

#include "rt_kernels.hpp"
#include "rt_rebuild_chunk.hpp"

namespace rtd {

namespace {

constexpr uint32_t kFlowWg = 256;
constexpr int kTX = 32, kTY = 16, kTZ = 16;   // a tile's interior

__device__ __forceinline__ uint8_t* flow_states(const FlowArgs& a, uint32_t which) {
    return reinterpret_cast<uint8_t*>(a.scratch + kFlowHeadWords + (size_t)which * flow_state_words(a.lo, a.hi));
}

// One tick of a cell that is neither a source nor fixed: `up` the state of c + z, n[k] the four horizontal neighbours and b[k] the
// cells under them.  D = max_level under a source or a flowing cell; S = the largest e(n) - 1 over the spreading neighbours.
__device__ __forceinline__ uint32_t flow_next(uint32_t up, const uint32_t n[4], const uint32_t b[4], uint32_t max_level) {
    uint32_t s = (up - 1u) < kFlowSource ? max_level : 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const bool source = n[k] == kFlowSource;
        const bool gives = (n[k] - 1u) < kFlowSource && (source || b[k] == kFlowFixed);
        const uint32_t e1 = source ? max_level : n[k] - 1u;
        if (gives && e1 > s) s = e1;
    }
    return s;
}

template <int LOGR>
__global__ __launch_bounds__(kFlowWg) void k_flow_seed(const uint8_t* __restrict__ mine_sw, const uint32_t* __restrict__ mat_sw, FlowArgs a) {
    const uint32_t ex = (uint32_t)(a.hi[0] - a.lo[0] + 1), ey = (uint32_t)(a.hi[1] - a.lo[1] + 1), ez = (uint32_t)(a.hi[2] - a.lo[2] + 1);
    const uint32_t sx = flow_row_cells((int)ex);
    if (blockIdx.x == 0u)
        for (uint32_t i = threadIdx.x; i < (uint32_t)kFlowHeadWords; i += kFlowWg) {
            if (i < (uint32_t)kFlowSpareCount) a.scratch[i] = 0u;
            else if (i >= (uint32_t)kFlowChunkFlags) a.scratch[i] = 0xFFFFFFFFu;
        }
    const uint32_t g = blockIdx.x * kFlowWg + threadIdx.x;
    const uint32_t x = g % sx, row = g / sx, y = row % ey, z = row / ey;
    if (x >= ex || z >= ez) return;   // (a row's pad cells stay unwritten here: every load of a state tests x < ex, so none is ever read)
    const uint32_t idx = swizzled_index(a.lo[0] + (int)x, a.lo[1] + (int)y, a.lo[2] + (int)z, LOGR - 2);
    uint32_t s = 0u;
    if (mine_sw[idx] == 0u) {
        const uint32_t w = mat_sw[idx], v = (w >> a.level_shift) & 0xFu;
        s = (w & a.fluid_mask) != a.fluid_value ? kFlowFixed : v == 15u ? kFlowSource : v < a.max_level ? v : a.max_level;
    }
    flow_states(a, 0u)[g] = (uint8_t)s;
}

template <int G>
__global__ __launch_bounds__(kFlowWg) void k_flow_ticks(FlowArgs a, uint32_t j, uint32_t n) {
    constexpr int DX = kTX + 2 * G, DY = kTY + 2 * G, DZ = kTZ + 2 * G, N = DX * DY * DZ, P = DX * DY;
    __shared__ uint8_t buf[2][N];
    if (j > 0u && a.scratch[j - 1u] == 0u) return;   // the launch before changed nothing (one address: the exit is the workgroup's)
    const int tid = (int)threadIdx.x;
    const int ex = a.hi[0] - a.lo[0] + 1, ey = a.hi[1] - a.lo[1] + 1, ez = a.hi[2] - a.lo[2] + 1;
    const uint32_t sx = flow_row_cells(ex);
    const uint32_t ntx = (uint32_t)(ex + kTX - 1) / kTX, nty = (uint32_t)(ey + kTY - 1) / kTY;
    const int tx = (int)(blockIdx.x % ntx), ty = (int)((blockIdx.x / ntx) % nty), tz = (int)(blockIdx.x / (ntx * nty));
    const uint8_t* in = flow_states(a, j & 1u);
    uint8_t* out = flow_states(a, (j + 1u) & 1u);

    // ---- the tile and its halo into LDS ------------------------------------------------------------------------------------------
    int any = 0;
    for (int i = tid; i < N; i += (int)kFlowWg) {
        const int lx = i % DX, r = i / DX, ly = r % DY, lz = r / DY;
        const int x = tx * kTX - G + lx, y = ty * kTY - G + ly, z = tz * kTZ - G + lz;
        uint32_t s = kFlowFixed;
        if ((uint32_t)x < (uint32_t)ex && (uint32_t)y < (uint32_t)ey && (uint32_t)z < (uint32_t)ez) s = in[((size_t)z * (size_t)ey + (size_t)y) * sx + (size_t)x];
        buf[0][i] = (uint8_t)s;
        any |= (s - 1u) < kFlowSource;
    }
    any = __syncthreads_or(any);

    // ---- n ticks, each on the cells that are still exact -----------------------------------------------------------------------------
    int changed = 0;
    uint32_t fin = 0u;
    if (any) {
#pragma unroll
        for (int t = 1; t <= G; t++) {
            if ((uint32_t)t <= n) {
                const uint8_t* src = buf[(t - 1) & 1];
                uint8_t* dst = buf[t & 1];
                const int RX = DX - 2 * t, RY = DY - 2 * t, RZ = DZ - 2 * t;
                for (int i = tid; i < RX * RY * RZ; i += (int)kFlowWg) {
                    const int lx = t + i % RX, r = i / RX, ly = t + r % RY, lz = t + r / RY;
                    const int c = lz * P + ly * DX + lx;
                    const uint32_t s = src[c];
                    uint32_t ns = s;
                    if (s < kFlowSource) {
                        const uint32_t nb[4] = {src[c - 1], src[c + 1], src[c - DX], src[c + DX]};
                        const uint32_t bl[4] = {src[c - 1 - P], src[c + 1 - P], src[c - DX - P], src[c + DX - P]};
                        ns = flow_next(src[c + P], nb, bl, a.max_level);
                        const bool interior = (uint32_t)(lx - G) < (uint32_t)kTX && (uint32_t)(ly - G) < (uint32_t)kTY && (uint32_t)(lz - G) < (uint32_t)kTZ;
                        changed |= (interior && ns != s) ? 1 : 0;
                    }
                    dst[c] = (uint8_t)ns;
                }
                __syncthreads();
            }
        }
        fin = n & 1u;
    }
    changed = __syncthreads_or(changed);
    if (changed && tid == 0) a.scratch[j] = 1u;   // (every writer stores the same value)

    // ---- the interior back, four cells a lane: rows are padded to four cells and a tile starts on a multiple of 32 ----------------------
    const uint8_t* src = buf[fin];
    for (int i = tid; i < (kTX / 4) * kTY * kTZ; i += (int)kFlowWg) {
        const int qx = i % (kTX / 4), r = i / (kTX / 4), ly = r % kTY, lz = r / kTY;
        const int x = tx * kTX + 4 * qx, y = ty * kTY + ly, z = tz * kTZ + lz;
        if (x >= ex || y >= ey || z >= ez) continue;
        const int c = (lz + G) * P + (ly + G) * DX + G + 4 * qx;
        const uint32_t v = (uint32_t)src[c] | ((uint32_t)src[c + 1] << 8) | ((uint32_t)src[c + 2] << 16) | ((uint32_t)src[c + 3] << 24);
        *reinterpret_cast<uint32_t*>(out + ((size_t)z * (size_t)ey + (size_t)y) * sx + (size_t)x) = v;
    }
}

template <int LOGR>
__global__ __launch_bounds__(kFlowWg) void k_flow_apply(uint8_t* __restrict__ mine_sw, uint32_t* __restrict__ mat_sw, FlowArgs a, uint32_t which) {
    const int ex = a.hi[0] - a.lo[0] + 1, ey = a.hi[1] - a.lo[1] + 1, ez = a.hi[2] - a.lo[2] + 1;
    const uint32_t sx = flow_row_cells(ex);
    const uint32_t g = blockIdx.x * kFlowWg + threadIdx.x;
    const int x = (int)(g % sx), y = (int)((g / sx) % (uint32_t)ey), z = (int)(g / sx / (uint32_t)ey);
    const uint8_t* cur = flow_states(a, which);
    uint32_t wetted = 0, dried = 0, changed = 0, active = 0;
    if (x < ex && z < ez) {
        const uint32_t f = cur[g], field = 0xFu << a.level_shift;
        const int vx = a.lo[0] + x, vy = a.lo[1] + y, vz = a.lo[2] + z;
        const uint32_t idx = swizzled_index(vx, vy, vz, LOGR - 2);
        const bool flowing = (f - 1u) < kFlowMaxLevel;
        bool dirty = false;
        if (mine_sw[idx] == 0u) {
            const uint32_t w = mat_sw[idx];
            if ((w & a.fluid_mask) == a.fluid_value && ((w >> a.level_shift) & 0xFu) != 15u) {   // it was a flowing cell
                if (flowing) {
                    const uint32_t nw = (w & ~field) | (f << a.level_shift);
                    if (nw != w) { mat_sw[idx] = nw; changed = 1u; }
                } else {
                    mine_sw[idx] = 1u;
                    mat_sw[idx] = a.air_material;
                    dried = 1u; changed = 1u; dirty = true;
                }
            }
        } else if (flowing) {
            mine_sw[idx] = 0u;
            mat_sw[idx] = a.fluid_word | (f << a.level_shift);
            wetted = 1u; changed = 1u; dirty = true;
        }
        if (dirty) {   // flags are z-major over the box's chunks
            const int ncx = (a.hi[0] >> 6) - (a.lo[0] >> 6) + 1, ncy = (a.hi[1] >> 6) - (a.lo[1] >> 6) + 1;
            const int ci = (((vz >> 6) - (a.lo[2] >> 6)) * ncy + ((vy >> 6) - (a.lo[1] >> 6))) * ncx + ((vx >> 6) - (a.lo[0] >> 6));
            a.scratch[kFlowChunkFlags + (size_t)ci] = 0u;
        }
        if (f < kFlowSource) {   // one more tick, from the global states
            auto at = [&](int px, int py, int pz) -> uint32_t {
                if ((uint32_t)px >= (uint32_t)ex || (uint32_t)py >= (uint32_t)ey || (uint32_t)pz >= (uint32_t)ez) return kFlowFixed;
                return cur[((size_t)pz * (size_t)ey + (size_t)py) * sx + (size_t)px];
            };
            const uint32_t nb[4] = {at(x - 1, y, z), at(x + 1, y, z), at(x, y - 1, z), at(x, y + 1, z)};
            const uint32_t bl[4] = {at(x - 1, y, z - 1), at(x + 1, y, z - 1), at(x, y - 1, z - 1), at(x, y + 1, z - 1)};
            active = flow_next(at(x, y, z + 1), nb, bl, a.max_level) != f ? 1u : 0u;
        }
    }
    // sums per wave, one atomic per wave and counter
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        wetted += __shfl_xor(wetted, off);
        dried += __shfl_xor(dried, off);
        changed += __shfl_xor(changed, off);
        active += __shfl_xor(active, off);
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (wetted) atomicAdd(a.counts + 0, wetted);
        if (dried) atomicAdd(a.counts + 1, dried);
        if (changed) atomicAdd(a.counts + 2, changed);
        if (active) atomicAdd(a.counts + 3, active);
    }
}

// the chunk rebuild's edit stage of a call whose edits the apply pass has already written
struct NoStage {
    __device__ __forceinline__ void operator()(uint32_t*, uint32_t, uint32_t, uint32_t, int, int) const {}
};

// One workgroup per chunk of the box, in the order of the chunk list.  The flag word is read by every thread (one address: a uniform
// value), so the exit is the workgroup's.
__global__ __launch_bounds__(1024) void k_flow_chunks(uint8_t* __restrict__ mine_sw, const uint32_t* __restrict__ chunks, FlowArgs a, int logr) {
    if (a.scratch[kFlowChunkFlags + blockIdx.x] != 0u) return;   // no cell of this chunk changed its occupancy: its bytes stay as they are
    if (threadIdx.x == 0) atomicAdd(a.counts + 4, 1u);
    rebuild_chunk(mine_sw, chunks, logr, NoStage{});
}

template <int G>
void launch_ticks(const FlowArgs& a, uint32_t tiles, hipStream_t st, hipError_t* e) {
    const uint32_t launches = (a.ticks + (uint32_t)G - 1u) / (uint32_t)G;
    for (uint32_t j = 0; j < launches && *e == hipSuccess; j++) {
        const uint32_t left = a.ticks - j * (uint32_t)G;
        hipLaunchKernelGGL(k_flow_ticks<G>, dim3(tiles), dim3(kFlowWg), 0, st, a, j, left < (uint32_t)G ? left : (uint32_t)G);
        *e = hipGetLastError();
    }
}

}  // namespace

hipError_t launch_flow_voxels(uint8_t* mine_sw, uint32_t* mat_sw, const uint32_t* chunks, uint32_t nchunks, int logr, const FlowArgs& a,
                              uint32_t group, hipStream_t st) {
    if (logr < 8 || logr > 10 || nchunks < 1u || nchunks > kFlowMaxChunks || a.ticks < 1u || a.ticks > kFlowMaxTicks || a.level_shift > 28u ||
        a.max_level < 1u || a.max_level > kFlowMaxLevel || (group != 1u && group != 2u && group != 4u && group != 8u) || !a.scratch || !a.counts)
        return hipErrorInvalidValue;
    uint64_t boxchunks = 1;
    for (int k = 0; k < 3; k++) {
        if (a.lo[k] < 0 || a.hi[k] >= (1 << logr) || a.lo[k] > a.hi[k] || a.hi[k] - a.lo[k] + 1 > kFlowMaxExtent) return hipErrorInvalidValue;
        boxchunks *= (uint64_t)((a.hi[k] >> 6) - (a.lo[k] >> 6) + 1);
    }
    if (boxchunks != nchunks) return hipErrorInvalidValue;
    const int ex = a.hi[0] - a.lo[0] + 1, ey = a.hi[1] - a.lo[1] + 1, ez = a.hi[2] - a.lo[2] + 1;
    const uint32_t cells = flow_row_cells(ex) * (uint32_t)ey * (uint32_t)ez, grid = (cells + kFlowWg - 1u) / kFlowWg;
    const uint32_t tiles = (uint32_t)((ex + kTX - 1) / kTX) * (uint32_t)((ey + kTY - 1) / kTY) * (uint32_t)((ez + kTZ - 1) / kTZ);
    const uint32_t launches = (a.ticks + group - 1u) / group;

    if (logr == 8) hipLaunchKernelGGL(k_flow_seed<8>, dim3(grid), dim3(kFlowWg), 0, st, mine_sw, mat_sw, a);
    else if (logr == 9) hipLaunchKernelGGL(k_flow_seed<9>, dim3(grid), dim3(kFlowWg), 0, st, mine_sw, mat_sw, a);
    else hipLaunchKernelGGL(k_flow_seed<10>, dim3(grid), dim3(kFlowWg), 0, st, mine_sw, mat_sw, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (group == 1u) launch_ticks<1>(a, tiles, st, &e);
    else if (group == 2u) launch_ticks<2>(a, tiles, st, &e);
    else if (group == 4u) launch_ticks<4>(a, tiles, st, &e);
    else launch_ticks<8>(a, tiles, st, &e);
    if (e != hipSuccess) return e;
    if (logr == 8) hipLaunchKernelGGL(k_flow_apply<8>, dim3(grid), dim3(kFlowWg), 0, st, mine_sw, mat_sw, a, launches & 1u);
    else if (logr == 9) hipLaunchKernelGGL(k_flow_apply<9>, dim3(grid), dim3(kFlowWg), 0, st, mine_sw, mat_sw, a, launches & 1u);
    else hipLaunchKernelGGL(k_flow_apply<10>, dim3(grid), dim3(kFlowWg), 0, st, mine_sw, mat_sw, a, launches & 1u);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_flow_chunks, dim3(nchunks), dim3(1024), 0, st, mine_sw, chunks, a, logr);
    return hipGetLastError();
}

}  // namespace rtd
