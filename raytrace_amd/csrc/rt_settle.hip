// rt_settle.hip — gfx950 kernels of rt_settle_voxels / rt_settle_voxels_async: the loose voxels of a box of texels fall along an axis
// (include/rt_abi.h "Voxel settling"; the rules are restated in tests/settle_voxels_ref.py).
//
//   k_settle_columns : one lane per column of the clipped box.  The lane walks its column upwards (h = 0 is the cell the voxels fall
//             towards) and keeps E, the number of unoccupied cells since the last fixed cell; a loose voxel drops by min(max_fall, E).
//             It writes in place: a target lies below the cell being read and belongs to the same lane, so no two lanes share a byte
//             and no cell is read after it was written.  A moved voxel's target gets minefield byte 0 and the voxel's word, its source a
//             non-zero byte (the chunk pass gives the final value) and air_material; a later voxel of the column may fill the source
//             again, in program order.  Addresses do not depend on loaded values: kBatch cells' bytes are loaded before the first is
//             used, then the material words the batch needs — of the occupied cells when the mask selects, else of the voxels that
//             move.  A lane that moves a voxel stores 0 to the flag words of the source's and the target's chunk (every writer stores
//             the same value).  moved / falling / distance are summed per wave and added with one atomic per wave and counter.
//             A wave's lanes lie 16 x 4 over the two axes across the fall axis, lane = 4 x 4 columns of each of four bricks: for axis =
//             2 a step's four loads cover four x-adjacent 64-byte bricks whole (256 contiguous bytes).
//   k_settle_chunks  : one workgroup per chunk of the box.  A workgroup whose flag word was never written returns before the first
//             barrier; the others add 1 to `chunks` and run the chunk rebuild (rt_rebuild_chunk.hpp) with a stage that does nothing.
//   (k_rebuild_chunk_maps, rt_edit.hip, follows over the same chunk list.)
//
// The flags are a block that the host fills with 0xFF bytes in front of the column pass.
#include <hip/hip_runtime.h>

#include "rt_kernels.hpp"
#include "rt_rebuild_chunk.hpp"

namespace rtd {

namespace {

constexpr uint32_t kColumnsWg = 256;   // four waves: 16 x 16 columns
constexpr int kBatch = 8;              // cells whose loads are in flight together, as DepositStage's rows

// (selects: an index that is not a constant would copy the kernel's arguments to scratch)
__device__ __forceinline__ int pick3(const int32_t v[3], int k) { return k == 0 ? v[0] : k == 1 ? v[1] : v[2]; }

// what coordinate v on axis k contributes to swizzled_index (rt_device.hpp): the index is the OR of the three axes' parts
template <int LB>
__device__ __forceinline__ uint32_t swizzled_part(int v, int k) {
    return ((uint32_t)(v >> 2) << (k * LB + 6)) | ((uint32_t)(v & 3) << (2 * k));
}

template <int LOGR, bool MASKED>
__global__ __launch_bounds__(kColumnsWg) void k_settle_columns(uint8_t* mine_sw, uint32_t* mat_sw, SettleArgs a) {
    constexpr int LB = LOGR - 2;
    const int axis = (int)a.axis, pa = axis == 0 ? 1 : 0, qa = axis == 2 ? 1 : 2;   // the column's own two axes, lower first
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lo_p = pick3(a.lo, pa), hi_p = pick3(a.hi, pa), lo_q = pick3(a.lo, qa), hi_q = pick3(a.hi, qa);
    const int lo_a = pick3(a.lo, axis), hi_a = pick3(a.hi, axis);
    // the workgroup's 16 x 16 columns are aligned to 16, so that a wave's 16 x 4 are four whole bricks' columns
    const int p = ((lo_p >> 4) + (int)blockIdx.x) * 16 + 4 * (lane >> 4) + (lane & 3);
    const int q = ((lo_q >> 4) + (int)blockIdx.y) * 16 + 4 * wave + ((lane >> 2) & 3);
    const bool active = p >= lo_p && p <= hi_p && q >= lo_q && q <= hi_q;

    uint32_t moved = 0, falling = 0, distance = 0;
    if (active) {
        const uint32_t base = swizzled_part<LB>(p, pa) | swizzled_part<LB>(q, qa);
        const int H = hi_a - lo_a + 1, start = a.toward ? hi_a : lo_a, dir = a.toward ? -1 : 1;
        // the flag word of the chunk at chunk coordinate c along the fall axis: flags are z-major over the box's chunks
        const int ncx = (a.hi[0] >> 6) - (a.lo[0] >> 6) + 1, ncy = (a.hi[1] >> 6) - (a.lo[1] >> 6) + 1;
        const int stride_p = pa == 0 ? 1 : ncx, stride_q = qa == 1 ? ncx : ncx * ncy, stride_a = axis == 0 ? 1 : axis == 1 ? ncx : ncx * ncy;
        const int flag_base = ((p >> 6) - (lo_p >> 6)) * stride_p + ((q >> 6) - (lo_q >> 6)) * stride_q - (lo_a >> 6) * stride_a;
        int flagged_a = -1, flagged_b = -1;   // the chunk coordinates this lane stored a flag for last

        uint32_t gap = 0;   // E: unoccupied cells since the last fixed cell
        for (int h0 = 0; h0 < H; h0 += kBatch) {
            uint32_t idx[kBatch], m[kBatch], w[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; u++) {   // (a cell past the column's top reads as unoccupied: it only counts into a gap nobody uses)
                idx[u] = base | swizzled_part<LB>(start + dir * (h0 + u), axis);
                m[u] = h0 + u < H ? (uint32_t)mine_sw[idx[u]] : 0xFFu;
            }
            if (MASKED) {
#pragma unroll
                for (int u = 0; u < kBatch; u++) w[u] = m[u] == 0u ? mat_sw[idx[u]] : 0u;
            } else {   // every occupied cell is loose: it moves iff a cell below it is free
                uint32_t g = gap;
#pragma unroll
                for (int u = 0; u < kBatch; u++) {
                    w[u] = (m[u] == 0u && g != 0u) ? mat_sw[idx[u]] : 0u;
                    g += m[u] != 0u ? 1u : 0u;
                }
            }
#pragma unroll
            for (int u = 0; u < kBatch; u++) {
                if (m[u] != 0u) { gap++; continue; }
                if (MASKED && (w[u] & a.loose_mask) != a.loose_value) { gap = 0u; continue; }   // fixed
                const uint32_t drop = gap < a.max_fall ? gap : a.max_fall;
                falling += gap > drop ? 1u : 0u;
                if (drop == 0u) continue;
                moved++;
                distance += drop;
                const int vs = start + dir * (h0 + u), vt = vs - dir * (int)drop;
                const uint32_t it = base | swizzled_part<LB>(vt, axis);
                mine_sw[it] = 0u;
                mat_sw[it] = w[u];
                mine_sw[idx[u]] = 1u;
                mat_sw[idx[u]] = a.air_material;
                const int cs = vs >> 6, ct = vt >> 6;
                if (cs != flagged_a) { a.flags[flag_base + cs * stride_a] = 0u; flagged_a = cs; }
                if (ct != flagged_a && ct != flagged_b) { a.flags[flag_base + ct * stride_a] = 0u; flagged_b = ct; }
            }
        }
    }
    // sums per wave, one atomic per wave and counter
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        moved += __shfl_xor(moved, off);
        falling += __shfl_xor(falling, off);
        distance += __shfl_xor(distance, off);
    }
    if (lane == 0) {
        if (moved) atomicAdd(a.counts + 0, moved);
        if (falling) atomicAdd(a.counts + 1, falling);
        if (distance) atomicAdd(a.counts + 2, distance);
    }
}

// the chunk rebuild's edit stage of a call whose edits the column pass has already written
struct NoStage {
    __device__ __forceinline__ void operator()(uint32_t*, uint32_t, uint32_t, uint32_t, int, int) const {}
};

// One workgroup per chunk of the box, in the order of the chunk list (ascending ids = z-major over the box's chunks, as the column
// pass numbers the flags).  The flag word is read by every thread (one address: a uniform value), so the exit is the workgroup's.
__global__ __launch_bounds__(1024) void k_settle_chunks(uint8_t* __restrict__ mine_sw, const uint32_t* __restrict__ chunks, SettleArgs a, int logr) {
    if (a.flags[blockIdx.x] != 0u) return;   // no voxel left or reached this chunk: its bytes stay as they are
    if (threadIdx.x == 0) atomicAdd(a.counts + 3, 1u);
    rebuild_chunk(mine_sw, chunks, logr, NoStage{});
}

template <int LOGR>
void launch_columns(dim3 grid, uint8_t* mine_sw, uint32_t* mat_sw, const SettleArgs& a, hipStream_t st) {
    if (a.loose_mask != 0u) hipLaunchKernelGGL((k_settle_columns<LOGR, true>), grid, dim3(kColumnsWg), 0, st, mine_sw, mat_sw, a);
    else hipLaunchKernelGGL((k_settle_columns<LOGR, false>), grid, dim3(kColumnsWg), 0, st, mine_sw, mat_sw, a);
}

}  // namespace

hipError_t launch_settle_voxels(uint8_t* mine_sw, uint32_t* mat_sw, const uint32_t* chunks, uint32_t nchunks, int logr, const SettleArgs& a,
                                hipStream_t st) {
    if (logr < 8 || logr > 10 || nchunks < 1u || a.axis > 2u || a.toward > 1u || a.max_fall < 1u || (a.loose_value & ~a.loose_mask) != 0u)
        return hipErrorInvalidValue;
    uint64_t boxchunks = 1;
    for (int k = 0; k < 3; k++) {
        if (a.lo[k] < 0 || a.hi[k] >= (1 << logr) || a.lo[k] > a.hi[k]) return hipErrorInvalidValue;
        boxchunks *= (uint64_t)((a.hi[k] >> 6) - (a.lo[k] >> 6) + 1);
    }
    if (boxchunks != nchunks) return hipErrorInvalidValue;
    const int pa = a.axis == 0u ? 1 : 0, qa = a.axis == 2u ? 1 : 2;
    const dim3 grid((uint32_t)((a.hi[pa] >> 4) - (a.lo[pa] >> 4) + 1), (uint32_t)((a.hi[qa] >> 4) - (a.lo[qa] >> 4) + 1));
    if (logr == 8) launch_columns<8>(grid, mine_sw, mat_sw, a, st);
    else if (logr == 9) launch_columns<9>(grid, mine_sw, mat_sw, a, st);
    else launch_columns<10>(grid, mine_sw, mat_sw, a, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_settle_chunks, dim3(nchunks), dim3(1024), 0, st, mine_sw, chunks, a, logr);
    return hipGetLastError();
}

}  // namespace rtd
