// rt_shape_rows.hpp — membership of RtShapeEdit's shapes on the device, a row of 64 texels at a time: the one definition that
// rt_edit_shapes' edit stage (rt_edit.hip, ShapeStage) and rt_emit_particles' kernels (rt_emit.hip) share.  Integer arithmetic
// only (include/rt_abi.h, RtShapeEdit: Membership).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rtd {

// bits lo..hi of a 64-voxel row, clipped to it (none when the range misses the row)
__device__ __forceinline__ uint64_t row_range(int lo, int hi) {
    const int l = lo < 0 ? 0 : lo > 63 ? 63 : lo, h = hi < 0 ? 0 : hi > 63 ? 63 : hi;
    return (lo > hi || hi < 0 || lo > 63) ? 0ull : (~0ull >> (63 - h)) & (~0ull << l);
}
// floor(sqrt(v)) for 0 <= v <= 2^26, bit by bit (the host's rule, api/edit_shapes.hpp)
__device__ __forceinline__ int isqrt26(int v) {
    int s = 0;
#pragma unroll
    for (int bit = 1 << 13; bit; bit >>= 1) {
        const int t = s | bit;
        s = t * t <= v ? t : s;
    }
    return s;
}

// The members of a shape among the 64 texels x0 .. x0 + 63 of row (y, z): bit i = texel x0 + i.  p = (a, -), q = (b, -) of the
// shape's record; kind 0 is the box, anything else the sphere.
__device__ __forceinline__ uint64_t shape_row(uint32_t kind, const int4& p, const int4& q, int x0, int y, int z) {
    if (kind == 0u) return (y >= p.y && y <= q.y && z >= p.z && z <= q.z) ? row_range(p.x - x0, q.x - x0) : 0ull;
    // what is left of (2 r)^2 for x: every term is below 2^26, so int32 is exact
    const int dy = 2 * y + 1 - p.y, dz = 2 * z + 1 - p.z;
    const int budget = q.x - dy * dy - dz * dz;
    const int r = isqrt26(budget < 0 ? 0 : budget);
    // a - r <= 2 x + 1 <= a + r: x from ceil((a - r - 1) / 2) to floor((a + r - 1) / 2)
    return budget < 0 ? 0ull : row_range(((p.x - r) >> 1) - x0, ((p.x + r - 1) >> 1) - x0);
}

}  // namespace rtd
