// detach_check.hpp — the host half of rt_detach_voxels that needs no context: the verdict on the call's plain arguments and on its
// RtVoxelDetach parameters, and the plan — the clipped box, the chunks it meets, the stamp's extent and the size of the device
// scratch.  Plain C++ with no HIP include, so that tests/detach_voxels_main.cpp runs this very code on the CPU.  The box's validity
// and clipping are rt_edit_shapes' (edit_shapes.hpp) and the chunk list is the deposits' (deposit_check.hpp): nothing of them is
// restated here.
#pragma once

#include <cstdint>

#include "../../../include/rt_abi.h"
#include "deposit_check.hpp"

namespace rta __attribute__((visibility("hidden"))) {

constexpr uint32_t kDetachMaxPasses = 256;     // RtVoxelDetach.max_passes
constexpr int32_t kDetachMaxExtent = 256;      // of the clipped box, per axis: the stamps' limit
constexpr uint32_t kDetachFlags = RT_DETACH_CARVE | RT_DETACH_CAPTURE | RT_DETACH_ANCHOR_MATERIAL;
constexpr size_t kDetachChunkWords = 64u * 64u * 2u;   // one bit per texel of a chunk: 32 KiB
constexpr size_t kDetachHeadWords = 288u;      // pass record (a word per pass and one more), spare RtDetachResult, padding

// The detach box as the deposits' parameters (box only), whose shape, clipping and chunk list this call shares.
inline RtParticleDeposit detach_box(const RtVoxelDetach& p) {
    RtParticleDeposit d{};
    for (int k = 0; k < 3; k++) { d.lo[k] = p.lo[k]; d.hi[k] = p.hi[k]; }
    return d;
}

// What is wrong with the arguments that are tested before the context is looked at, or nullptr.
inline const char* detach_args_error(const RtVoxelDetach* params, const uint32_t* stamp_out) {
    if (!params) return "null params";
    if ((params->flags & ~kDetachFlags) != 0u) return "unknown flag bit";
    if ((params->flags & RT_DETACH_CAPTURE) != 0u && !stamp_out) return "RT_DETACH_CAPTURE needs stamp_out";
    return nullptr;
}

// The clipped box of valid parameters with the deposits' chunk list (deposit_fill_chunks serves both) and the stamp's extent.
struct DetachPlan : DepositPlan {
    int32_t ext[3] = {0, 0, 0};   // of the clipped box = of the stamp
};

inline DetachPlan detach_plan(const RtVoxelDetach& p, int logr) {
    DetachPlan s;
    static_cast<DepositPlan&>(s) = deposit_plan(detach_box(p), logr);
    if (s.empty) return s;
    for (int k = 0; k < 3; k++) s.ext[k] = s.box.hi[k] - s.box.lo[k] + 1;
    return s;
}

// What is wrong with the parameters for a region of edge 2^logr, or nullptr.
inline const char* detach_params_error(const RtVoxelDetach& p, int logr) {
    if (!shape_valid(deposit_shape(detach_box(p)), (int32_t)1 << logr)) return "the box must have lo <= hi and coordinates within [-4R, 4R]";
    if (p.max_passes < 1u || p.max_passes > kDetachMaxPasses) return "max_passes must be 1..256";
    if (p.anchor_faces > 63u) return "anchor_faces has a bit above 5";
    if ((p.anchor_value & ~p.anchor_mask) != 0u) return "anchor_value has a bit outside anchor_mask";
    if ((p.flags & RT_DETACH_ANCHOR_MATERIAL) == 0u && (p.anchor_mask != 0u || p.anchor_value != 0u))
        return "anchor_mask and anchor_value must be 0 without RT_DETACH_ANCHOR_MATERIAL";
    if (p.reserved0[0] != 0u || p.reserved0[1] != 0u || p.reserved0[2] != 0u) return "a reserved byte is not 0";
    const DetachPlan s = detach_plan(p, logr);
    for (int k = 0; k < 3 && !s.empty; k++)
        if (s.ext[k] > kDetachMaxExtent) return "an extent of the clipped box is above 256";
    return nullptr;
}

// Words of the device scratch: the head (pass record, spare result), a flag per chunk of the box (to a multiple of four words), then
// three bit arrays of 32 KiB per chunk — the occupancy and the two reach buffers (rtd::detach_scratch_words).
inline size_t detach_scratch_need(const DetachPlan& s) {
    return kDetachHeadWords + (((size_t)s.nchunks + 3u) & ~(size_t)3u) + 3u * kDetachChunkWords * (size_t)s.nchunks;
}

}  // namespace rta
