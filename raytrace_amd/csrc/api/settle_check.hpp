// settle_check.hpp — the host half of rt_settle_voxels that needs no context: the verdict on the call's plain arguments and on its
// RtVoxelSettle parameters, and the plan — the clipped box, its columns and their height along the fall axis, the chunks it meets
// and the size of the device scratch.  Plain C++ with no HIP include, so that tests/settle_voxels_main.cpp runs this very code on the
// CPU.  The box's validity and clipping are rt_edit_shapes' (edit_shapes.hpp) and the chunk list is the deposits'
// (deposit_check.hpp): nothing of them is restated here.
#pragma once

#include <cstdint>

#include "../../../include/rt_abi.h"
#include "deposit_check.hpp"

namespace rta __attribute__((visibility("hidden"))) {

constexpr uint32_t kSettleUnlimited = 0xFFFFFFFFu;   // RtVoxelSettle.max_fall: until the voxel rests

// The settle box as the deposits' parameters (box only), whose shape, clipping and chunk list this call shares.
inline RtParticleDeposit settle_box(const RtVoxelSettle& p) {
    RtParticleDeposit d{};
    for (int k = 0; k < 3; k++) { d.lo[k] = p.lo[k]; d.hi[k] = p.hi[k]; }
    return d;
}

// What is wrong with the arguments that are tested before the context is looked at, or nullptr.
inline const char* settle_args_error(const void* params) { return params ? nullptr : "null params"; }

// What is wrong with the parameters for a region of edge 2^logr, or nullptr.
inline const char* settle_params_error(const RtVoxelSettle& p, int logr) {
    if (!shape_valid(deposit_shape(settle_box(p)), (int32_t)1 << logr)) return "the box must have lo <= hi and coordinates within [-4R, 4R]";
    if (p.axis > 2u) return "axis must be 0, 1 or 2";
    if (p.toward > 1u) return "toward must be 0 or 1";
    if (p.max_fall == 0u) return "max_fall must be at least 1";
    if ((p.loose_value & ~p.loose_mask) != 0u) return "loose_value has a bit outside loose_mask";
    if (p.reserved0[0] != 0u || p.reserved0[1] != 0u || p.reserved1 != 0u) return "a reserved byte or word is not 0";
    return nullptr;
}

// The clipped box of valid parameters with the deposits' chunk list (deposit_fill_chunks serves both), the columns a lane each walks
// and their height.
struct SettlePlan : DepositPlan {
    uint64_t columns = 0;   // cells of the clipped box's face across `axis`
    uint32_t height = 0;    // H: cells of a column
};

inline SettlePlan settle_plan(const RtVoxelSettle& p, int logr) {
    SettlePlan s;
    static_cast<DepositPlan&>(s) = deposit_plan(settle_box(p), logr);
    if (s.empty) return s;
    s.height = (uint32_t)(s.box.hi[p.axis] - s.box.lo[p.axis] + 1);
    s.columns = s.texels / s.height;
    return s;
}

// Words of the device scratch: a flag per chunk of the box and a spare RtSettleCount (rtd::settle_scratch_words).
inline size_t settle_scratch_need(const SettlePlan& s) { return (size_t)s.nchunks + 4u; }

}  // namespace rta
