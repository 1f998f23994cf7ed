// flow_check.hpp — the host half of rt_flow_voxels that needs no context: the verdict on the call's plain arguments and on its
// RtVoxelFlow parameters, and the plan — the clipped box, the chunks it meets, the tiles of a tick launch, the launches for a number
// of ticks per launch and the size of the device scratch.  Plain C++ with no HIP include, so that tests/flow_voxels_main.cpp runs this
// very code on the CPU.  The box's validity and clipping are rt_edit_shapes' (edit_shapes.hpp) and the chunk list is the deposits'
// (deposit_check.hpp): nothing of them is restated here.
#pragma once

#include <cstdint>

#include "../../../include/rt_abi.h"
#include "deposit_check.hpp"

namespace rta __attribute__((visibility("hidden"))) {

constexpr uint32_t kFlowMaxTicks = 256;      // RtVoxelFlow.ticks
constexpr uint32_t kFlowMaxLevel = 13;       // RtVoxelFlow.max_level: the states fit a nibble (empty, 1..13, source, fixed)
constexpr uint32_t kFlowMaxShift = 28;       // RtVoxelFlow.level_shift
constexpr int32_t kFlowMaxExtent = 256;      // of the clipped box, per axis: the bound of the per-texel scratch
constexpr uint32_t kFlowGroup = 4;           // G: ticks per launch (RT_FLOW_TICKS chooses 1, 2, 4 or 8)
constexpr int32_t kFlowTile[3] = {32, 16, 16};   // cells of a tile's interior
constexpr size_t kFlowHeadWords = 512u;      // a word per tick launch, a spare RtFlowCount, a flag per chunk of the box

// The flow box as the deposits' parameters (box only), whose shape, clipping and chunk list this call shares.
inline RtParticleDeposit flow_box(const RtVoxelFlow& p) {
    RtParticleDeposit d{};
    for (int k = 0; k < 3; k++) { d.lo[k] = p.lo[k]; d.hi[k] = p.hi[k]; }
    return d;
}

// What is wrong with the arguments that are tested before the context is looked at, or nullptr.
inline const char* flow_args_error(const void* params) { return params ? nullptr : "null params"; }

// The clipped box of valid parameters with the deposits' chunk list (deposit_fill_chunks serves both), its extent, the tiles of a tick
// launch and the cells of a state array (rows padded to four cells).
struct FlowPlan : DepositPlan {
    int32_t ext[3] = {0, 0, 0};        // of the clipped box
    uint32_t tiles[3] = {0, 0, 0};     // per axis
    uint32_t ntiles = 0;               // workgroups of a tick launch
    uint64_t cells = 0;                // bytes of one state array
};

inline FlowPlan flow_plan(const RtVoxelFlow& p, int logr) {
    FlowPlan s;
    static_cast<DepositPlan&>(s) = deposit_plan(flow_box(p), logr);
    if (s.empty) return s;
    s.ntiles = 1;
    for (int k = 0; k < 3; k++) {
        s.ext[k] = s.box.hi[k] - s.box.lo[k] + 1;
        s.tiles[k] = (uint32_t)(s.ext[k] + kFlowTile[k] - 1) / (uint32_t)kFlowTile[k];
        s.ntiles *= s.tiles[k];
    }
    s.cells = (uint64_t)(((uint32_t)s.ext[0] + 3u) & ~3u) * (uint64_t)s.ext[1] * (uint64_t)s.ext[2];
    return s;
}

// Tick launches of a call of `ticks` ticks at `group` ticks per launch.
inline uint32_t flow_launches(uint32_t ticks, uint32_t group) { return (ticks + group - 1u) / group; }

// What is wrong with the parameters for a region of edge 2^logr, or nullptr.
inline const char* flow_params_error(const RtVoxelFlow& p, int logr) {
    if (!shape_valid(deposit_shape(flow_box(p)), (int32_t)1 << logr)) return "the box must have lo <= hi and coordinates within [-4R, 4R]";
    if (p.ticks < 1u || p.ticks > kFlowMaxTicks) return "ticks must be 1..256";
    if (p.level_shift > kFlowMaxShift) return "level_shift must be 0..28";
    if (p.max_level < 1u || p.max_level > kFlowMaxLevel) return "max_level must be 1..13";
    if (p.fluid_mask == 0u) return "fluid_mask must not be 0";
    const uint32_t field = 0xFu << p.level_shift;
    if ((p.fluid_mask & field) != 0u) return "fluid_mask overlaps the level field";
    if ((p.fluid_value & ~p.fluid_mask) != 0u) return "fluid_value has a bit outside fluid_mask";
    if ((p.fluid_word & field) != 0u) return "fluid_word has a bit in the level field";
    if ((p.fluid_word & p.fluid_mask) != p.fluid_value) return "fluid_word does not pass the fluid test";
    if (p.reserved0 != 0u || p.reserved1[0] != 0u || p.reserved1[1] != 0u || p.reserved2[0] != 0u || p.reserved2[1] != 0u || p.reserved2[2] != 0u)
        return "a reserved byte or word is not 0";
    const FlowPlan s = flow_plan(p, logr);
    for (int k = 0; k < 3 && !s.empty; k++)
        if (s.ext[k] > kFlowMaxExtent) return "an extent of the clipped box is above 256";
    return nullptr;
}

// Words of the device scratch: the head, then the two state arrays (rtd::flow_scratch_words).
inline size_t flow_scratch_need(const FlowPlan& s) { return kFlowHeadWords + 2u * (size_t)(s.cells / 4u); }

}  // namespace rta
