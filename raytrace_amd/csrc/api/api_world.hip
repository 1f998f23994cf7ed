// api_world.hip — the kinds of world change and their staging: whole-region upload, streamed slabs, sparse voxel edits, shape
// edits, voxel stamps (their store, capture and placement), particle deposits, voxel settling, voxel detachment, fluid flow and terrain generated on the device; rt_read_box reads
// the resident region back.  The ordering protocols stand here once each: world_change_begin / world_change_end round every change,
// world_send / world_applied for the changes that come through a staging set (rt_context.hpp's staging_claim and staging_send, plus
// the world change), and chunk_edit with its history rule (edit_history) for the four calls that rewrite whole chunks from a staged
// list of chunk ids: rt_edit_voxels, rt_edit_shapes, rt_edit_stamps, the deposits, the settling, a carving detachment and the fluid
// flow hand it only what differs between them.
#include "deposit_check.hpp"
#include "detach_check.hpp"
#include "flow_check.hpp"
#include "rt_context.hpp"
#include "settle_check.hpp"

using namespace rta;

namespace {

// ---- a change of the resident world on the render stream (slabs, edits, generated terrain) ---------------------------------------
// before its launches: they wait for the frames in flight on every lane and for the queries recorded so far (both read the region)
hipError_t world_change_begin(RtContext* c) {
    hipError_t e = join_lanes_into(c, c->stream);
    if (e == hipSuccess) e = c->ev_query.wait(c->stream);
    return e;
}
// after them: later queries (ev_world) and later frames, whichever lane they start on, see what changed
hipError_t world_change_end(RtContext* c) {
    hipError_t e = c->ev_world.record(c->stream);
    return e == hipSuccess ? fence_lanes_after(c, c->stream) : e;
}

// ---- a world change through a staging set: rt_context.hpp's staging_claim and staging_send, and the world change round the launch ---
// the render stream waits for the transfer, and for the frames in flight on the other lane (they read what the launch changes)
hipError_t world_send(RtContext* c, StagingSet& s, size_t bytes) {
    const hipError_t e = staging_send(c, s, bytes, c->stream);
    return e == hipSuccess ? world_change_begin(c) : e;
}
// after the launch that read the device block: later frames, whichever lane they start on, see what it changed
hipError_t world_applied(RtContext* c, StagingSet& s) {
    const hipError_t e = s.ev_applied.record(c->stream);
    return e == hipSuccess ? world_change_end(c) : e;
}

// ---- chunk edits: rt_edit_voxels, rt_edit_shapes, rt_edit_stamps and the particle deposits ----------------------------------------
// The history rule of an edit that brings `nboxes` pending boxes.  RtConfig.edit_radius == 0: the history restarts.  Otherwise it
// stays and the boxes (`write(dst)` writes them and returns how many) wait for the next frame drawn, which restarts only the pixels
// an edit can have changed (api_frame.hip); a set that would pass its capacity is emptied and that frame restarts.
template <typename Write>
void edit_history(RtContext* c, uint32_t nboxes, Write&& write) {
    if (c->edit_radius == 0u) { c->accum_valid = false; return; }
    if (c->edit_overflow) return;
    if (c->edit_nbox + nboxes > rtd::kTemporalMaxBoxes) {
        c->edit_nbox = 0;
        c->edit_overflow = true;
    } else {
        c->edit_nbox += write(c->edit_boxes + c->edit_nbox);
    }
}

// One edit of `nchunks` chunks, whose ids head the staged block.  The four kinds share the two edit sets and one counter, so that
// they apply in call order: the transfer on the upload stream, then the launches on the render stream after the frames already
// submitted (every lane), and later frames after them — the ordering of rt_upload_slice.  `fill(host)` writes the block (at most `need`
// bytes; a set that must grow gets `alloc`) and returns the bytes to send; `apply(dev)` enqueues, and times, what rewrites the chunks'
// voxels; the rebuild of their nibble maps follows, then `users` (a scratch block's event, or null) is recorded.
template <typename Fill, typename Write, typename Apply>
int chunk_edit(RtContext* c, size_t need, size_t alloc, uint32_t nchunks, uint32_t nboxes, Fill&& fill, Write&& write, Apply&& apply,
               LatchEvent* users = nullptr) {
    StagingSet& s = c->edit_sets[c->edit_batches & 1u];
    RT_HIP(c, staging_claim(c, s, need, alloc));
    const size_t bytes = fill(s.host);
    c->edit_batches++;
    edit_history(c, nboxes, write);
    invalidate_prepass(c);
    RT_HIP(c, world_send(c, s, bytes));
    const int rc = apply(s.dev);
    if (rc != RT_OK) return rc;
    {
        LaunchTimer lt(c, 1);
        RT_HIP(c, rtd::launch_rebuild_chunk_maps(c->d_mine_sw, c->d_coarse, c->d_brick, reinterpret_cast<const uint32_t*>(s.dev), nchunks, c->logr, c->stream));
    }
    if (users) RT_HIP(c, users->record(c->stream));
    RT_HIP(c, world_applied(c, s));
    return RT_OK;
}

// ---- RtConfig.stream_history: a slab that keeps the lighting history ------------------------------------------------------------
// An accepted slab takes the next pending slot, or — a fifth — empties the set and marks it overflowed; returns the slot's masks
// (old set, then new), or null where nothing is to be scanned.  Called once nothing can reject the slab any more.
uint32_t* slab_take_slot(RtContext* c) {
    if (!c->stream_history) { restart_history(c); return nullptr; }
    if (c->slab_overflow) return nullptr;
    if (c->slab_pending == rtd::kSlabSlots) { c->slab_pending = 0; c->slab_overflow = true; return nullptr; }
    return c->d_slab_masks + (size_t)rtd::kSlabSlotWords * c->slab_pending++;
}
// inside world_change_begin / world_change_end, in front of the launch that writes the slab: the slot is cleared, then what the
// slab holds now is scanned into its old set
hipError_t slab_scan_old(RtContext* c, uint32_t* masks, int axis, int offset) {
    if (!masks) return hipSuccess;
    hipError_t e = hipMemsetAsync(masks, 0, rtd::kSlabSlotWords * sizeof(uint32_t), c->stream);
    LaunchTimer t(c, 1);
    return e == hipSuccess ? rtd::launch_slab_occupancy(c->d_mine_sw, c->logr, axis, offset, masks, c->stream) : e;
}
// ... and behind it: what arrived, into the new set
hipError_t slab_scan_new(RtContext* c, uint32_t* masks, int axis, int offset) {
    if (!masks) return hipSuccess;
    LaunchTimer t(c, 1);
    return rtd::launch_slab_occupancy(c->d_mine_sw, c->logr, axis, offset, masks + rtd::kSlabSetWords, c->stream);
}

int reflatten(RtContext* c, const uint8_t* d_mine_lin, const uint32_t* d_mat_lin) {
    RT_HIP(c, hipMemsetAsync(c->d_flag, 0, sizeof(uint32_t), c->stream));
    RT_HIP(c, rtd::launch_flatten(d_mine_lin, d_mat_lin, c->d_mine_sw, c->d_mat_sw, c->d_coarse, c->d_brick, c->d_flag, c->logr, c->stream));
    uint32_t flag = 0;
    RT_HIP(c, hipMemcpyAsync(&flag, c->d_flag, sizeof(flag), hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    if (flag) return fail(c, RT_ERR_INVALID_ARG, "minefield holds a value above 30 (the reference writes 0..6, src/world/chunk.rs:163-183)");
    return RT_OK;
}

// ---- terrain on the device (rt_generate_world, rt_generate_slice) -------------------------------------------------------------
// The window [lo, lo + ext) on every axis: 16-aligned, every voxel (and so lr = lo + R/2) inside int32.
bool terrain_window_ok(const int64_t lo[3], const int64_t ext[3]) {
    for (int a = 0; a < 3; a++)
        if (lo[a] % RT_SLICE_SIZE != 0 || lo[a] < (int64_t)INT32_MIN || lo[a] + ext[a] - 1 > (int64_t)INT32_MAX) return false;
    return true;
}
// Generates the window on the render stream after every frame already submitted (every lane) and every earlier query; later frames,
// lanes and queries see the result (the ordering of rt_upload_slice, without staging: the kernels read nothing from the host).
int generate_terrain(RtContext* c, uint64_t seed, const int64_t lo[3], int axis) {
    RT_HIP(c, hipSetDevice(c->device));
    if (!c->d_heights) {
        const size_t cols = (size_t)(c->region + RT_CHUNK_SIZE) * (size_t)(c->region + RT_CHUNK_SIZE);
        RT_HIP(c, dev_alloc(c, &c->d_heights, cols));
    }
    // (a whole region restarts the history; a slab does unless the context keeps it: RtConfig.stream_history)
    uint32_t* masks = nullptr;
    if (axis < 0) restart_history(c); else masks = slab_take_slot(c);
    const int offset = axis < 0 ? 0 : (int)((lo[axis] + c->region / 2) & (int64_t)(c->region - 1));
    invalidate_prepass(c);
    RT_HIP(c, world_change_begin(c));
    RT_HIP(c, slab_scan_old(c, masks, axis, offset));
    {
        LaunchTimer t(c, 1);
        RT_HIP(c, rtd::launch_terrain(c->d_mine_sw, c->d_mat_sw, c->d_coarse, c->d_brick, c->d_heights, c->logr, seed, lo, axis, c->stream));
    }
    RT_HIP(c, slab_scan_new(c, masks, axis, offset));
    RT_HIP(c, world_change_end(c));
    return RT_OK;
}

// ---- voxel stamps (rt_stamp_*): device arrays of their own, counted in device_bytes while the stamp lives -----------------------
// the arrays of a new entry; on failure nothing stays allocated and the entry is removed
hipError_t stamp_alloc(RtContext* c, StampEntry* e) {
    void *m = nullptr, *s = nullptr;
    hipError_t err = hipMalloc(&m, e->voxels() * sizeof(uint32_t));
    if (err == hipSuccess) err = hipMalloc(&s, e->voxels());
    if (err != hipSuccess) {
        if (m) (void)hipFree(m);
        c->stamps.remove(e);
        return err;
    }
    e->mats = reinterpret_cast<uint64_t>(m);
    e->state = reinterpret_cast<uint64_t>(s);
    c->device_bytes += e->voxels() * 5u;
    return hipSuccess;
}
void stamp_free(RtContext* c, StampEntry* e) {
    c->device_bytes -= e->voxels() * 5u;
    (void)hipFree(reinterpret_cast<void*>(e->mats));
    (void)hipFree(reinterpret_cast<void*>(e->state));
    c->stamps.remove(e);
}

// ---- particle deposits (rt_deposit_particles[_async]): a world change whose targets only the device knows -----------------------
static_assert(sizeof(RtParticleDeposit) == 48 && sizeof(RtDepositCount) == 16, "the layout the header states");
static_assert(kMaxDepositParticles == rtd::kMaxParticles && kMaxDepositBoxTexels == rtd::kMaxDepositTexels, "the host's limits are the kernels'");

// checks shared by the two calls, and the plan; RT_OK when there is work to enqueue, 1 for a call that enqueues nothing
int deposit_check(RtContext* c, const char* fn, const RtParticleDeposit* p, const void* states, const void* draw, uint32_t count, const void* counts,
                  DepositPlan* plan) {
    const char* e = deposit_args_error(p, states, draw, count, counts);
    if (!e) e = deposit_params_error(*p, c->logr);
    if (e) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": " + e + "; nothing was applied");
    *plan = deposit_plan(*p, c->logr);
    if (plan->texels > kMaxDepositBoxTexels) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": the clipped box covers more than 2^24 texels; nothing was applied");
    if (!c->world_resident) return fail(c, RT_ERR_NOT_READY, std::string(fn) + ": upload the full region first");
    return count == 0u || plan->empty ? 1 : RT_OK;
}

// A chunk edit (the clipped box's chunk ids; one pending box, the clipped box) whose apply step fills the scratch and runs the chunk
// pass over it.  The pointers are device addresses the stream may use.
int deposit_run(RtContext* c, const RtParticleDeposit& p, const DepositPlan& plan, void* states_dev, void* draw_dev, void* counts_dev, uint32_t count) {
    const size_t words = deposit_scratch_need(plan);
    const int rc = deposit_scratch_reserve(c, words);
    if (rc != RT_OK) return rc;
    rtd::DepositArgs a;
    a.states = reinterpret_cast<uint4*>(states_dev);
    a.draw = reinterpret_cast<uint4*>(draw_dev);
    a.claims = c->deposit_scratch;
    a.flags = c->deposit_scratch + plan.texels;
    a.counts = counts_dev ? reinterpret_cast<uint32_t*>(counts_dev) : c->deposit_scratch + plan.texels + plan.nchunks;
    a.count = count;
    a.max_speed = p.max_speed;
    for (int k = 0; k < 3; k++) { a.lr[k] = p.lr[k]; a.lo[k] = plan.box.lo[k]; a.hi[k] = plan.box.hi[k]; }
    return chunk_edit(
        c, plan.need, staging_alloc(plan.need), plan.nchunks, 1u,
        [&](uint8_t* host) { deposit_fill_chunks(plan, c->logr, reinterpret_cast<uint32_t*>(host)); return plan.need; },
        [&](EditBox* boxes) { *boxes = plan.box; return 1u; },
        [&](const uint8_t* dev) -> int {
            RT_HIP(c, c->ev_deposit.wait_elsewhere(c->stream));   // the scratch is the previous call's until its chunk pass has run
            {
                LaunchTimer lt(c, 1);
                RT_HIP(c, hipMemsetAsync(c->deposit_scratch, 0xFF, words * sizeof(uint32_t), c->stream));
            }
            LaunchTimer lt(c, 1);
            RT_HIP(c, rtd::launch_deposit_particles(c->d_mine_sw, c->d_mat_sw, reinterpret_cast<const uint32_t*>(dev), plan.nchunks, c->logr, a, c->stream));
            return RT_OK;
        },
        &c->ev_deposit);
}

// ---- voxel settling (rt_settle_voxels[_async]): a world change whose sources and targets only the device knows --------------------
static_assert(sizeof(RtVoxelSettle) == 48 && sizeof(RtSettleCount) == 16, "the layout the header states");

// checks shared by the two calls, and the plan; RT_OK when there is work to enqueue, 1 for a call that enqueues nothing
int settle_check(RtContext* c, const char* fn, const RtVoxelSettle* p, SettlePlan* plan) {
    const char* e = settle_args_error(p);
    if (!e) e = settle_params_error(*p, c->logr);
    if (e) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": " + e + "; nothing was applied");
    if (!c->world_resident) return fail(c, RT_ERR_NOT_READY, std::string(fn) + ": upload the full region first");
    *plan = settle_plan(*p, c->logr);
    return plan->empty ? 1 : RT_OK;
}

// A chunk edit (the clipped box's chunk ids; one pending box, the clipped box) whose apply step fills the flags and runs the column and
// the chunk pass.  The scratch is the deposits' block, handled as they handle it.  counts_dev is a device address the stream may use.
int settle_run(RtContext* c, const RtVoxelSettle& p, const SettlePlan& plan, void* counts_dev) {
    const size_t words = settle_scratch_need(plan);
    const int rc = deposit_scratch_reserve(c, words);
    if (rc != RT_OK) return rc;
    rtd::SettleArgs a;
    a.flags = c->deposit_scratch;
    a.counts = counts_dev ? reinterpret_cast<uint32_t*>(counts_dev) : c->deposit_scratch + plan.nchunks;
    for (int k = 0; k < 3; k++) { a.lo[k] = plan.box.lo[k]; a.hi[k] = plan.box.hi[k]; }
    a.max_fall = p.max_fall; a.air_material = p.air_material; a.loose_mask = p.loose_mask; a.loose_value = p.loose_value;
    a.axis = p.axis; a.toward = p.toward;
    return chunk_edit(
        c, plan.need, staging_alloc(plan.need), plan.nchunks, 1u,
        [&](uint8_t* host) { deposit_fill_chunks(plan, c->logr, reinterpret_cast<uint32_t*>(host)); return plan.need; },
        [&](EditBox* boxes) { *boxes = plan.box; return 1u; },
        [&](const uint8_t* dev) -> int {
            RT_HIP(c, c->ev_deposit.wait_elsewhere(c->stream));   // the scratch is the previous call's until its chunk pass has run
            {
                LaunchTimer lt(c, 1);
                RT_HIP(c, hipMemsetAsync(c->deposit_scratch, 0xFF, words * sizeof(uint32_t), c->stream));
            }
            LaunchTimer lt(c, 1);
            RT_HIP(c, rtd::launch_settle_voxels(c->d_mine_sw, c->d_mat_sw, reinterpret_cast<const uint32_t*>(dev), plan.nchunks, c->logr, a, c->stream));
            return RT_OK;
        },
        &c->ev_deposit);
}

// ---- fluid flow (rt_flow_voxels[_async]): a world change whose cells only the device knows ------------------------------------------
static_assert(sizeof(RtVoxelFlow) == 64 && sizeof(RtFlowCount) == 32, "the layout the header states");
static_assert(kFlowMaxTicks == rtd::kFlowMaxTicks && kFlowMaxLevel == rtd::kFlowMaxLevel && kFlowMaxExtent == rtd::kFlowMaxExtent &&
                  kFlowHeadWords == rtd::kFlowHeadWords,
              "the host's limits and layout are the kernels'");

// checks shared by the two calls, and the plan; RT_OK when there is work to enqueue, 1 for a call that enqueues nothing
int flow_check(RtContext* c, const char* fn, const RtVoxelFlow* p, FlowPlan* plan) {
    const char* e = flow_args_error(p);
    if (!e) e = flow_params_error(*p, c->logr);
    if (e) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": " + e + "; nothing was applied");
    if (!c->world_resident) return fail(c, RT_ERR_NOT_READY, std::string(fn) + ": upload the full region first");
    *plan = flow_plan(*p, c->logr);
    return plan->empty ? 1 : RT_OK;
}

// A chunk edit (the clipped box's chunk ids; one pending box, the clipped box) whose apply step runs the seed, tick, apply and chunk
// launches.  The scratch is a block of its own, handled as the deposits' is.  counts_dev is a device address the stream may use.
int flow_run(RtContext* c, const RtVoxelFlow& p, const FlowPlan& plan, void* counts_dev) {
    if (!c->flow_planned) {   // RT_FLOW_TICKS: 1, 2, 4 or 8 ticks per launch (A/B timing)
        uint32_t g = 0;
        if (env_int("RT_FLOW_TICKS", 1, 8, &g) && (g & (g - 1u)) == 0u) c->flow_group = g;
        c->flow_planned = true;
    }
    const int rc = flow_scratch_reserve(c, flow_scratch_need(plan));
    if (rc != RT_OK) return rc;
    rtd::FlowArgs a;
    a.scratch = c->flow_scratch;
    a.counts = counts_dev ? reinterpret_cast<uint32_t*>(counts_dev) : c->flow_scratch + rtd::kFlowSpareCount;
    for (int k = 0; k < 3; k++) { a.lo[k] = plan.box.lo[k]; a.hi[k] = plan.box.hi[k]; }
    a.ticks = p.ticks; a.air_material = p.air_material; a.fluid_mask = p.fluid_mask; a.fluid_value = p.fluid_value; a.fluid_word = p.fluid_word;
    a.level_shift = p.level_shift; a.max_level = p.max_level;
    return chunk_edit(
        c, plan.need, staging_alloc(plan.need), plan.nchunks, 1u,
        [&](uint8_t* host) { deposit_fill_chunks(plan, c->logr, reinterpret_cast<uint32_t*>(host)); return plan.need; },
        [&](EditBox* boxes) { *boxes = plan.box; return 1u; },
        [&](const uint8_t* dev) -> int {
            RT_HIP(c, c->ev_flow.wait_elsewhere(c->stream));   // the scratch is the previous call's until its chunk pass has run
            LaunchTimer lt(c, 1);
            RT_HIP(c, rtd::launch_flow_voxels(c->d_mine_sw, c->d_mat_sw, reinterpret_cast<const uint32_t*>(dev), plan.nchunks, c->logr, a, c->flow_group,
                                              c->stream));
            return RT_OK;
        },
        &c->ev_flow);
}

// ---- voxel detachment (rt_detach_voxels[_async]): a world change (RT_DETACH_CARVE) or a query whose voxels only the device knows ---
static_assert(sizeof(RtVoxelDetach) == 48 && sizeof(RtDetachResult) == 48, "the layout the header states");
static_assert(kDetachMaxExtent == kMaxStampExtent && kDetachMaxPasses == rtd::kDetachMaxPasses && kDetachChunkWords == rtd::kDetachChunkWords &&
                  kDetachHeadWords == rtd::kDetachHeadWords,
              "the host's limits and layout are the stamps' and the kernels'");

// checks shared by the two calls, and the plan; RT_OK when there is work to enqueue, 1 for a call that enqueues nothing
int detach_check(RtContext* c, const char* fn, const RtVoxelDetach* p, const uint32_t* stamp_out, DetachPlan* plan) {
    const char* e = detach_args_error(p, stamp_out);
    if (!e) e = detach_params_error(*p, c->logr);
    if (e) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": " + e + "; nothing was applied");
    if (!c->world_resident) return fail(c, RT_ERR_NOT_READY, std::string(fn) + ": upload the full region first");
    *plan = detach_plan(*p, c->logr);
    if (plan->empty) return 1;
    if ((p->flags & RT_DETACH_CAPTURE) != 0u && c->stamps.live == kMaxStamps)
        return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": 1024 stamps are live; nothing was applied");
    return RT_OK;
}

// The launches of one call, `e` the new stamp or null.  With RT_DETACH_CARVE a chunk edit (the clipped box's chunk ids; one pending
// box, the clipped box); without it rt_stamp_capture's protocol: the launches go to the stream the edits use, behind every earlier world
// change, and read the region only; what they write — the scratch, the result, the stamp's arrays — is followed in stream order, by
// ev_capture (entity queries on the query stream) and by the fence (a later change may start on the other lane's stream).
int detach_enqueue(RtContext* c, const RtVoxelDetach& p, const DetachPlan& plan, void* result_dev, StampEntry* e) {
    rtd::DetachArgs a;
    a.scratch = c->detach_scratch;
    a.result = result_dev ? reinterpret_cast<uint32_t*>(result_dev) : c->detach_scratch + rtd::kDetachSpareResult;
    a.stamp_mats = e ? reinterpret_cast<uint32_t*>(e->mats) : nullptr;
    a.stamp_state = e ? reinterpret_cast<uint8_t*>(e->state) : nullptr;
    for (int k = 0; k < 3; k++) { a.lo[k] = plan.box.lo[k]; a.hi[k] = plan.box.hi[k]; }
    a.flags = p.flags; a.air_material = p.air_material; a.anchor_mask = p.anchor_mask; a.anchor_value = p.anchor_value;
    a.max_passes = p.max_passes; a.anchor_faces = p.anchor_faces;
    if (e && !c->ev_capture.ev) RT_HIP(c, new_event(c, &c->ev_capture.ev));
    auto launches = [&](const uint8_t* dev) -> int {
        RT_HIP(c, c->ev_detach.wait_elsewhere(c->stream));   // the scratch is the previous call's until its last launch has run
        LaunchTimer lt(c, 1);
        RT_HIP(c, rtd::launch_detach_voxels(c->d_mine_sw, c->d_mat_sw, reinterpret_cast<const uint32_t*>(dev), plan.nchunks, c->logr, a, c->stream));
        if (e) RT_HIP(c, c->ev_capture.record(c->stream));
        return RT_OK;
    };
    if ((p.flags & RT_DETACH_CARVE) != 0u)
        return chunk_edit(
            c, plan.need, staging_alloc(plan.need), plan.nchunks, 1u,
            [&](uint8_t* host) { deposit_fill_chunks(plan, c->logr, reinterpret_cast<uint32_t*>(host)); return plan.need; },
            [&](EditBox* boxes) { *boxes = plan.box; return 1u; }, launches, &c->ev_detach);
    const int rc = launches(nullptr);
    if (rc != RT_OK) return rc;
    RT_HIP(c, c->ev_detach.record(c->stream));
    RT_HIP(c, fence_lanes_after(c, c->stream));
    return RT_OK;
}

// The scratch, the stamp (created before anything is enqueued, removed again if anything after that fails) and the launches.
// result_dev is a device address the stream may use, or null.
int detach_run(RtContext* c, const RtVoxelDetach& p, const DetachPlan& plan, void* result_dev, uint32_t* stamp_out) {
    int rc = detach_scratch_reserve(c, detach_scratch_need(plan));
    if (rc != RT_OK) return rc;
    StampEntry* e = nullptr;
    if ((p.flags & RT_DETACH_CAPTURE) != 0u) {
        e = c->stamps.add(plan.ext);
        RT_HIP(c, stamp_alloc(c, e));
    }
    rc = detach_enqueue(c, p, plan, result_dev, e);
    if (rc != RT_OK) {
        if (e) {
            (void)hipStreamSynchronize(c->stream);
            stamp_free(c, e);
        }
        return rc;
    }
    if (e) e->used = true;
    if (stamp_out) *stamp_out = e ? e->id : 0u;
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_upload_world(RtContext* ctx, const uint32_t* materials, const uint8_t* minefield) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!materials || !minefield) return fail(ctx, RT_ERR_INVALID_ARG, "rt_upload_world: null pointer");
    restart_history(ctx);
    invalidate_prepass(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, sync_lanes(ctx));
    // the caller-layout copy lives for the duration of this call only (it used to stay resident — 160 MiB at
    // R = 256, 5 GiB at R = 1024 — although nothing but this function reads it)
    uint32_t* d_mat_lin = nullptr; uint8_t* d_mine_lin = nullptr;
    hipError_t e = hipMalloc((void**)&d_mat_lin, ctx->vox * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&d_mine_lin, ctx->vox);
    if (e == hipSuccess) e = hipMemcpy(d_mat_lin, materials, ctx->vox * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_mine_lin, minefield, ctx->vox, hipMemcpyHostToDevice);
    int rc = RT_OK;
    if (e != hipSuccess) rc = fail(ctx, e == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP, std::string("rt_upload_world: ") + hipGetErrorString(e));
    else {
        ctx->has_world = false;
        ctx->world_resident = false;
        rc = reflatten(ctx, d_mine_lin, d_mat_lin);      // synchronises the stream before it returns
    }
    if (d_mat_lin) (void)hipFree(d_mat_lin);
    if (d_mine_lin) (void)hipFree(d_mine_lin);
    if (rc != RT_OK) return rc;
    ctx->has_world = true;
    ctx->world_resident = true;
    ctx->ev_world.forget();   // (the region is complete on the device: reflatten synchronised)
    return RT_OK;
}

int rt_slice_staging(RtContext* ctx, uint32_t** materials, uint8_t** minefield) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!materials || !minefield) return fail(ctx, RT_ERR_INVALID_ARG, "rt_slice_staging: null pointer");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    // staging of one slab: pinned host memory (the reference's upload buffers are host-visible mapped Vulkan buffers,
    // terrain_upload.rs:65-82) holding the materials, then the minefield, and its device twin
    const size_t n = (size_t)RT_SLICE_SIZE * (size_t)ctx->region * (size_t)ctx->region;
    StagingSet& s = ctx->slab_sets[ctx->slabs & 1u];   // the set the NEXT rt_upload_slice uses: the slab before last has left it
    RT_HIP(ctx, staging_claim(ctx, s, 5 * n, 5 * n));
    *materials = reinterpret_cast<uint32_t*>(s.host);
    *minefield = s.host + 4 * n;
    return RT_OK;
}

int rt_upload_slice(RtContext* ctx, int axis, int texel_offset, const uint32_t* materials, const uint8_t* minefield) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!materials || !minefield) return fail(ctx, RT_ERR_INVALID_ARG, "rt_upload_slice: null pointer");
    // (RtConfig.stream_history: the history, and the slabs that wait, change only once the slab is accepted)
    if (!ctx->stream_history) restart_history(ctx);
    invalidate_prepass(ctx);
    const size_t kR = (size_t)ctx->region;
    if (axis < 0 || axis > 2 || texel_offset < 0 || texel_offset + RT_SLICE_SIZE > ctx->region || texel_offset % RT_SLICE_SIZE != 0)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_upload_slice: bad axis or offset");
    if (!ctx->world_resident) return fail(ctx, RT_ERR_NOT_READY, "rt_upload_slice: upload the full region first");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    // Incremental and asynchronous.  The slab goes pinned host staging -> device staging (5 bytes x 16 x R^2) on the upload
    // stream; the render stream waits for that event (not the host), then ONE launch re-tiles the slab's 16 R^2 voxels into the
    // brick-swizzled arrays and a second rebuilds the nibble-map words it touches.  Frames in flight keep reading the region
    // until then by stream order — the host waits for nothing on the device (the reference blocks on vkQueueWaitIdle here,
    // pipeline.rs:181-189); only a previous slab still leaving the pinned staging is waited for.
    const size_t n = (size_t)RT_SLICE_SIZE * kR * kR;
    StagingSet& s = ctx->slab_sets[ctx->slabs & 1u];
    RT_HIP(ctx, staging_claim(ctx, s, 5 * n, 5 * n));
    if ((ctx->cfg.flags & RT_FLAG_TRUSTED_WORLD) == 0) {
        // values above 30 are rejected as in rt_upload_world — BEFORE anything is written or transferred: a rejected slab leaves
        // the region (and what can be drawn) as it was.  The bytes are in host memory, so the check is a host loop over 16 R^2
        // bytes (~20 us at R = 256) and needs no device round trip; a host that vouches for its data skips it.
        uint8_t worst = 0;
        for (size_t i = 0; i < n; i++) worst = minefield[i] > worst ? minefield[i] : worst;
        if (worst > rtd::kMaxStepValue)
            return fail(ctx, RT_ERR_INVALID_ARG, "minefield slab holds a value above 30 (the reference writes 0..6, src/world/chunk.rs:163-183); the region is unchanged");
    }
    uint32_t* h_mat = reinterpret_cast<uint32_t*>(s.host);
    uint8_t* h_mine = s.host + 4 * n;
    if (materials != h_mat) memcpy(h_mat, materials, n * sizeof(uint32_t));   // borrowed buffers are released at return;
    if (minefield != h_mine) memcpy(h_mine, minefield, n);                     // rt_slice_staging's pointers need no copy
    ctx->slabs++;
    uint32_t* masks = ctx->stream_history ? slab_take_slot(ctx) : nullptr;
    RT_HIP(ctx, world_send(ctx, s, 5 * n));
    RT_HIP(ctx, slab_scan_old(ctx, masks, axis, texel_offset));
    {
        LaunchTimer t(ctx, 1);
        RT_HIP(ctx, rtd::launch_flatten_slab(s.dev + 4 * n, reinterpret_cast<const uint32_t*>(s.dev), ctx->d_mine_sw, ctx->d_mat_sw,
                                             ctx->d_coarse, ctx->d_brick, ctx->logr, axis, texel_offset, ctx->stream));
    }
    RT_HIP(ctx, slab_scan_new(ctx, masks, axis, texel_offset));
    RT_HIP(ctx, world_applied(ctx, s));
    return RT_OK;
}

int rt_generate_world(RtContext* ctx, uint64_t seed, const int64_t window_lo[3]) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const int64_t R = ctx->region;
    const int64_t lo[3] = {window_lo ? window_lo[0] : -R / 2, window_lo ? window_lo[1] : -R / 2, window_lo ? window_lo[2] : -R / 2};
    const int64_t ext[3] = {R, R, R};
    if (!terrain_window_ok(lo, ext))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_generate_world: window_lo must be a multiple of 16 and the window inside int32; nothing was enqueued");
    const int rc = generate_terrain(ctx, seed, lo, -1);
    if (rc != RT_OK) return rc;
    ctx->has_world = true;
    ctx->world_resident = true;
    return RT_OK;
}

int rt_generate_slice(RtContext* ctx, uint64_t seed, int axis, const int64_t window_lo[3]) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (axis < 0 || axis > 2 || !window_lo) return fail(ctx, RT_ERR_INVALID_ARG, "rt_generate_slice: bad axis or null window; nothing was enqueued");
    const int64_t R = ctx->region;
    const int64_t lo[3] = {window_lo[0], window_lo[1], window_lo[2]};
    const int64_t ext[3] = {axis == 0 ? RT_SLICE_SIZE : R, axis == 1 ? RT_SLICE_SIZE : R, axis == 2 ? RT_SLICE_SIZE : R};
    if (!terrain_window_ok(lo, ext))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_generate_slice: window_lo must be a multiple of 16 and the window inside int32; nothing was enqueued");
    if (!ctx->world_resident) return fail(ctx, RT_ERR_NOT_READY, "rt_generate_slice: upload or generate the full region first");
    return generate_terrain(ctx, seed, lo, axis);
}

int rt_edit_voxels(RtContext* ctx, const RtVoxelEdit* edits, uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (count > (1u << 24)) return fail(ctx, RT_ERR_INVALID_ARG, "rt_edit_voxels: more than 2^24 edits in one call; nothing was applied");
    if (count == 0) return RT_OK;
    if (!edits) return fail(ctx, RT_ERR_INVALID_ARG, "rt_edit_voxels: null edits");
    if (!ctx->world_resident) return fail(ctx, RT_ERR_NOT_READY, "rt_edit_voxels: upload the full region first");
    // Binning on the host, all of it before anything is enqueued (edit_binning.hpp)
    EditBins bins;
    const uint32_t bad = edit_bin(ctx->edit_binning, edits, count, ctx->logr, &bins);
    if (bad != count)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_edit_voxels: edit " + std::to_string(bad) +
                                                 " has a coordinate outside the region or reserved != 0; nothing was applied");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    // (not staging_alloc alone: a set that grows for 43.7 to 64 KiB of need has always got half as much again here, not 64 KiB)
    const size_t half_more = align16(bins.need + bins.need / 2u), cap = half_more > staging_alloc(bins.need) ? half_more : staging_alloc(bins.need);
    // the chunk ids, the per-chunk edit ranges, the records; one pending box per touched chunk
    return chunk_edit(
        ctx, bins.need, cap, bins.touched, bins.touched,
        [&](uint8_t* host) {
            const uint32_t nrec = edit_fill(ctx->edit_binning, edits, ctx->logr, reinterpret_cast<uint32_t*>(host),
                                            reinterpret_cast<uint32_t*>(host + bins.off_offs), reinterpret_cast<uint32_t*>(host + bins.off_recs));
            return bins.off_recs + (size_t)nrec * 8u;
        },
        [&](EditBox* boxes) { return edit_chunk_boxes(ctx->edit_binning, edits, ctx->logr, boxes); },
        [&](const uint8_t* dev) -> int {
            LaunchTimer lt(ctx, 1);
            RT_HIP(ctx, rtd::launch_rebuild_chunks(ctx->d_mine_sw, ctx->d_mat_sw, reinterpret_cast<const uint32_t*>(dev),
                                                   reinterpret_cast<const uint32_t*>(dev + bins.off_offs), reinterpret_cast<const uint2*>(dev + bins.off_recs),
                                                   bins.touched, ctx->logr, ctx->stream));
            return RT_OK;
        });
}

int rt_edit_shapes(RtContext* ctx, const RtShapeEdit* shapes, uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (count > kMaxShapes) return fail(ctx, RT_ERR_INVALID_ARG, "rt_edit_shapes: more than 4096 shapes in one call; nothing was applied");
    if (count == 0) return RT_OK;
    if (!shapes) return fail(ctx, RT_ERR_INVALID_ARG, "rt_edit_shapes: null shapes");
    if (!ctx->world_resident) return fail(ctx, RT_ERR_NOT_READY, "rt_edit_shapes: upload the full region first");
    // Validation, bounding boxes and the touched chunks on the host, all of it before anything is enqueued (edit_shapes.hpp)
    const uint32_t bad = shapes_validate(shapes, count, ctx->logr);
    if (bad != count)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_edit_shapes: shape " + std::to_string(bad) +
                                                 " has a bad kind, where or reserved, a coordinate outside [-4R, 4R], a box with a > b or a"
                                                 " sphere with b[0] outside [0, 2^26] or b[1], b[2] != 0; nothing was applied");
    const ShapePlan plan = shapes_touched(ctx->shape_scratch, shapes, count, ctx->logr);
    if (plan.touched == 0u) return RT_OK;   // (every shape lies outside the region: nothing is enqueued, nothing is reset)
    RT_HIP(ctx, hipSetDevice(ctx->device));
    // the chunk ids, then the records; one pending box per shape that has a bounding box
    return chunk_edit(
        ctx, plan.need, staging_alloc(plan.need), plan.touched, plan.boxes,
        [&](uint8_t* host) {
            shapes_fill_chunks(ctx->shape_scratch, reinterpret_cast<uint32_t*>(host));
            memcpy(host + plan.off_shapes, shapes, (size_t)count * sizeof(RtShapeEdit));
            return plan.need;
        },
        [&](EditBox* boxes) { return shape_pending_boxes(shapes, count, ctx->logr, boxes); },
        [&](const uint8_t* dev) -> int {
            LaunchTimer lt(ctx, 1);
            RT_HIP(ctx, rtd::launch_shape_chunks(ctx->d_mine_sw, ctx->d_mat_sw, reinterpret_cast<const uint32_t*>(dev), dev + plan.off_shapes, count,
                                                 plan.touched, ctx->logr, ctx->stream));
            return RT_OK;
        });
}

int rt_deposit_particles(RtContext* ctx, const RtParticleDeposit* params, RtParticleState* states, RtParticle* draw, uint32_t count,
                         RtDepositCount* counts) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    DepositPlan plan;
    int rc = deposit_check(ctx, "rt_deposit_particles", params, states, draw, count, counts, &plan);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    // states, draw records and counts through the synchronous calls' pinned and device block on the render stream, the launches
    // there, and all three back
    const size_t state_bytes = (size_t)count * sizeof(RtParticleState), draw_bytes = draw ? (size_t)count * sizeof(RtParticle) : 0u;
    const RtDepositCount before = counts ? *counts : RtDepositCount{0u, 0u, 0u, 0u};
    uint8_t* dev[3];
    rc = stage_sync(ctx, ctx->stream, {{states, state_bytes}, {&before, sizeof before}, {draw, draw_bytes}}, dev);
    if (rc != RT_OK) return rc;
    rc = deposit_run(ctx, *params, plan, dev[0], draw ? dev[2] : nullptr, dev[1], count);
    if (rc != RT_OK) return rc;
    const size_t bytes = (size_t)(dev[2] - dev[0]) + draw_bytes;
    RT_HIP(ctx, hipMemcpyAsync(ctx->query_block.host, ctx->query_block.dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(states, ctx->query_block.host, state_bytes);
    if (counts) memcpy(counts, ctx->query_block.host + (dev[1] - dev[0]), sizeof *counts);
    if (draw) memcpy(draw, ctx->query_block.host + (dev[2] - dev[0]), draw_bytes);
    return RT_OK;
}

int rt_deposit_particles_async(RtContext* ctx, const RtParticleDeposit* params, RtParticleState* states_dev, RtParticle* draw_dev,
                               uint32_t count, RtDepositCount* counts_dev) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    DepositPlan plan;
    int rc = deposit_check(ctx, "rt_deposit_particles_async", params, states_dev, draw_dev, count, counts_dev, &plan);
    if (rc != RT_OK && rc != 1) return rc;
    if (count == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!query_device_ptr(ctx, states_dev) || (draw_dev && !query_device_ptr(ctx, draw_dev)) || (counts_dev && !query_device_ptr(ctx, counts_dev)))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_deposit_particles_async: states, draw and counts must be 16-byte aligned memory of the context's device");
    if (rc == 1) return RT_OK;
    return deposit_run(ctx, *params, plan, states_dev, draw_dev, counts_dev, count);
}

int rt_settle_voxels(RtContext* ctx, const RtVoxelSettle* params, RtSettleCount* counts) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    SettlePlan plan;
    int rc = settle_check(ctx, "rt_settle_voxels", params, &plan);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!counts) return settle_run(ctx, *params, plan, nullptr);
    // the counts through the synchronous calls' pinned and device block on the render stream, the launches there, and the counts back
    uint8_t* dev[1];
    rc = stage_sync(ctx, ctx->stream, {{counts, sizeof *counts}}, dev);
    if (rc != RT_OK) return rc;
    rc = settle_run(ctx, *params, plan, dev[0]);
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipMemcpyAsync(ctx->query_block.host, ctx->query_block.dev, sizeof *counts, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(counts, ctx->query_block.host, sizeof *counts);
    return RT_OK;
}

int rt_settle_voxels_async(RtContext* ctx, const RtVoxelSettle* params, RtSettleCount* counts_dev) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    SettlePlan plan;
    const int rc = settle_check(ctx, "rt_settle_voxels_async", params, &plan);
    if (rc != RT_OK && rc != 1) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (counts_dev && !query_device_ptr(ctx, counts_dev))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_settle_voxels_async: counts must be 16-byte aligned memory of the context's device");
    if (rc == 1) return RT_OK;
    return settle_run(ctx, *params, plan, counts_dev);
}

int rt_flow_voxels(RtContext* ctx, const RtVoxelFlow* params, RtFlowCount* counts) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    FlowPlan plan;
    int rc = flow_check(ctx, "rt_flow_voxels", params, &plan);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!counts) return flow_run(ctx, *params, plan, nullptr);
    // the counts through the synchronous calls' pinned and device block on the render stream, the launches there, and the counts back
    uint8_t* dev[1];
    rc = stage_sync(ctx, ctx->stream, {{counts, sizeof *counts}}, dev);
    if (rc != RT_OK) return rc;
    rc = flow_run(ctx, *params, plan, dev[0]);
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipMemcpyAsync(ctx->query_block.host, ctx->query_block.dev, sizeof *counts, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(counts, ctx->query_block.host, offsetof(RtFlowCount, reserved));   // (reserved is never written)
    return RT_OK;
}

int rt_flow_voxels_async(RtContext* ctx, const RtVoxelFlow* params, RtFlowCount* counts_dev) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    FlowPlan plan;
    const int rc = flow_check(ctx, "rt_flow_voxels_async", params, &plan);
    if (rc != RT_OK && rc != 1) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (counts_dev && !query_device_ptr(ctx, counts_dev))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_flow_voxels_async: counts must be 16-byte aligned memory of the context's device");
    if (rc == 1) return RT_OK;
    return flow_run(ctx, *params, plan, counts_dev);
}

int rt_detach_voxels(RtContext* ctx, const RtVoxelDetach* params, RtDetachResult* result, uint32_t* stamp_out) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    DetachPlan plan;
    int rc = detach_check(ctx, "rt_detach_voxels", params, stamp_out, &plan);
    if (rc == 1 && stamp_out) *stamp_out = 0u;
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!result) return detach_run(ctx, *params, plan, nullptr, stamp_out);
    // the result through the synchronous calls' pinned and device block on the render stream, the launches there, and the result back
    uint8_t* dev[1];
    rc = stage_sync(ctx, ctx->stream, {{result, sizeof *result}}, dev);
    if (rc != RT_OK) return rc;
    rc = detach_run(ctx, *params, plan, dev[0], stamp_out);
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipMemcpyAsync(ctx->query_block.host, ctx->query_block.dev, sizeof *result, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(result, ctx->query_block.host, sizeof *result);
    return RT_OK;
}

int rt_detach_voxels_async(RtContext* ctx, const RtVoxelDetach* params, RtDetachResult* result_dev, uint32_t* stamp_out) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    DetachPlan plan;
    const int rc = detach_check(ctx, "rt_detach_voxels_async", params, stamp_out, &plan);
    if (rc != RT_OK && rc != 1) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (result_dev && !query_device_ptr(ctx, result_dev))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_detach_voxels_async: result must be 16-byte aligned memory of the context's device");
    if (rc == 1) {
        if (stamp_out) *stamp_out = 0u;
        return RT_OK;
    }
    return detach_run(ctx, *params, plan, result_dev, stamp_out);
}

int rt_stamp_create(RtContext* ctx, const int32_t extent[3], const uint32_t* materials, const uint8_t* state, uint32_t* id_out) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!extent || !materials || !state || !id_out) return fail(ctx, RT_ERR_INVALID_ARG, "rt_stamp_create: null pointer");
    if (!stamp_extent_valid(extent)) return fail(ctx, RT_ERR_INVALID_ARG, "rt_stamp_create: an extent outside 1..256");
    const size_t n = (size_t)extent[0] * (size_t)extent[1] * (size_t)extent[2];
    for (size_t i = 0; i < n; i++)
        if (state[i] > RT_STAMP_SOLID) return fail(ctx, RT_ERR_INVALID_ARG, "rt_stamp_create: a state above 2");
    if (ctx->stamps.live == kMaxStamps) return fail(ctx, RT_ERR_INVALID_ARG, "rt_stamp_create: 1024 stamps are live");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->upload_stream) RT_HIP(ctx, new_stream(ctx, &ctx->upload_stream));
    StampEntry* e = ctx->stamps.add(extent);
    RT_HIP(ctx, stamp_alloc(ctx, e));
    // the arrays, then the words of ABSENT voxels cleared, on the upload stream; the host waits for both, so that the caller's
    // arrays are free and every later call, whatever its stream, finds the stamp complete
    hipError_t err = hipMemcpyAsync(reinterpret_cast<void*>(e->mats), materials, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->upload_stream);
    if (err == hipSuccess) err = hipMemcpyAsync(reinterpret_cast<void*>(e->state), state, n, hipMemcpyHostToDevice, ctx->upload_stream);
    if (err == hipSuccess) err = rtd::launch_stamp_clean(reinterpret_cast<uint32_t*>(e->mats), reinterpret_cast<const uint8_t*>(e->state), (uint32_t)n, ctx->upload_stream);
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->upload_stream);
    if (err != hipSuccess) {
        stamp_free(ctx, e);
        return fail(ctx, err == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP, std::string("rt_stamp_create: ") + hipGetErrorString(err));
    }
    *id_out = e->id;
    return RT_OK;
}

int rt_stamp_capture(RtContext* ctx, const int32_t lo[3], const int32_t extent[3], uint32_t flags, uint32_t* id_out) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!lo || !extent || !id_out) return fail(ctx, RT_ERR_INVALID_ARG, "rt_stamp_capture: null pointer");
    if ((flags & ~RT_STAMP_SKIP_AIR) != 0u) return fail(ctx, RT_ERR_INVALID_ARG, "rt_stamp_capture: unknown flag");
    if (!stamp_extent_valid(extent)) return fail(ctx, RT_ERR_INVALID_ARG, "rt_stamp_capture: an extent outside 1..256");
    for (int k = 0; k < 3; k++)
        if (lo[k] < 0 || extent[k] > ctx->region - lo[k]) return fail(ctx, RT_ERR_INVALID_ARG, "rt_stamp_capture: box outside the region");
    if (!ctx->world_resident) return fail(ctx, RT_ERR_NOT_READY, "rt_stamp_capture: upload the full region first");
    if (ctx->stamps.live == kMaxStamps) return fail(ctx, RT_ERR_INVALID_ARG, "rt_stamp_capture: 1024 stamps are live");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    StampEntry* e = ctx->stamps.add(extent);
    RT_HIP(ctx, stamp_alloc(ctx, e));
    // One launch on the stream the edits use: behind every earlier world change (they ran there, or the lanes were fenced behind
    // them), and every later one joins the lanes before it writes.  It reads the region only, so frames and ray queries need no
    // order.  It WRITES the stamp's arrays: what reads them on this stream (placements, draws, shadows) follows in stream order, and an
    // entity query, which reads them on the query stream, waits for ev_capture.
    hipError_t err = ctx->ev_capture.ev ? hipSuccess : new_event(ctx, &ctx->ev_capture.ev);
    if (err == hipSuccess) {
        LaunchTimer lt(ctx, 1);
        err = rtd::launch_stamp_capture(ctx->d_mine_sw, ctx->d_mat_sw, ctx->logr, lo[0], lo[1], lo[2], extent[0], extent[1], extent[2],
                                        (flags & RT_STAMP_SKIP_AIR) != 0u, reinterpret_cast<uint32_t*>(e->mats), reinterpret_cast<uint8_t*>(e->state),
                                        ctx->stream);
    }
    if (err == hipSuccess) err = ctx->ev_capture.record(ctx->stream);
    if (err == hipSuccess) err = fence_lanes_after(ctx, ctx->stream);   // (a later change may start on the other lane's stream)
    if (err != hipSuccess) {
        (void)hipStreamSynchronize(ctx->stream);
        stamp_free(ctx, e);
        return fail(ctx, RT_ERR_HIP, std::string("rt_stamp_capture: ") + hipGetErrorString(err));
    }
    e->used = true;
    *id_out = e->id;
    return RT_OK;
}

int rt_stamp_info(RtContext* ctx, uint32_t id, int32_t extent_out[3]) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const StampEntry* e = ctx->stamps.find(id);
    if (!e) return fail(ctx, RT_ERR_INVALID_ARG, "rt_stamp_info: unknown stamp id");
    if (!extent_out) return fail(ctx, RT_ERR_INVALID_ARG, "rt_stamp_info: null pointer");
    for (int k = 0; k < 3; k++) extent_out[k] = e->ext[k];
    return RT_OK;
}

int rt_stamp_read(RtContext* ctx, uint32_t id, uint32_t* materials, uint8_t* state) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    StampEntry* e = ctx->stamps.find(id);
    if (!e) return fail(ctx, RT_ERR_INVALID_ARG, "rt_stamp_read: unknown stamp id");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, sync_lanes(ctx));   // (a capture may still be writing it)
    e->used = false;
    if (materials) RT_HIP(ctx, hipMemcpy(materials, reinterpret_cast<const void*>(e->mats), e->voxels() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (state) RT_HIP(ctx, hipMemcpy(state, reinterpret_cast<const void*>(e->state), e->voxels(), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_stamp_destroy(RtContext* ctx, uint32_t id) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    StampEntry* e = ctx->stamps.find(id);
    if (!e) return fail(ctx, RT_ERR_INVALID_ARG, "rt_stamp_destroy: unknown stamp id");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (e->used) RT_HIP(ctx, sync_lanes(ctx));   // the capture that wrote it and the placements that read it have finished
    stamp_free(ctx, e);
    return RT_OK;
}

int rt_edit_stamps(RtContext* ctx, const RtStampPlace* places, uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (count > kMaxStampPlaces) return fail(ctx, RT_ERR_INVALID_ARG, "rt_edit_stamps: more than 4096 placements in one call; nothing was applied");
    if (count == 0) return RT_OK;
    if (!places) return fail(ctx, RT_ERR_INVALID_ARG, "rt_edit_stamps: null places");
    if (!ctx->world_resident) return fail(ctx, RT_ERR_NOT_READY, "rt_edit_stamps: upload the full region first");
    // Validation, bounding boxes and the touched chunks on the host, all of it before anything is enqueued (edit_stamps.hpp)
    const uint32_t bad = places_validate(ctx->stamps, places, count, ctx->logr);
    if (bad != count)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_edit_stamps: placement " + std::to_string(bad) +
                                                 " has an unknown stamp id, orient >= 48, where > 2, a non-zero reserved field or an at[k]"
                                                 " outside [-4R, 4R]; nothing was applied");
    const StampPlan plan = stamps_touched(ctx->shape_scratch, ctx->stamps, places, count, ctx->logr);
    if (plan.touched == 0u) return RT_OK;   // (every placement lies outside the region: nothing is enqueued, nothing is reset)
    RT_HIP(ctx, hipSetDevice(ctx->device));
    // the chunk ids, then one record per placement with the id resolved into the stamp's device arrays; one pending box per placement
    // that has a bounding box
    return chunk_edit(
        ctx, plan.need, staging_alloc(plan.need), plan.touched, plan.boxes,
        [&](uint8_t* host) {
            shapes_fill_chunks(ctx->shape_scratch, reinterpret_cast<uint32_t*>(host));
            stamp_fill_records(ctx->stamps, places, count, ctx->logr, reinterpret_cast<StampRecord*>(host + plan.off_recs));
            for (uint32_t i = 0; i < count; i++) ctx->stamps.find(places[i].stamp)->used = true;
            return plan.need;
        },
        [&](EditBox* boxes) { return stamp_pending_boxes(ctx->stamps, places, count, ctx->logr, boxes); },
        [&](const uint8_t* dev) -> int {
            LaunchTimer lt(ctx, 1);
            RT_HIP(ctx, rtd::launch_stamp_chunks(ctx->d_mine_sw, ctx->d_mat_sw, reinterpret_cast<const uint32_t*>(dev), dev + plan.off_recs, count,
                                                 plan.touched, ctx->logr, ctx->stream));
            return RT_OK;
        });
}

int rt_read_box(RtContext* ctx, int x0, int y0, int z0, int ex, int ey, int ez, uint32_t* materials, uint8_t* minefield) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const int R = ctx->region;
    if (x0 < 0 || y0 < 0 || z0 < 0 || ex < 1 || ey < 1 || ez < 1 || ex > R - x0 || ey > R - y0 || ez > R - z0)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_read_box: box outside the region");
    if (!ctx->world_resident) return fail(ctx, RT_ERR_NOT_READY, "rt_read_box: no region uploaded");
    if (!materials && !minefield) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, sync_lanes(ctx));
    // z-slabs of at most 2^24 voxels through a temporary device buffer (80 MiB)
    const size_t plane = (size_t)ex * (size_t)ey;
    const int nz = (int)(((size_t)1 << 24) / plane >= (size_t)ez ? (size_t)ez : (((size_t)1 << 24) / plane > 0 ? ((size_t)1 << 24) / plane : 1));
    uint32_t* d_mat = nullptr; uint8_t* d_mine = nullptr;
    hipError_t e = hipSuccess;
    if (materials) e = hipMalloc((void**)&d_mat, plane * (size_t)nz * sizeof(uint32_t));
    if (e == hipSuccess && minefield) e = hipMalloc((void**)&d_mine, plane * (size_t)nz);
    for (int z = 0; z < ez && e == hipSuccess; z += nz) {
        const int n = ez - z < nz ? ez - z : nz;
        e = rtd::launch_read_box(ctx->d_mine_sw, ctx->d_mat_sw, ctx->logr, x0, y0, z0 + z, ex, ey, n, d_mat, d_mine, ctx->stream);
        if (e == hipSuccess && materials)
            e = hipMemcpyAsync(materials + plane * (size_t)z, d_mat, plane * (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && minefield)
            e = hipMemcpyAsync(minefield + plane * (size_t)z, d_mine, plane * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (d_mat) (void)hipFree(d_mat);
    if (d_mine) (void)hipFree(d_mine);
    if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP, std::string("rt_read_box: ") + hipGetErrorString(e));
    return RT_OK;
}

}  // extern "C"
