// rt_context.hpp — the context behind the C ABI of include/rt_abi.h, shared by the api_*.hip translation units: its structs and
// constants, the small helper types (LatchEvent, StagingBlock, TimingPool, env_int), the hand-over of a staging set (staging_claim,
// staging_send), the synchronous calls' staging (stage_sync) and the few functions that cross files.
//
// One context = one GPU.  Nothing here runs ray-trace work on the CPU: if the HIP runtime or a device is missing, rt_create fails
// with RT_ERR_NO_DEVICE and the caller gets no context.  Everything internal lives in namespace rta (hidden visibility): the
// library exports the C ABI and nothing of this.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../../include/rt_abi.h"
#include "../../../include/rt_math.h"
#include "../rt_kernels.hpp"
#include "edit_binning.hpp"
#include "edit_shapes.hpp"
#include "edit_stamps.hpp"
#include "draw_stamps.hpp"
#include "nav_check.hpp"

namespace rta __attribute__((visibility("hidden"))) {

constexpr size_t kBytesPerPixel[RT_BUF_COUNT] = {8, 2, 1, 4, 4, 4, 16, 16, 4, 4};

constexpr size_t kWlSetWords = 64, kWlClearWords = 33;   // FrameSlot::wl_count: words of one set, and those of it that are in use
constexpr size_t kCursorWords = 8 * 32;   // path cursors of the persistent kernels: one word per XCD group, each on its own 128-byte line
// light records of one launch above which k_paths streams them out and k_accumulate_paths streams them in (see frame_path_batches)
constexpr uint64_t kStreamRecordBytes = 384ull << 20;

// ---- the route: which kernel each launch of a frame runs on (Route, resolve_route) --------------------------------------------
// RT_KERNEL_DEFAULT: ONE-sample frames of fewer pixels than this run on k_frame — the whole frame in one launch, no prepass,
// worklist or accumulate (rt_frame.hip; RT_FRAME_CROSSOVER overrides).  Measured (profiles/r4_frame_kernel.txt), k_frame against
// prepass + k_persist, ms per frame: 256^2 0.084 / 0.186, 1024^2 (the reference's frame) 0.163 / 0.225, 1280x720 0.155 / 0.218,
// 1920x1080 0.275 / 0.297, 2048x1440 0.355 / 0.360 (k_paths: 0.353).
constexpr uint64_t kFrameCrossover = 5ull << 19;
// More than one sample per pixel: k_frame deals the (pixel, sample) paths of a workgroup's pixels to its lanes and adds a pixel's
// samples in order itself.  It wins while the frame is so small that the persistent kernels' ~0.14 ms per launch dominates — measured
// (k_frame / k_persist, ms per frame): 256^2 spp 2 depth 2 0.105 / 0.176, spp 4 depth 2 0.106 / 0.179, 128^2 spp 16 depth 4 0.213 / 0.206,
// 256^2 spp 16 depth 4 0.246 / 0.211, 512^2 spp 4 depth 4 0.234 / 0.217, 1024^2 spp 2 depth 4 0.352 / 0.290 — i.e. below about 1.5 M
// pixel-sample-levels (pixels x spp x depth; RT_FRAME_CROSSOVER_MULTI overrides).
constexpr uint64_t kFrameCrossoverMulti = 3ull << 19;
// RT_KERNEL_DEFAULT, frames k_frame does not take: path launches of at least this many pixel-samples run on k_paths, smaller ones on
// k_persist.  k_paths pays for its two contexts per lane once there is enough work to keep them filled: measured crossover against
// k_persist (tools/kernel_crossover.sh) between 4 M and 8 M paths per launch — 1080p spp 1: 0.28 against 0.22 ms, 256^2 spp 64: 0.35
// against 0.32, 1080p spp 4: 0.47 against 0.50, spp 16: 1.29 against 1.65; the reference's own 1024^2 1-spp frame: 0.20 against 0.14;
// round 3, same box: 1080p spp 1 (2.1 M) 0.351 against 0.348 ms per frame, spp 2 (4.1 M) 0.409 against 0.442; 1024^2 spp 1 0.252
// against 0.229.  (RT_KERNEL_PATHS and RT_KERNEL_FRAME ask for k_paths whatever the size.)
constexpr uint64_t kPathsCrossover = 3ull << 20;

constexpr size_t kMaxTimerEvents = 2 * 4096;   // TimingPool cap: pairs beyond it are not timed (LaunchTimer counts them in timer_overflow)

struct Route {
    int family = RT_KERNEL_PERSISTENT;   // RT_KERNEL_MEGA, RT_KERNEL_WAVEFRONT, or RT_KERNEL_PERSISTENT (k_frame, k_persist and k_paths)
    bool frame = false;                  // every frame is one k_frame launch
    uint32_t paths_from = UINT32_MAX;    // path launches of at least this many samples run on k_paths, smaller ones on k_persist
    uint32_t threshold_persist = 0, threshold_paths = 0;   // PersistArgs::threshold of a k_persist / k_paths launch
    bool direct = false;                 // one-sample launches store the pixel's lighting themselves: no light records, no accumulate
    int in_use = RT_KERNEL_PERSISTENT;   // rt_kernel_in_use: the kernel of a frame's last launch
    bool on_paths(uint32_t ns) const { return ns >= paths_from; }
};

// An event that may not have been recorded yet: waiting for it is a no-op until it has been.
struct LatchEvent {
    hipEvent_t ev = nullptr;
    hipStream_t on = nullptr;   // the stream of the record
    bool recorded = false;
    hipError_t record(hipStream_t st) {
        const hipError_t e = hipEventRecord(ev, st);
        if (e == hipSuccess) { recorded = true; on = st; }
        return e;
    }
    hipError_t wait(hipStream_t st) const { return recorded ? hipStreamWaitEvent(st, ev, 0) : hipSuccess; }
    // ... and none either when `st` is the stream it was recorded on (stream order does it)
    hipError_t wait_elsewhere(hipStream_t st) const { return on != st ? wait(st) : hipSuccess; }
    hipError_t host_wait() const { return recorded ? hipEventSynchronize(ev) : hipSuccess; }
    void forget() { recorded = false; }   // everything before has finished
};

// A pinned host block and its device twin of `cap` bytes each, replaced by a larger pair when a user needs more.
struct StagingBlock {
    uint8_t* host = nullptr;   // hipHostMalloc
    uint8_t* dev = nullptr;    // hipMalloc (counted in device_bytes)
    size_t cap = 0;
    // at least `need` bytes: a smaller pair is freed and one of `alloc` bytes takes its place (nobody may still be using the old one)
    hipError_t grow(RtContext* c, size_t need, size_t alloc);
    void release();
};

// Pinned host staging -> device twin (upload stream) -> the launch that applies it (render stream): rt_upload_slice's slabs and
// rt_edit_voxels' batches.  Each kind has TWO sets used in turn: transfer n waits for the launch of n - 2, not of n - 1,
// which sits behind the frames on the render stream — a host that sends one slab or batch per frame never waits for a frame.
struct StagingSet : StagingBlock {
    LatchEvent ev_copied;    // the transfer has read the host block (recorded = a copy is pending)
    LatchEvent ev_applied;   // the launch has read the device block
};

// (start, stop) event pairs round launches, summed and reused by drain.  The pool owns its events.
struct TimingPool {
    static constexpr size_t npos = (size_t)-1;
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    // the index of a pair whose start is recorded on `st`; npos with *e == hipSuccess when the pool is full, with the error otherwise
    size_t acquire(hipStream_t st, hipError_t* e) {
        *e = hipSuccess;
        if (used + 2 > kMaxTimerEvents) return npos;
        while (ev.size() < used + 2) {
            hipEvent_t n;
            if ((*e = hipEventCreate(&n)) != hipSuccess) return npos;
            ev.push_back(n);
        }
        const size_t idx = used;
        used += 2;
        *e = hipEventRecord(ev[idx], st);
        return idx;
    }
    hipError_t release(size_t idx, hipStream_t st) { return hipEventRecord(ev[idx + 1], st); }
    // each(pair, ms) for every pair handed out since the last drain (the caller has synchronised their streams)
    template <typename F>
    hipError_t drain(F&& each) {
        for (size_t i = 0; i + 1 < used; i += 2) {
            float ms = 0.0f;
            const hipError_t e = hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            if (e != hipSuccess) return e;
            each(i / 2, ms);
        }
        used = 0;
        return hipSuccess;
    }
};

struct Lane {
    hipStream_t stream = nullptr;      // lane 0: the context's stream (its own or the caller's, rt_set_stream); lane 1: the library's second stream
    uint32_t* cursor = nullptr;        // kCursorWords: eight path cursors, one 128-byte line each
    bool cursor_clean = false;         // all zero (create-time memset, or the prepass in front of the launch cleared it)
    uint32_t* pstack = nullptr;        // albedo stack of the launch in flight (global part)
    rtd::PathLight* ppl = nullptr;     // light records of the launch in flight
    hipEvent_t ev_join = nullptr;      // "everything submitted to this lane so far" (join_lanes_into)
};
struct FrameSlot {
    void* planes[RT_BUF_COUNT] = {};
    void* gbuffer = nullptr;           // planes 0..5 back to back (256-byte aligned each)
    uint32_t* worklist = nullptr;
    float4* phit = nullptr;            // primary-hit records of the worklist (rtd::PrimaryArgs::phit)
    float4* pacc = nullptr;
    uint32_t* wl_count = nullptr;      // two sets of kWlSetWords: worklist counter (word 0) and the prepass' tile cursor (word 32), on lines of
                                       // their own; the frame in the slot uses set [wl_parity] while its prepass clears the other
    int wl_parity = 0;                 // the set the slot's NEXT prepass uses (the prepass that ran last used the other)
    bool wl_clean[2] = {false, false};
    // the slot holds the prepass of a frame drawn under prepass_key (worklist, count, primary hits, the primary-only planes, finished sky
    // lighting) and nothing has changed what that prepass read or wrote since: a frame with the same key may skip its prepass
    bool prepass_valid = false;
    uint32_t prepass_key[16] = {};
    void* denoise_work[2] = {nullptr, nullptr};   // ping/pong working planes of the denoise passes (16 B/pixel), allocated on first use
    hipEvent_t ev_prepass = nullptr;   // the frame's prepass and tables are done (launches on the other lane wait for it)
    hipEvent_t ev_acc = nullptr;       // the frame's most recent accumulate launch (the next one adds to the same sums, in sample order)
    LatchEvent ev_tail;                // everything submitted for the frame in this slot: the slot's next frame starts after it
};

// the wavefront baseline's queues: the launch arguments as create_wavefront filled them (draw_wavefront sets what varies per batch
// and level in a copy)
struct WavefrontState {
    rtd::TraceArgs trace{};
    rtd::ShadeArgs shade{};
    float4* acc = nullptr;
    uint32_t* ctrl = nullptr;     // per batch: [RT_MAX_DEPTH+2] pair counts, then [RT_MAX_DEPTH+2] cursors
    uint32_t batch_samples = 1;   // samples per batch
    uint32_t cap = 0;             // paths per batch (allocation)
    uint32_t refill_threshold = 24;
};

}  // namespace rta

struct __attribute__((visibility("hidden"))) RtContext {
    RtConfig cfg{};
    int device = 0;
    int num_cus = 256;
    int logr = 8;                       // log2 of the region edge
    int region = RT_ROOT_BLOCK_SIZE;    // R
    size_t vox = 0;                     // R^3
    hipStream_t own_stream = nullptr, stream = nullptr;   // stream: where the frame drawn last ended (post passes, gather, readback follow it there)
    bool user_stream = false;           // rt_set_stream gave a stream: one lane, one slot
    std::string err = "";
    bool has_world = false, has_noise = false;
    bool world_resident = false;          // a full region has been uploaded once (slabs may patch it)

    // every stream and event the context made (new_stream, new_event), the timing pools' apart: rt_destroy's list
    std::vector<hipEvent_t> events;
    std::vector<hipStream_t> streams;

    // scene
    // (the caller-layout copy of the region exists only inside rt_upload_world: 5 B/voxel, 5 GiB at R = 1024)
    uint8_t* d_mine_sw = nullptr; uint32_t* d_mat_sw = nullptr;
    uint32_t* d_coarse = nullptr; uint32_t* d_noise = nullptr; uint32_t* d_flag = nullptr;
    uint32_t* d_brick = nullptr;          // R > 256: per-brick nibble map (rtd::Scene::brick), R^3 / 128 bytes
    // staging (StagingSet): rt_upload_slice's 16-thick slab (materials, then minefield at 4 x 16 R^2) is re-tiled, rt_edit_voxels'
    // binned batch (touched chunks, per-chunk edit ranges, records) and rt_edit_shapes' (touched chunks, shape records) rebuild
    // their chunks, as does rt_edit_stamps' (touched chunks, one 64-byte record per placement); the edit sets grow when a batch needs more
    hipStream_t upload_stream = nullptr;
    rta::StagingSet slab_sets[2], edit_sets[2];
    uint64_t slabs = 0, edit_batches = 0;   // submitted so far: the next one uses set slabs & 1 / edit_batches & 1
    rta::EditBinning edit_binning;        // host binning scratch, kept between calls
    rta::ShapeScratch shape_scratch;      // rt_edit_shapes: the mark per chunk, kept between calls (it shares the edit sets)
    rta::StampStore stamps;               // the live voxel stamps (rt_stamp_*): device arrays of their own, counted in device_bytes
    rta::NavStore navs;                   // the live navigation fields (rt_nav_*): one device block each, counted in device_bytes
    int32_t* d_heights = nullptr;         // rt_generate_world / rt_generate_slice: column heights of (R/64 + 1)^2 chunks, on first use

    // tiling
    int tiles_x = 0, tiles_y = 0, ntiles_total = 0, ntiles_local = 0, tile_capacity = 0;
    uint32_t npix_pad = 0;     // ntiles_local * 64
    size_t plane_pixels = 0;   // pixels per output plane

    // the planes of the frame drawn last (aliases of its slot's: rt_device_ptr, rt_readback, the post passes and the gather use them)
    void* planes[RT_BUF_COUNT] = {};
    void* gbuffer = nullptr;
    size_t gbuffer_offset[6] = {};
    size_t gbuffer_bytes = 0;
    rta::Lane lanes[2];
    int nlanes = 1;                     // 2: path launches alternate between two streams (persistent kernels on the context's own stream)
    rta::FrameSlot slots[2];
    int nslots = 1;                     // 2 with RT_FLAG_FRAMES_IN_FLIGHT_2
    int cur_slot = 0;                   // slot of the frame drawn last
    uint64_t frames_drawn = 0, path_launches = 0;
    hipEvent_t ev_fence = nullptr;      // fence_lanes_after
    rta::LatchEvent ev_gather;          // the previous rt_gather_gbuffer (gathers share staging: they run one after the other)

    rta::Route route;

    rta::WavefrontState wave;     // wavefront pipeline state
    // persistent kernel state (per-launch and per-frame buffers live in the lanes and slots above)
    float4* sphere_lut = nullptr;
    float4* sun_lut = nullptr;
    float4* dif_lut = nullptr;
    uint32_t persist_batch = 1;
    int pl_stream_mode = -1;      // RT_PL_STREAM: -1 = by size (kStreamRecordBytes); bit 0 streaming stores, bit 1 streaming loads
    uint32_t persist_chunk = 0;   // RT_PERSIST_CHUNK: paths per cursor atomic (multiple of 64); 0 = automatic
    uint32_t persist_threshold = 0;   // RT_PERSIST_THRESHOLD: 0 = the route's default per kernel
    uint64_t frame_crossover = rta::kFrameCrossover;
    uint64_t frame_crossover_multi = rta::kFrameCrossoverMulti;   // ... and frames of more than one sample per pixel below this many pixel-sample-levels
    uint32_t frame_threshold = 0; // RT_FRAME_THRESHOLD: parked lanes per wave that trigger k_frame's pass; 0 = the default
    uint32_t frame_tiles = 0;     // RT_FRAME_TILES (per wave, 1..4) / RT_FRAME_GROUP_TILES (1..16): tiles per four-wave workgroup of k_frame; 0 = by frame size and spp
    float lut_key[6] = {0, 0, 0, 0, 0, 0};   // sun vector + colour the per-frame tables were built for
    bool lut_valid = false;
    int primary_version = 2;      // 1 = k_primary (thread per pixel), 2 = k_primary2 (nibble map in LDS); RT_PRIMARY_V
    rtd::DevCounters* d_counters = nullptr;
    unsigned long long* d_selftest = nullptr;
    uint64_t host_noise_base = 0, host_frames = 0;

    // timing
    hipEvent_t ev_frame0 = nullptr, ev_frame1 = nullptr;
    rta::TimingPool launch_times;   // LaunchTimer's pairs (rt_get_timing) ...
    std::vector<int> launch_kind; // ... and per pair: 0 = trace, 1 = other
    uint32_t timer_overflow = 0;  // launches that found the pool full (RT_FLAG_TIMING without rt_get_timing)
    bool frame_recorded = false;

    // multi-GPU gather (rt_gather_gbuffer): root's staging for the ranks' blocks; the overlapped mode's second stream,
    // two send-side staging copies of this rank's block and the events that order them
    void* frame_planes[6] = {};   // root, frames_dev == NULL: the library's own row-major full-frame planes (rt_frame_ptr)
    uint8_t* gathered[2] = {nullptr, nullptr};
    uint8_t* stage[2] = {nullptr, nullptr};
    hipStream_t gather_stream = nullptr;
    hipEvent_t ev_ready[2] = {nullptr, nullptr};
    rta::LatchEvent ev_free[2];
    uint64_t gathers = 0;
    rta::TimingPool gather_times;   // RT_FLAG_TIMING: pairs round the rt_gather_gbuffer calls (rt_get_gather_timing)

    std::vector<void*> allocs;
    uint64_t device_bytes = 0;       // sum of the context's device allocations (rt_get_info)
    uint64_t light_budget_bytes = 0; // what the per-path light records were sized for

    // progressive accumulation (RT_FLAG_ACCUMULATE): per-pixel running sum of the lighting by plane index (PixelId::out_index),
    // shared by the frame slots; what it holds is host-side state
    float4* d_accum = nullptr;
    bool accum_valid = false;           // the next frame may continue the sum (a frame was drawn and nothing reset it since)
    bool prepass_reuse = true;          // RT_PREPASS_REUSE=0: every frame runs its prepass (FrameSlot::prepass_valid)
    uint32_t accum_key[16] = {};        // live uniforms other than seed of the frame drawn last (bit patterns)
    uint64_t accum_frames = 0, accum_samples = 0;   // frames and samples the planes of the frame drawn last hold
    bool drawn = false;                 // a frame was drawn (rt_get_accumulation of a context without the flag)
    // the last step of the frame drawn last that touched d_accum (two lanes only): the step that touches the running sum follows
    // the previous frame's (wait_elsewhere), not the whole previous frame
    rta::LatchEvent ev_accum;
    // temporal reprojection (RT_FLAG_REPROJECT): two history sets used in turn — a frame's pass reads the set the previous frame's
    // pass wrote and writes the other.  Sums by row-major pixel (set 0's is d_accum) and (depth_f32 bits, count | normal << 27)
    // records; the previous frame's camera is accum_key's origin, forward, up and right
    bool reproject = false;
    uint32_t history_cap = 32;
    float4* d_hist_sum[2] = {nullptr, nullptr};
    uint2* d_hist_rec[2] = {nullptr, nullptr};
    int hist_cur = 0;                   // the set the pass of the frame drawn last wrote
    // RtConfig.edit_radius > 0 (with RT_FLAG_REPROJECT): rt_edit_voxels keeps the history and records one texel box per touched
    // chunk; the next frame drawn turns them into world boxes (its lr) and restarts only the pixels near or shadowed by one.
    // More than kTemporalMaxBoxes pending: the set is emptied and marked overflowed, and that frame restarts.
    uint32_t edit_radius = 0;           // 0: an edit restarts the history (accum_valid = false), no boxes are kept
    rta::EditBox edit_boxes[rtd::kTemporalMaxBoxes];
    uint32_t edit_nbox = 0;
    bool edit_overflow = false;
    // RtConfig.stream_history (with RT_FLAG_REPROJECT and edit_radius > 0): rt_upload_slice and rt_generate_slice keep the history.
    // An accepted slab takes the next of rtd::kSlabSlots mask slots — cleared and scanned in stream order round the launch that
    // writes the slab (rt_slab.hip) — and the next frame drawn consumes the pending slots: k_place_slab_boxes, then the moved pass
    // with the slab boxes.  A slot is written again only by a later slab call, whose launches follow every frame submitted before
    // it on every lane (world_change_begin), the frame that consumed the slot among them.
    bool stream_history = false;
    uint32_t* d_slab_masks = nullptr;   // kSlabSlots x kSlabSlotWords
    rtd::SlabBoxes* d_slab_boxes = nullptr;   // the frame's pass reads it behind k_place_slab_boxes, on the stream of both
    uint32_t slab_pending = 0;          // slots 0 .. slab_pending - 1 wait for the next frame, in call order
    bool slab_overflow = false;         // a fifth slab came: the set was emptied and the next frame restarts
    bool slab_boxes_drawn = false;      // the frame drawn last placed boxes (rt_read_slab_boxes reads them)

    // ray queries (rt_trace_rays, rt_pick_pixels): a stream of their own (the device's highest priority), so that a query waits for
    // the world changes before it (ev_world) and not for the frames; the world changes wait for the queries before them (ev_query)
    hipStream_t query_stream = nullptr;
    rta::LatchEvent ev_world, ev_query;
    rta::StagingBlock query_block;   // the synchronous calls' pinned and device staging (inputs, then hits), grown on demand
    // rt_draw_stamps[_async]: the models' device records (and the synchronous call's face lights).  The asynchronous call returns
    // before its transfer has run, so the records cannot share query_block with the synchronous queries: two sets used in turn, as
    // for the edits (call n waits for the transfer of call n - 2 to leave the host block and for its launch to leave the device block)
    rta::StagingSet draw_sets[2];
    uint64_t draw_batches = 0;
    // the most recent rt_stamp_capture: its launch writes a stamp's arrays on the render stream, where the draws and the shadows read
    // them in stream order; an entity query reads them on the query stream and waits for this first
    rta::LatchEvent ev_capture;
    // light probes (rt_probe_light): the path records of a launch whose samples one workgroup cannot add itself (16 bytes per path),
    // grown on demand up to kProbeScratchBytes, in c->allocs (device_bytes; freed by rt_destroy)
    float4* probe_scratch = nullptr;
    size_t probe_scratch_bytes = 0;
    bool probe_pair = true;          // RT_PROBE_PAIR=0: the plain form of k_probe (A/B timing)
    // rt_draw_particles[_async]: the binning scratch (rtd::particle_scratch_words of the call's count and the frame), grown on demand
    // and never shrunk, in c->allocs (device_bytes; freed by rt_destroy).  One block serves every call: a call's launches follow the
    // previous call's (ev_particles) wherever the frames' streams have taken them.
    uint32_t* particle_scratch = nullptr;
    size_t particle_scratch_words = 0;
    rta::LatchEvent ev_particles;
    // rt_emit_particles[_async]: the masks and particle numbers of a call's items (rtd::emit_scratch_words), grown on demand and never
    // shrunk, in c->allocs (device_bytes; freed by rt_destroy), handled as the particle scratch is: a call's launches follow the
    // previous call's (ev_emit) when the stream has changed between them.
    uint32_t* emit_scratch = nullptr;
    size_t emit_scratch_words = 0;
    rta::LatchEvent ev_emit;
    // rt_deposit_particles[_async]: a claim word per texel of the clipped box, a flag word per chunk of it and a spare count record
    // (rtd::deposit_scratch_words; at most 64 MiB and a little), grown on demand and never shrunk, in c->allocs (device_bytes; freed by
    // rt_destroy).  Every call uses it on the render stream or behind a lane join, so its launches follow the previous call's.
    // rt_settle_voxels[_async] keeps its flag words and spare count record (rtd::settle_scratch_words) in the same block, the same way.
    uint32_t* deposit_scratch = nullptr;
    size_t deposit_scratch_words = 0;
    rta::LatchEvent ev_deposit;
    // rt_detach_voxels[_async]: the pass record, a spare result record, a flag word per chunk of the clipped box and three bitmaps of
    // 32 KiB per chunk — occupancy and two reach buffers (rtd::detach_scratch_words; at most 125 chunks: 12 MiB), grown on demand and
    // never shrunk, in c->allocs (device_bytes; freed by rt_destroy), handled as the deposits' block is.
    uint32_t* detach_scratch = nullptr;
    size_t detach_scratch_words = 0;
    rta::LatchEvent ev_detach;
    // rt_flow_voxels[_async]: the head (a word per tick launch, a spare count record, a flag word per chunk of the clipped box) and two
    // state arrays of a byte per cell of the box (rtd::flow_scratch_words; at most 2 x 256^3 bytes and the head), grown on demand and
    // never shrunk, in c->allocs (device_bytes; freed by rt_destroy), handled as the deposits' block is.
    uint32_t* flow_scratch = nullptr;
    size_t flow_scratch_words = 0;
    rta::LatchEvent ev_flow;
    uint32_t flow_group = 4;         // G, ticks per launch; RT_FLOW_TICKS = 1, 2, 4 or 8 when the context first plans a flow call (A/B timing)
    bool flow_planned = false;
};

namespace rta __attribute__((visibility("hidden"))) {

extern thread_local std::string g_create_error;   // rt_last_error(NULL): why the last rt_create of this thread failed

// What restarts the accumulation / the history outright (uploads, generated terrain, new noise, rt_reset_accumulation): the next
// frame starts from zero, and edit boxes and slabs still waiting for it mean nothing any more.
inline void restart_history(RtContext* c) {
    c->accum_valid = false;
    c->edit_nbox = 0;
    c->edit_overflow = false;
    c->slab_pending = 0;
    c->slab_overflow = false;
}

inline int fail(RtContext* c, int code, const std::string& msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

#define RT_HIP(ctx, call)                                                                             \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return rta::fail(ctx, e_ == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP,                \
                             std::string(#call) + ": " + hipGetErrorString(e_));                      \
    } while (0)

template <typename T>
hipError_t dev_alloc(RtContext* c, T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    hipError_t e = hipMalloc((void**)p, count * sizeof(T));
    if (e == hipSuccess) { c->allocs.push_back((void*)*p); c->device_bytes += count * sizeof(T); }
    return e;
}

// Every stream and event of the context is made here and destroyed by rt_destroy, which knows them by these lists alone.
inline hipError_t new_event(RtContext* c, hipEvent_t* ev, unsigned flags = hipEventDisableTiming) {
    const hipError_t e = hipEventCreateWithFlags(ev, flags);
    if (e == hipSuccess) c->events.push_back(*ev);
    return e;
}
// (non-blocking; `priority` for one of that stream priority)
inline hipError_t new_stream(RtContext* c, hipStream_t* st, const int* priority = nullptr) {
    const hipError_t e = priority ? hipStreamCreateWithPriority(st, hipStreamNonBlocking, *priority) : hipStreamCreateWithFlags(st, hipStreamNonBlocking);
    if (e == hipSuccess) c->streams.push_back(*st);
    return e;
}

inline hipError_t StagingBlock::grow(RtContext* c, size_t need, size_t alloc) {
    if (need <= cap) return hipSuccess;
    if (dev) c->device_bytes -= cap;
    release();
    hipError_t e = hipHostMalloc((void**)&host, alloc, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&dev, alloc);
    if (e == hipSuccess) { cap = alloc; c->device_bytes += alloc; }
    return e;
}
inline void StagingBlock::release() {
    if (host) { (void)hipHostFree(host); host = nullptr; }
    if (dev) { (void)hipFree(dev); dev = nullptr; }
    cap = 0;
}

// What a staging pair that must hold `need` bytes is allocated with when it has to grow: 64 KiB at least, else half as much again.
inline size_t staging_alloc(size_t need) { return need < ((size_t)64 << 10) ? ((size_t)64 << 10) : align16(need + need / 2u); }

// ---- the hand-over of a staging set (StagingSet): claim, fill the host block, send, launch on `reader`, record ev_applied there ------
// The host may write `need` bytes to the set: its previous transfer has left the host block; a smaller set is replaced by one of
// `alloc` bytes once the launch that reads its device block has run.  (The upload stream and the set's events are made on first use.)
inline hipError_t staging_claim(RtContext* c, StagingSet& s, size_t need, size_t alloc) {
    hipError_t e = c->upload_stream ? hipSuccess : new_stream(c, &c->upload_stream);
    for (hipEvent_t* ev : {&s.ev_copied.ev, &s.ev_applied.ev})
        if (e == hipSuccess && !*ev) e = new_event(c, ev);
    if (e == hipSuccess) e = s.ev_copied.host_wait();
    if (e == hipSuccess) s.ev_copied.forget();
    if (e != hipSuccess || need <= s.cap) return e;
    e = s.ev_applied.host_wait();
    if (e == hipSuccess) s.ev_applied.forget();
    return e == hipSuccess ? s.grow(c, need, alloc) : e;
}
// The first `bytes` of the host block to the device block on the upload stream (so that the transfer does not queue behind a frame),
// after the set's previous launch has read it; `reader`, the stream whose launch will read the device block, waits for the transfer.
inline hipError_t staging_send(RtContext* c, StagingSet& s, size_t bytes, hipStream_t reader) {
    hipError_t e = s.ev_applied.wait(c->upload_stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.dev, s.host, bytes, hipMemcpyHostToDevice, c->upload_stream);
    if (e == hipSuccess) e = s.ev_copied.record(c->upload_stream);
    return e == hipSuccess ? hipStreamWaitEvent(reader, s.ev_copied.ev, 0) : e;
}

// One part of a synchronous call's staging: `bytes` copied from `host`, or (host == nullptr) room for what the launch leaves there.
struct StagePart { const void* host; size_t bytes; };
// The parts of a synchronous call through query_block, back to back and each on a 16-byte boundary: the host parts (they come first)
// into the pinned half and from there to the device half in one transfer on `st`; dev[i] is part i's device address.  (The previous
// synchronous call has finished with the block: it waited for its launch or its results.)
inline int stage_sync(RtContext* c, hipStream_t st, std::initializer_list<StagePart> parts, uint8_t** dev) {
    StagingBlock& q = c->query_block;
    size_t need = 0, send = 0;
    for (const StagePart& p : parts) { need = align16(need) + p.bytes; if (p.host) send = need; }
    RT_HIP(c, q.grow(c, need, staging_alloc(need)));
    size_t off = 0;
    for (const StagePart& p : parts) {
        off = align16(off);
        *dev++ = q.dev + off;
        if (p.host) memcpy(q.host + off, p.host, p.bytes);
        off += p.bytes;
    }
    RT_HIP(c, hipMemcpyAsync(q.dev, q.host, send, hipMemcpyHostToDevice, st));
    return RT_OK;
}

// At least `words` words in a scratch block that grows on demand and is never shrunk (*block of *have words, in c->allocs and counted in
// device_bytes).  `users`: recorded behind the launches that use the block; a block that must grow waits for them before it is freed.
inline int scratch_reserve(RtContext* c, uint32_t** block, size_t* have, LatchEvent* users, size_t words) {
    if (!users->ev) RT_HIP(c, new_event(c, &users->ev));
    if (words <= *have) return RT_OK;
    if (*block) {
        RT_HIP(c, users->host_wait());
        users->forget();
        for (size_t i = 0; i < c->allocs.size(); i++)
            if (c->allocs[i] == *block) { c->allocs.erase(c->allocs.begin() + (long)i); break; }
        (void)hipFree(*block);
        c->device_bytes -= *have * sizeof(uint32_t);
        *block = nullptr;
        *have = 0;
    }
    RT_HIP(c, dev_alloc(c, block, words));
    *have = words;
    return RT_OK;
}
// rt_draw_particles' binning scratch, rt_emit_particles' masks and particle numbers and rt_deposit_particles' claims and flags
inline int particle_scratch_reserve(RtContext* c, size_t words) {
    return scratch_reserve(c, &c->particle_scratch, &c->particle_scratch_words, &c->ev_particles, words);
}
inline int emit_scratch_reserve(RtContext* c, size_t words) { return scratch_reserve(c, &c->emit_scratch, &c->emit_scratch_words, &c->ev_emit, words); }
inline int deposit_scratch_reserve(RtContext* c, size_t words) {
    return scratch_reserve(c, &c->deposit_scratch, &c->deposit_scratch_words, &c->ev_deposit, words);
}
inline int detach_scratch_reserve(RtContext* c, size_t words) {
    return scratch_reserve(c, &c->detach_scratch, &c->detach_scratch_words, &c->ev_detach, words);
}
inline int flow_scratch_reserve(RtContext* c, size_t words) { return scratch_reserve(c, &c->flow_scratch, &c->flow_scratch_words, &c->ev_flow, words); }

// An environment knob (experiments, A/B timing): *field = v when `s` holds an integer in lo..hi; anything else is ignored.
template <typename T>
bool parse_knob(const char* s, long long lo, long long hi, T* field) {
    if (!s) return false;
    const long long v = atoll(s);
    if (v < lo || v > hi) return false;
    *field = (T)v;
    return true;
}
template <typename T>
bool env_int(const char* name, long long lo, long long hi, T* field) { return parse_knob(getenv(name), lo, hi, field); }

// Event pair bracketing one launch (only with RT_FLAG_TIMING), recorded on the stream the launch goes to.
struct LaunchTimer {
    RtContext* c; bool on; size_t idx; hipStream_t st;
    // kind 0 = traversal kernel (RT_FLAG_TIMING), 1 = any other launch (RT_FLAG_TIMING_ALL: each pair of events costs a few us)
    LaunchTimer(RtContext* ctx, int kind, hipStream_t stream = nullptr)
        : c(ctx), on(kind == 0 ? (ctx->cfg.flags & RT_FLAG_TIMING) != 0 : (ctx->cfg.flags & RT_FLAG_TIMING_ALL) == RT_FLAG_TIMING_ALL), idx(0),
          st(stream ? stream : ctx->stream) {
        if (!on) return;
        hipError_t e;
        idx = c->launch_times.acquire(st, &e);
        if (idx == TimingPool::npos) { if (e == hipSuccess) c->timer_overflow++; on = false; return; }
        if (c->launch_kind.size() <= idx / 2) c->launch_kind.resize(idx / 2 + 1);
        c->launch_kind[idx / 2] = kind;
    }
    ~LaunchTimer() { if (on) (void)c->launch_times.release(idx, st); }
};

// ---- what crosses the files (api_context.hip; the last two api_frame.hip) -------------------------------------------------------
hipError_t join_lanes_into(RtContext* c, hipStream_t st);
hipError_t fence_lanes_after(RtContext* c, hipStream_t st);
hipError_t sync_lanes(RtContext* c);
void invalidate_prepass(RtContext* c);
void plane_written(RtContext* c, const void* ptr);
rtd::Scene scene_of(const RtContext* c);
rtd::Planes planes_of(void* const* planes);
inline rtd::Planes planes_of(const RtContext* c) { return planes_of(c->planes); }
void resolve_route(RtContext* c);
rtd::Frame frame_of(const RtContext* c, const RtUniforms* u);
bool query_device_ptr(const RtContext* c, const void* p);   // api_query.hip: rt_trace_rays_async's test of a caller's device pointer
// api_passes.hip: the verdict on a batch of models, and their way to the device for the launch `reader` will run (the entity draws,
// the entity shadows, the entity queries and sweeps and the emitters share both)
int models_check(RtContext* c, const std::string& fn, const RtDrawStamp* models, uint32_t n, const char* nothing);
// What upload_models hands the launch: the staging set in use and its device block.  An entity set's models are optional: with none
// (models_send) the batch is empty, recs() is null and applied() records nothing.
struct ModelBatch {
    StagingSet* set = nullptr;
    uint8_t* dev = nullptr;
    const uint4* recs() const { return reinterpret_cast<const uint4*>(dev); }
    // behind the launch on `reader`: the set's next transfer and rt_stamp_destroy wait for it
    hipError_t applied(hipStream_t reader) { return set ? set->ev_applied.record(reader) : hipSuccess; }
};
int upload_models(RtContext* c, const RtDrawStamp* models, uint32_t n, const void* extra_host, size_t extra_bytes, hipStream_t reader, ModelBatch* batch);
int models_send(RtContext* c, const RtDrawStamp* models, uint32_t n, hipStream_t reader, ModelBatch* batch);

}  // namespace rta
