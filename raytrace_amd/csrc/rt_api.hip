// rt_api.hip — implementation of the C ABI in include/rt_abi.h on top of the kernels in rt_kernels.hip.
//
// One context = one GPU = one HIP stream.  Nothing here runs ray-trace work on the CPU: if the HIP runtime or a
// device is missing, rt_create fails with RT_ERR_NO_DEVICE and the caller gets no context.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: the library is dlopen'ed on first use (rt_comm_* / rt_gather_gbuffer)

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/rt_abi.h"
#include "../../include/rt_math.h"
#include "rt_kernels.hpp"

namespace {

thread_local std::string g_create_error = "";


const size_t kBytesPerPixel[RT_BUF_COUNT] = {8, 2, 1, 4, 4, 4, 16, 16, 4, 4};

}  // namespace

constexpr size_t kWlSetWords = 64, kWlClearWords = 33;   // FrameSlot::wl_count: words of one set, and those of it that are in use
constexpr size_t kCursorWords = 8 * 32;   // path cursors of the persistent kernels: one word per XCD group, each on its own 128-byte line
// light records of one launch above which k_paths streams them out and k_accumulate_paths streams them in (see draw_path_batches)
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

struct Route {
    int family = RT_KERNEL_PERSISTENT;   // RT_KERNEL_MEGA, RT_KERNEL_WAVEFRONT, or RT_KERNEL_PERSISTENT (k_frame, k_persist and k_paths)
    bool frame = false;                  // every frame is one k_frame launch
    uint32_t paths_from = UINT32_MAX;    // path launches of at least this many samples run on k_paths, smaller ones on k_persist
    uint32_t threshold_persist = 0, threshold_paths = 0;   // PersistArgs::threshold of a k_persist / k_paths launch
    bool direct = false;                 // one-sample launches store the pixel's lighting themselves: no light records, no accumulate
    int in_use = RT_KERNEL_PERSISTENT;   // rt_kernel_in_use: the kernel of a frame's last launch
    bool on_paths(uint32_t ns) const { return ns >= paths_from; }
};

// Pinned host staging -> device twin (upload stream) -> the launch that applies it (render stream): rt_upload_slice's slabs and
// rt_edit_voxels' batches.  Each kind has TWO sets used in turn: transfer n waits for the launch of n - 2, not of n - 1,
// which sits behind the frames on the render stream — a host that sends one slab or batch per frame never waits for a frame.
struct StagingSet {
    uint8_t* host = nullptr;           // hipHostMalloc
    uint8_t* dev = nullptr;            // hipMalloc (counted in device_bytes)
    size_t cap = 0;                    // bytes of each block
    hipEvent_t ev_copied = nullptr;    // the transfer has read the host block
    hipEvent_t ev_applied = nullptr;   // the launch has read the device block
    bool copy_pending = false, apply_recorded = false;
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
    hipEvent_t ev_tail = nullptr;      // everything submitted for the frame in this slot: the slot's next frame starts after it
    bool tail_recorded = false;
};

struct RtContext {
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

    // scene
    // (the caller-layout copy of the region exists only inside rt_upload_world: 5 B/voxel, 5 GiB at R = 1024)
    uint8_t* d_mine_sw = nullptr; uint32_t* d_mat_sw = nullptr;
    uint32_t* d_coarse = nullptr; uint32_t* d_noise = nullptr; uint32_t* d_flag = nullptr;
    uint32_t* d_brick = nullptr;          // R > 256: per-brick nibble map (rtd::Scene::brick), R^3 / 128 bytes
    // staging (StagingSet): rt_upload_slice's 16-thick slab (materials, then minefield at 4 x 16 R^2) is re-tiled, rt_edit_voxels'
    // binned batch (touched chunks, per-chunk edit ranges, records) rebuilds its chunks; the edit sets grow when a batch needs more
    hipStream_t upload_stream = nullptr;
    StagingSet slab_sets[2], edit_sets[2];
    uint64_t slabs = 0, edit_batches = 0;   // submitted so far: the next one uses set slabs & 1 / edit_batches & 1
    std::vector<uint32_t> edit_chunk, edit_order, edit_start, edit_stamp;   // host binning scratch, kept between calls
    uint32_t edit_gen = 0;                // edit_stamp generation: a voxel's slot holds the generation of the chunk run that kept it
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
    Lane lanes[2];
    int nlanes = 1;                     // 2: path launches alternate between two streams (persistent kernels on the context's own stream)
    FrameSlot slots[2];
    int nslots = 1;                     // 2 with RT_FLAG_FRAMES_IN_FLIGHT_2
    int cur_slot = 0;                   // slot of the frame drawn last
    uint64_t frames_drawn = 0, path_launches = 0;
    hipEvent_t ev_fence = nullptr;      // fence_lanes_after
    hipEvent_t ev_gather = nullptr;     // the previous rt_gather_gbuffer (gathers share staging: they run one after the other)
    bool gather_recorded = false;

    Route route;

    // wavefront pipeline state
    uint32_t batch_samples = 1;   // samples per batch
    uint32_t cap = 0;             // paths per batch (allocation)
    uint32_t refill_threshold = 24;
    float *qox = nullptr, *qoy = nullptr, *qoz = nullptr, *qdx = nullptr, *qdy = nullptr, *qdz = nullptr;
    uint32_t* qid = nullptr;
    float *hx = nullptr, *hy = nullptr, *hz = nullptr;
    uint32_t* hinfo = nullptr;
    uint8_t *sunres = nullptr, *pnormal = nullptr, *pstate = nullptr;
    float *pdx = nullptr, *pdy = nullptr, *pdz = nullptr, *plx = nullptr, *ply = nullptr, *plz = nullptr;
    uint32_t *sunbits = nullptr, *stack = nullptr;
    float4* acc = nullptr;
    uint32_t* ctrl = nullptr;     // per batch: [RT_MAX_DEPTH+2] pair counts, then [RT_MAX_DEPTH+2] cursors
    // persistent kernel state (per-launch and per-frame buffers live in the lanes and slots above)
    float4* sphere_lut = nullptr;
    float4* sun_lut = nullptr;
    float4* dif_lut = nullptr;
    uint32_t persist_batch = 1;
    int pl_stream_mode = -1;      // RT_PL_STREAM: -1 = by size (kStreamRecordBytes); bit 0 streaming stores, bit 1 streaming loads
    uint32_t persist_chunk = 0;   // RT_PERSIST_CHUNK: paths per cursor atomic (multiple of 64); 0 = automatic
    uint32_t persist_threshold = 0, persist_rmin = 12;   // RT_PERSIST_THRESHOLD: 0 = the route's default per kernel
    uint64_t frame_crossover = kFrameCrossover;
    uint64_t frame_crossover_multi = kFrameCrossoverMulti;   // ... and frames of more than one sample per pixel below this many pixel-sample-levels
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
    std::vector<hipEvent_t> ev_pool;
    std::vector<int> ev_kind;     // per (start,stop) pair: 0 = trace, 1 = other
    size_t ev_used = 0;
    bool frame_recorded = false;
    uint64_t rays_bound = 0;

    // multi-GPU gather (rt_gather_gbuffer): root's staging for the ranks' blocks; the overlapped mode's second stream,
    // two send-side staging copies of this rank's block and the events that order them
    void* frame_planes[6] = {};   // root, frames_dev == NULL: the library's own row-major full-frame planes (rt_frame_ptr)
    uint8_t* gathered[2] = {nullptr, nullptr};
    uint8_t* stage[2] = {nullptr, nullptr};
    hipStream_t gather_stream = nullptr;
    hipEvent_t ev_ready[2] = {nullptr, nullptr}, ev_free[2] = {nullptr, nullptr};
    bool ev_free_recorded[2] = {false, false};
    uint64_t gathers = 0;
    uint32_t timer_overflow = 0;   // launches that found the event pool full (RT_FLAG_TIMING without rt_get_timing)
    std::vector<hipEvent_t> gather_ev;   // RT_FLAG_TIMING: (start, stop) pairs round the rt_gather_gbuffer calls (rt_get_gather_timing)
    size_t gather_ev_used = 0;

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
    hipEvent_t ev_accum = nullptr;      // the last step of the frame drawn last that touched d_accum (two lanes only) ...
    hipStream_t accum_stream = nullptr; // ... recorded on this stream
    bool accum_recorded = false;
    // temporal reprojection (RT_FLAG_REPROJECT): two history sets used in turn — a frame's pass reads the set the previous frame's
    // pass wrote and writes the other.  Sums by row-major pixel (set 0's is d_accum) and (depth_f32 bits, count | normal << 27)
    // records; the previous frame's camera is accum_key's origin, forward, up and right
    bool reproject = false;
    uint32_t history_cap = 32;
    float4* d_hist_sum[2] = {nullptr, nullptr};
    uint2* d_hist_rec[2] = {nullptr, nullptr};
    int hist_cur = 0;                   // the set the pass of the frame drawn last wrote

    // ray queries (rt_trace_rays, rt_pick_pixels): a stream of their own (the device's highest priority), so that a query waits for
    // the world changes before it (ev_world) and not for the frames; the world changes wait for the queries before them (ev_query)
    hipStream_t query_stream = nullptr;
    hipEvent_t ev_world = nullptr, ev_query = nullptr;
    bool world_recorded = false, query_recorded = false;
    uint8_t *q_host = nullptr, *q_dev = nullptr;   // the synchronous calls' pinned and device staging (inputs, then hits), grown on demand
    size_t q_cap = 0;
};

constexpr size_t kMaxTimerEvents = 2 * 4096;   // LaunchTimer pool cap: pairs beyond it are not timed (counted in timer_overflow)

namespace {

int fail(RtContext* c, int code, const std::string& msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

#define RT_HIP(ctx, call)                                                                             \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail(ctx, e_ == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP,                     \
                        std::string(#call) + ": " + hipGetErrorString(e_));                           \
    } while (0)

template <typename T>
hipError_t dev_alloc(RtContext* c, T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    hipError_t e = hipMalloc((void**)p, count * sizeof(T));
    if (e == hipSuccess) { c->allocs.push_back((void*)*p); c->device_bytes += count * sizeof(T); }
    return e;
}

// Every input to the route is fixed when the context is created (kernel, primary cache, accumulation, spp, depth, region, frame size,
// samples per launch and the crossover knobs), so rt_create decides it once, after persist_batch; rt_draw_frame, rt_kernel_in_use
// and rt_get_info read the result.  The baselines run their own kernel.
void resolve_route(RtContext* c) {
    Route& r = c->route;
    if (r.family != RT_KERNEL_PERSISTENT) { r.in_use = r.family; return; }
    const RtConfig& cfg = c->cfg;
    const int kernel = cfg.kernel;
    const bool cache = (cfg.flags & RT_FLAG_CACHE_PRIMARY) != 0;
    const uint32_t spp = (uint32_t)cfg.spp, B = c->persist_batch;
    const uint64_t npix = c->npix_pad;
    rtd::Frame f{};   // (launch_frame_ok and launch_paths_direct_ok read depth and logr only)
    f.depth = cfg.depth; f.logr = c->logr;
    // k_frame takes whatever it covers of RT_KERNEL_FRAME and the small frames of RT_KERNEL_DEFAULT.  It caches primaries by
    // construction (with one sample per pixel every kernel does: the flag is not needed); more samples than one need the whole
    // frame's light records in one lane's array; and it adds a pixel's samples from 0, so an accumulating frame of more than one
    // sample continues the running sum on the persistent kernels instead.
    const bool small = spp == 1u ? npix < c->frame_crossover
                                 : npix * spp * (uint64_t)(cfg.depth > 1 ? cfg.depth : 1) < c->frame_crossover_multi;
    r.frame = (cache || spp == 1u) && rtd::launch_frame_ok(f) && spp <= B && !((cfg.flags & RT_FLAG_ACCUMULATE) && spp > 1u) &&
              (kernel == RT_KERNEL_FRAME || (kernel == RT_KERNEL_DEFAULT && small));
    // k_paths needs cached primaries; RT_KERNEL_DEFAULT gives it the launches of at least kPathsCrossover pixel-samples
    if (cache && kernel != RT_KERNEL_PERSISTENT)
        r.paths_from = kernel != RT_KERNEL_DEFAULT ? 0u : npix == 0 ? UINT32_MAX : (uint32_t)((kPathsCrossover + npix - 1) / npix);
    // one sample per pixel (the reference's own frames): k_persist and k_paths store the pixel's lighting themselves, no light
    // records and no accumulate launch (raytrace.comp:352-356 has no accumulation either)
    r.direct = spp == 1u && (!r.on_paths(1) || rtd::launch_paths_direct_ok(f));
    // parked lanes that trigger a pass (RT_PERSIST_THRESHOLD overrides): measured optima per kernel.  k_persist 32.  k_paths (lanes
    // with a parked context, three steps between looks), round 3, same box: 24 4.28 ms per headline launch, 28 4.22, 32 4.17, 36
    // 4.06-4.15, 40 4.08-4.14, 44 4.12, 48 4.27; deeper frames at region 256 (depth 5..8: longer paths, fewer new ones per pass) like
    // 40 — 3840x2160 spp 256 depth 8 launch 51.2 ms at 28, 50.7 at 32, 50.0 at 36, 49.6 at 40 and 44 —, the 1024^3 frame stays at 36
    // (20.74 against 20.86 at 40, 21.2 at 44)
    r.threshold_persist = c->persist_threshold ? c->persist_threshold : 32u;
    r.threshold_paths = c->persist_threshold ? c->persist_threshold : (cfg.depth > 4 && c->region == 256) ? 40u : 36u;
    // the last launch of a frame covers the samples left after the full batches; a cached frame of depth 0 is its prepass alone
    // and reports the kernel the configuration names
    if (r.frame) r.in_use = RT_KERNEL_FRAME;
    else if (cache && cfg.depth == 0) r.in_use = kernel == RT_KERNEL_PERSISTENT ? RT_KERNEL_PERSISTENT : RT_KERNEL_PATHS;
    else r.in_use = r.on_paths((spp - 1u) % B + 1u) ? RT_KERNEL_PATHS : RT_KERNEL_PERSISTENT;
}

rtd::Scene scene_of(const RtContext* c) {
    rtd::Scene s;
    s.mine = c->d_mine_sw; s.mat = c->d_mat_sw; s.coarse = c->d_coarse; s.noise = c->d_noise;
    s.brick = c->d_brick ? reinterpret_cast<const uint8_t*>(c->d_brick) : reinterpret_cast<const uint8_t*>(c->d_coarse);
    return s;
}

rtd::Planes planes_of(void* const* planes) {
    rtd::Planes p;
    p.lighting_rgba16 = (uint16_t*)planes[RT_BUF_LIGHTING_RGBA16];
    p.depth_r16 = (uint16_t*)planes[RT_BUF_DEPTH_R16UI];
    p.normal_r8 = (uint8_t*)planes[RT_BUF_NORMAL_R8UI];
    p.albedo_rgba8 = (uint32_t*)planes[RT_BUF_ALBEDO_RGBA8];
    p.emission_rgba8 = (uint32_t*)planes[RT_BUF_EMISSION_RGBA8];
    p.fog_rgba8 = (uint32_t*)planes[RT_BUF_FOG_RGBA8];
    p.lighting_f32 = (float*)planes[RT_BUF_LIGHTING_F32];
    p.fog_f32 = (float*)planes[RT_BUF_FOG_F32];
    p.depth_f32 = (float*)planes[RT_BUF_DEPTH_F32];
    return p;
}
rtd::Planes planes_of(const RtContext* c) { return planes_of(c->planes); }

// raytrace.comp:317-318 — uniform over the frame, so evaluated once here with the same rt_math.h the kernels use.
void sun_constants(float a, float* sunangle, float* sunlight) {
    float s, c;
    rtm_sincos(a, &s, &c);
    rtm_vec3 v = rtm_normalize3({c * 0.5f + (a - 0.5f) * 0.5f, s, c});
    sunangle[0] = v.x; sunangle[1] = v.y; sunangle[2] = v.z;
    // sun_color, raytrace.comp:259-269
    float horizon = rtm_length2(v.x, v.y);
    float sun_amount = rtm_min(1.0f - horizon, 0.02f) * 50.0f;
    const float main_color[3] = {0.9647f * 2.0f, 0.7843f * 2.0f, 0.8824f * 2.0f};
    const float sunset_color[3] = {0.7412f * 2.0f, 0.2157f * 2.0f, 0.1686f * 2.0f};
    for (int k = 0; k < 3; k++)
        sunlight[k] = v.z >= 0.0f ? rtm_mix(sunset_color[k], main_color[k], sun_amount)
                                  : rtm_mix(sunset_color[k], 0.0f, sun_amount * 2);
}

// RT_FLAG_ACCUMULATE: the uniforms a frame continues the accumulation under — every live field but seed, bit for bit
void accum_key_of(const RtUniforms* u, uint32_t key[16]) {
    memcpy(&key[0], &u->sun_angle, 4);
    memcpy(&key[1], u->origin, 12); memcpy(&key[4], u->forward, 12); memcpy(&key[7], u->up, 12); memcpy(&key[10], u->right, 12);
    memcpy(&key[13], u->lr, 12);
}

rtd::Frame frame_of(const RtContext* c, const RtUniforms* u) {
    rtd::Frame f;
    for (int k = 0; k < 3; k++) {
        f.origin[k] = u->origin[k]; f.forward[k] = u->forward[k]; f.up[k] = u->up[k]; f.right[k] = u->right[k];
        f.lr[k] = (float)u->lr[k];    // vec3 current_rotation = uniform_data.lr (raytrace.comp:104)
    }
    sun_constants(u->sun_angle, f.sunangle, f.sunlight);
    f.seed = u->seed;
    f.width = c->cfg.width; f.height = c->cfg.height;
    f.tiles_x = c->tiles_x; f.tiles_y = c->tiles_y;
    f.tile_rank = c->cfg.tile_rank; f.tile_world = c->cfg.tile_world;
    f.ntiles_local = c->ntiles_local;
    f.spp = c->cfg.spp; f.depth = c->cfg.depth;
    f.lr_zero = (u->lr[0] == 0 && u->lr[1] == 0 && u->lr[2] == 0) ? 1 : 0;
    f.logr = c->logr;
    f.region = (float)c->region;
    return f;
}

// Event pair bracketing one launch (only with RT_FLAG_TIMING), recorded on the stream the launch goes to.
struct LaunchTimer {
    RtContext* c; bool on; size_t idx; hipStream_t st;
    // kind 0 = traversal kernel (RT_FLAG_TIMING), 1 = any other launch (RT_FLAG_TIMING_ALL: each pair of events costs a few us)
    LaunchTimer(RtContext* ctx, int kind, hipStream_t stream = nullptr)
        : c(ctx), on(kind == 0 ? (ctx->cfg.flags & RT_FLAG_TIMING) != 0 : (ctx->cfg.flags & RT_FLAG_TIMING_ALL) == RT_FLAG_TIMING_ALL), idx(0),
          st(stream ? stream : ctx->stream) {
        if (!on) return;
        if (c->ev_used + 2 > kMaxTimerEvents) { c->timer_overflow++; on = false; return; }
        if (c->ev_used + 2 > c->ev_pool.size()) {
            for (int k = 0; k < 2; k++) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) { on = false; return; } c->ev_pool.push_back(e); }
        }
        idx = c->ev_used; c->ev_used += 2;
        if (c->ev_kind.size() < c->ev_used / 2) c->ev_kind.resize(c->ev_used / 2);
        c->ev_kind[idx / 2] = kind;
        (void)hipEventRecord(c->ev_pool[idx], st);
    }
    ~LaunchTimer() { if (on) (void)hipEventRecord(c->ev_pool[idx + 1], st); }
};

// ---- lanes (round 4): ordering between the library's streams, all on the device -------------------------------------------
// `st` waits for everything submitted so far on the other lanes (and on the stream the last frame ended on)
hipError_t join_lanes_into(RtContext* c, hipStream_t st) {
    for (int l = 0; l < c->nlanes; l++) {
        Lane& ln = c->lanes[l];
        if (ln.stream == st || !ln.stream) continue;
        hipError_t e = hipEventRecord(ln.ev_join, ln.stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, ln.ev_join, 0);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
// ... and the other lanes wait for what `st` holds now
hipError_t fence_lanes_after(RtContext* c, hipStream_t st) {
    if (c->nlanes < 2) return hipSuccess;
    hipError_t e = hipEventRecord(c->ev_fence, st);
    for (int l = 0; l < c->nlanes && e == hipSuccess; l++)
        if (c->lanes[l].stream != st) e = hipStreamWaitEvent(c->lanes[l].stream, c->ev_fence, 0);
    return e;
}
// host-side wait for every stream of the context that renders
hipError_t sync_lanes(RtContext* c) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && c->query_stream) e = hipStreamSynchronize(c->query_stream);
    for (int l = 0; l < c->nlanes && e == hipSuccess; l++)
        if (c->lanes[l].stream && c->lanes[l].stream != c->stream) e = hipStreamSynchronize(c->lanes[l].stream);
    return e;
}

// ---- a change of the resident world on the render stream (slabs, edits, generated terrain) ---------------------------------------
// before its launches: they wait for the frames in flight on every lane and for the queries recorded so far (both read the region)
hipError_t world_change_begin(RtContext* c) {
    hipError_t e = join_lanes_into(c, c->stream);
    if (e == hipSuccess && c->query_recorded) e = hipStreamWaitEvent(c->stream, c->ev_query, 0);
    return e;
}
// after them: later queries (ev_world) and later frames, whichever lane they start on, see what changed
hipError_t world_change_end(RtContext* c) {
    if (c->ev_world) {
        hipError_t e = hipEventRecord(c->ev_world, c->stream);
        if (e != hipSuccess) return e;
        c->world_recorded = true;
    }
    return fence_lanes_after(c, c->stream);
}

// ---- staging (StagingSet) ---------------------------------------------------------------------------------------------------
// the upload stream and the set's events, created on first use
hipError_t staging_create(RtContext* c, StagingSet& s) {
    hipError_t e = hipSuccess;
    if (!c->upload_stream) e = hipStreamCreateWithFlags(&c->upload_stream, hipStreamNonBlocking);
    for (hipEvent_t* ev : {&s.ev_copied, &s.ev_applied})
        if (e == hipSuccess && !*ev) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    return e;
}
// the host may write `need` bytes to the set: its previous transfer has left the host block; a smaller set is replaced by one of
// `alloc` bytes once its device block has been applied
hipError_t staging_claim(RtContext* c, StagingSet& s, size_t need, size_t alloc) {
    hipError_t e = staging_create(c, s);
    if (e == hipSuccess && s.copy_pending) { e = hipEventSynchronize(s.ev_copied); if (e == hipSuccess) s.copy_pending = false; }
    if (e != hipSuccess || need <= s.cap) return e;
    if (s.apply_recorded) e = hipEventSynchronize(s.ev_applied);
    if (e != hipSuccess) return e;
    if (s.host) { (void)hipHostFree(s.host); s.host = nullptr; }
    if (s.dev) { (void)hipFree(s.dev); s.dev = nullptr; c->device_bytes -= s.cap; }
    s.cap = 0;
    e = hipHostMalloc((void**)&s.host, alloc, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&s.dev, alloc);
    if (e == hipSuccess) { s.cap = alloc; c->device_bytes += alloc; }
    return e;
}
// the first `bytes` of the host block to the device block on the upload stream, after the set's previous launch has read it; the
// render stream waits for the transfer, and for the frames in flight on the other lane (they read what the launch changes)
hipError_t staging_send(RtContext* c, StagingSet& s, size_t bytes) {
    hipError_t e = s.apply_recorded ? hipStreamWaitEvent(c->upload_stream, s.ev_applied, 0) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpyAsync(s.dev, s.host, bytes, hipMemcpyHostToDevice, c->upload_stream);
    if (e == hipSuccess) e = hipEventRecord(s.ev_copied, c->upload_stream);
    if (e != hipSuccess) return e;
    s.copy_pending = true;
    e = hipStreamWaitEvent(c->stream, s.ev_copied, 0);
    return e == hipSuccess ? world_change_begin(c) : e;
}
// after the launch that read the device block: later frames, whichever lane they start on, see what it changed
hipError_t staging_applied(RtContext* c, StagingSet& s) {
    hipError_t e = hipEventRecord(s.ev_applied, c->stream);
    if (e != hipSuccess) return e;
    s.apply_recorded = true;
    return world_change_end(c);
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

int draw_wavefront(RtContext* c, const rtd::Frame& f) {
    const bool count = (c->cfg.flags & RT_FLAG_COUNTERS) != 0;
    const rtd::Scene sc = scene_of(c);
    const rtd::Planes pl = planes_of(c);
    const int D = c->cfg.depth;
    const uint32_t spp = (uint32_t)c->cfg.spp;
    const uint32_t B = c->batch_samples;
    const uint32_t ctrl_words = 2 * (RT_MAX_DEPTH + 2);
    uint32_t batch = 0;
    for (uint32_t s0 = 0; s0 < spp; s0 += B, batch++) {
        const uint32_t ns = spp - s0 < B ? spp - s0 : B;
        const uint32_t npaths = c->npix_pad * ns;
        uint32_t* counts = c->ctrl;
        uint32_t* cursors = c->ctrl + (RT_MAX_DEPTH + 2);
        RT_HIP(c, hipMemsetAsync(c->ctrl, 0, ctrl_words * sizeof(uint32_t), c->stream));

        rtd::TraceArgs ta{};
        ta.qox = c->qox; ta.qoy = c->qoy; ta.qoz = c->qoz; ta.qdx = c->qdx; ta.qdy = c->qdy; ta.qdz = c->qdz; ta.qid = c->qid;
        ta.qcap = c->cap; ta.nprimary = npaths; ta.npix_pad = c->npix_pad; ta.refill_threshold = c->refill_threshold;
        ta.hx = c->hx; ta.hy = c->hy; ta.hz = c->hz; ta.hinfo = c->hinfo; ta.sunres = c->sunres; ta.counters = c->d_counters;

        rtd::ShadeArgs sa{};
        sa.qox = c->qox; sa.qoy = c->qoy; sa.qoz = c->qoz; sa.qdx = c->qdx; sa.qdy = c->qdy; sa.qdz = c->qdz; sa.qid = c->qid;
        sa.qcap = c->cap; sa.npaths = npaths; sa.npaths_cap = c->cap; sa.npix_pad = c->npix_pad; sa.sample0 = s0;
        sa.hx = c->hx; sa.hy = c->hy; sa.hz = c->hz; sa.hinfo = c->hinfo; sa.sunres = c->sunres;
        sa.pdx = c->pdx; sa.pdy = c->pdy; sa.pdz = c->pdz; sa.pnormal = c->pnormal; sa.pstate = c->pstate;
        sa.sunbits = c->sunbits; sa.stack = c->stack; sa.plx = c->plx; sa.ply = c->ply; sa.plz = c->plz;
        sa.counters = c->d_counters;

        // primary wave
        ta.qcount = counts + 0; ta.cursor = cursors + 0;
        { LaunchTimer t(c, 0); RT_HIP(c, rtd::launch_trace(sc, f, ta, true, count, c->num_cus, c->stream)); }
        sa.qcount_next = counts + 1;
        { LaunchTimer t(c, 1); RT_HIP(c, rtd::launch_shade0(sc, f, sa, pl, count, c->stream)); }
        for (int level = 1; level <= D; level++) {
            ta.qcount = counts + level; ta.cursor = cursors + level;
            { LaunchTimer t(c, 0); RT_HIP(c, rtd::launch_trace(sc, f, ta, false, count, c->num_cus, c->stream)); }
            sa.qcount_next = counts + level + 1;
            { LaunchTimer t(c, 1); RT_HIP(c, rtd::launch_shadeN(sc, f, sa, level, count, c->stream)); }
        }
        { LaunchTimer t(c, 1); RT_HIP(c, rtd::launch_accumulate(c->plx, c->ply, c->plz, c->acc, c->npix_pad, ns, batch == 0, c->stream)); }
    }
    { LaunchTimer t(c, 1); RT_HIP(c, rtd::launch_resolve(f, c->acc, pl, c->npix_pad, c->stream)); }
    return RT_OK;
}

// ---- a frame of the persistent family (k_frame, or prepass + path launches on k_persist / k_paths) ----------------------------
// The steps below run in this order, each only if the ones before it enqueued without error; draw_persistent then publishes the
// frame whatever happened (later frames depend on the slot, lane and accumulation state it leaves).
struct PersistFrame {
    const rtd::Frame& f;
    bool count = false, cache = false;
    int nl = 1, nsl = 1;                // lanes and frame slots in use (one each on a caller's stream)
    int si = 0;                         // the frame's slot
    FrameSlot* fs = nullptr;
    rtd::Planes pl{};                   // the slot's planes
    bool one_lane = false;              // every launch of the frame on lane 0
    Lane* L0 = nullptr;                 // the lane of the prepass and the first launch ...
    hipStream_t st0 = nullptr;          // ... and its stream
    hipStream_t tail = nullptr;         // the stream the frame ends on
    uint32_t* wlc = nullptr;            // the frame's worklist counter (the slot has two: the other is its next prepass')
    bool reuse = false;                 // the slot's prepass is this frame's too: no prepass launch
    // RT_FLAG_ACCUMULATE
    bool accum = false, accum_cont = false;   // the context accumulates; this frame continues the running sum
    uint32_t key[16] = {};
    uint64_t accum_n = 0;               // samples the sum holds after this frame
    float4* accum_multi = nullptr;      // d_accum for frames of more than one sample
    int temporal_mode = rtd::TEMPORAL_RESTART;   // RT_FLAG_REPROJECT: how this frame's pass treats the history
};

// Something the prepasses read or wrote has changed (the world, the stream, a plane, a failed frame): no slot's is reused.
void invalidate_prepass(RtContext* c) {
    for (FrameSlot& fs : c->slots) fs.prepass_valid = false;
}

// A library call writes device memory the caller names (a post pass in place, an untiled frame): if that lies in a plane of a frame
// slot, the slot's prepass results are no longer what its planes hold (rt_denoise rewrites the sky pixels' lighting in place).
void plane_written(RtContext* c, const void* ptr) {
    const uint8_t* q = static_cast<const uint8_t*>(ptr);
    for (int sl = 0; sl < c->nslots; sl++)
        for (int b = 0; b < RT_BUF_COUNT; b++) {
            if (b == RT_BUF_FINAL_BGRA8) continue;   // (rt_finalize's output: no prepass result)
            const uint8_t* base = static_cast<const uint8_t*>(c->slots[sl].planes[b]);
            if (base && q >= base && q < base + c->plane_pixels * kBytesPerPixel[b]) c->slots[sl].prepass_valid = false;
        }
}

// the step that touches the running sum follows the previous frame's (ev_accum), not the whole previous frame
hipError_t accum_wait(RtContext* c, hipStream_t st) {
    return c->accum_recorded && c->accum_stream != st ? hipStreamWaitEvent(st, c->ev_accum, 0) : hipSuccess;
}

// The frame's slot and first lane, its accumulation key; then the slot's previous frame has finished with the slot.
hipError_t frame_begin(RtContext* c, PersistFrame& p, const RtUniforms* u, bool frame_events) {
    p.count = (c->cfg.flags & RT_FLAG_COUNTERS) != 0;
    p.cache = (c->cfg.flags & RT_FLAG_CACHE_PRIMARY) != 0;
    p.nl = c->user_stream ? 1 : c->nlanes;
    p.nsl = c->user_stream ? 1 : c->nslots;
    hipError_t e = hipSuccess;
    // What the host put behind the previous frame since (post passes, gather, a slab) belongs to that frame's use of its slot.
    FrameSlot& prev = c->slots[c->cur_slot];
    if (c->frame_recorded) { e = hipEventRecord(prev.ev_tail, c->stream); prev.tail_recorded = e == hipSuccess; }
    // This frame's slot, and the lane its prepass and first path launch go to (launches alternate between the lanes).
    p.si = p.nsl == 2 ? (int)(c->frames_drawn & 1u) : 0;
    p.fs = &c->slots[p.si];
    p.pl = planes_of(p.fs->planes);
    // (a one-slot context whose frames are one launch each stays on lane 0: frame k + 1 cannot start before frame k has finished
    // with the slot, so alternating would only put an event wait between two streams in front of every frame)
    p.one_lane = p.nsl == 1 && (uint32_t)c->cfg.spp <= c->persist_batch;
    p.L0 = &c->lanes[p.one_lane ? 0u : c->path_launches % (uint64_t)p.nl];
    p.st0 = p.tail = p.L0->stream;
    accum_key_of(u, p.key);
    // The primary ray reads no noise, so what the prepass leaves in the slot depends on every live uniform but the seed (the
    // accumulation key), the context's configuration and the world.  A frame whose slot still holds the prepass of that key skips
    // its own: a still camera over an unchanged world re-traces nothing.  Not where the prepass does more than that: counters
    // (they count the prepass' rays), a running sum or history (the prepass then runs as a one-sample frame and k_accumulate_frame /
    // the temporal pass rewrite the lighting it finished).  Everything else a later launch of the frame writes, it writes again
    // in every frame (the lighting of worklist pixels: the last accumulate launch, or the path launch itself on the direct
    // route; the per-pixel sums of a multi-batch frame start from 0 in its first batch).
    p.reuse = c->prepass_reuse && p.cache && !c->route.frame && !p.count && c->d_accum == nullptr && !c->reproject &&
              (c->cfg.flags & (RT_FLAG_ACCUMULATE | RT_FLAG_REPROJECT)) == 0 && p.fs->prepass_valid &&
              memcmp(p.key, p.fs->prepass_key, sizeof(p.key)) == 0;
    // worklist counter of this frame: clean already if the slot's previous prepass cleared it, otherwise cleared there; a reusing
    // frame reads the one its slot's last prepass counted in (no flip, no clear)
    p.wlc = p.fs->wl_count + kWlSetWords * (size_t)(p.fs->wl_parity ^ (p.reuse ? 1 : 0));
    // RT_FLAG_ACCUMULATE: does this frame continue the running sum, and how many samples will it hold (the lighting's divisor)?
    // One-sample frames add theirs in k_accumulate_frame after the frame's launches.  Frames of more samples continue the ordered
    // sum from the running one: k_accumulate_frame for the pixels the prepass finishes, k_accumulate_paths<.., ACCUM> for the
    // paths' (its first batch starts from the running sum, its last stores it back).
    const uint32_t spp = (uint32_t)c->cfg.spp;
    p.accum = c->d_accum != nullptr;
    p.accum_cont = p.accum && c->accum_valid && memcmp(p.key, c->accum_key, sizeof(p.key)) == 0 && c->accum_samples + spp <= (1ull << 24);
    p.accum_n = p.accum_cont ? c->accum_samples + spp : spp;
    p.accum_multi = p.accum && spp > 1u ? c->d_accum : nullptr;
    // RT_FLAG_REPROJECT (one-sample frames): a camera change no longer restarts the history — only sun_angle, what invalidates the
    // sum anyway and the 2^24 bound do.  accum_n is then the upper bound of any pixel's count.
    if (c->reproject) {
        const bool still = p.accum_cont;   // (every live uniform equal, valid, below 2^24)
        const bool same_camera = memcmp(p.key, c->accum_key, sizeof(p.key)) == 0;
        if (still) p.temporal_mode = rtd::TEMPORAL_STILL;
        else if (c->accum_valid && !same_camera && p.key[0] == c->accum_key[0]) p.temporal_mode = rtd::TEMPORAL_MOVED;
        else p.temporal_mode = rtd::TEMPORAL_RESTART;
        if (p.temporal_mode == rtd::TEMPORAL_MOVED) {
            p.accum_cont = true;
            p.accum_n = (c->accum_samples < c->history_cap ? c->accum_samples : (uint64_t)c->history_cap) + 1u;
        }
    }
    // the frame that used the slot before (frame k - 2 with two slots, k - 1 with one) has finished with it
    if (e == hipSuccess && p.fs->tail_recorded) e = hipStreamWaitEvent(p.st0, p.fs->ev_tail, 0);
    if (e == hipSuccess && frame_events) e = hipEventRecord(c->ev_frame0, p.st0);
    return e;
}

// Cached primaries, frames k_frame does not take: the prepass traces the primary rays and queues the pixels that go on.
hipError_t frame_prepass(RtContext* c, PersistFrame& p) {
    FrameSlot& fs = *p.fs;
    const bool prepass_clears = c->primary_version == 2 && c->npix_pad != 0;
    hipError_t e = hipSuccess;
    fs.prepass_valid = false;   // (until this one is enqueued: it overwrites the worklist)
    if (!fs.wl_clean[fs.wl_parity]) e = hipMemsetAsync(p.wlc, 0, kWlClearWords * sizeof(uint32_t), p.st0);
    fs.wl_clean[fs.wl_parity] = false;
    LaunchTimer t(c, 1, p.st0);
    rtd::PrimaryArgs pr{};
    pr.phit = fs.phit;
    pr.worklist = fs.worklist; pr.wl_count = p.wlc; pr.tile_cursor = p.wlc + 32; pr.acc = fs.pacc; pr.counters = c->d_counters;
    // the prepass clears what the NEXT users need zeroed instead of a memset of its own in front of them: the slot's other
    // worklist counter and tile cursor (the slot's next prepass) and, unless the lane's last accumulate launch has done it, the
    // path cursors of the lane it runs on (this frame's first launch)
    const bool clear_cursors = prepass_clears && !p.L0->cursor_clean;
    pr.zero_words = prepass_clears ? fs.wl_count + kWlSetWords * (size_t)(fs.wl_parity ^ 1) : nullptr; pr.zero_count = (uint32_t)kWlClearWords;
    pr.zero_words2 = clear_cursors ? p.L0->cursor : nullptr; pr.zero_count2 = (uint32_t)kCursorWords;
    // accumulating: the prepass runs as a one-sample frame, so the light of a pixel it finishes is 16 x its lighting_f32 exactly;
    // k_accumulate_frame then adds it spp times to the pixel's running sum (the prepass adds it spp times to 0 otherwise)
    rtd::Frame fpre = p.f;
    if (p.accum_multi) fpre.spp = 1;
    if (e == hipSuccess) e = rtd::launch_primary(scene_of(c), fpre, p.pl, pr, p.count, c->primary_version, c->num_cus, p.st0);
    if (e == hipSuccess && p.accum_multi) e = accum_wait(c, p.st0);
    if (e == hipSuccess && p.accum_multi)
        e = rtd::launch_accumulate_frame(p.f, p.pl, c->d_accum, c->npix_pad, p.accum_cont, (int)p.accum_n, c->cfg.spp, true, p.st0);
    if (prepass_clears && e == hipSuccess) { fs.wl_clean[fs.wl_parity ^ 1] = true; p.L0->cursor_clean = true; }
    fs.wl_parity ^= 1;
    if (e == hipSuccess) { fs.prepass_valid = true; memcpy(fs.prepass_key, p.key, sizeof(p.key)); }
    return e;
}

// The two per-frame tables depend on the sun vector and colour only: rebuilt when those change (bit compare) — after every launch
// that reads the old ones, on either lane, and before any launch that follows.
hipError_t frame_tables(RtContext* c, PersistFrame& p) {
    const float lut_key[6] = {p.f.sunangle[0], p.f.sunangle[1], p.f.sunangle[2], p.f.sunlight[0], p.f.sunlight[1], p.f.sunlight[2]};
    if (c->cfg.depth < 1 || (c->lut_valid && memcmp(lut_key, c->lut_key, sizeof(lut_key)) == 0)) return hipSuccess;
    hipError_t e = p.nl == 2 ? join_lanes_into(c, p.st0) : hipSuccess;
    {
        LaunchTimer t(c, 1, p.st0);
        if (e == hipSuccess) e = rtd::launch_sun_lut(p.f, c->sun_lut, p.st0);
        if (e == hipSuccess) e = rtd::launch_sky_lut(p.f, c->dif_lut, p.st0);
    }
    if (e == hipSuccess && p.nl == 2) e = fence_lanes_after(c, p.st0);
    c->lut_valid = e == hipSuccess;
    memcpy(c->lut_key, lut_key, sizeof(lut_key));
    return e;
}

// k_frame: the whole frame in one launch.  With two frame slots consecutive frames go to the two streams in turn (frame k + 1
// starts while frame k's last workgroups finish); with one slot a frame follows the previous one anyway, and staying on one
// stream spares the cross-stream event wait between them.
hipError_t frame_one_launch(RtContext* c, PersistFrame& p) {
    if (p.nsl == 2) c->path_launches++;
    rtd::FrameArgs fa{};
    fa.threshold = c->frame_threshold; fa.tiles_per_group = c->frame_tiles; fa.sun_lut = c->sun_lut; fa.dif_lut = c->dif_lut; fa.pl = p.L0->ppl; fa.counters = c->d_counters;
    if (getenv("RT_DEBUG_WAVE_DUMP") && (size_t)c->ntiles_local * 32u <= (size_t)4 * c->num_cus * 1024 * sizeof(uint32_t))
        fa.dbg_waves = reinterpret_cast<unsigned long long*>(c->lanes[0].pstack);   // (idle while k_frame runs)
    LaunchTimer t(c, 0, p.st0);
    return rtd::launch_frame(scene_of(c), p.f, p.pl, fa, p.count, c->num_cus, p.st0);
}

// The path launches, persist_batch samples each, on the kernels the route gives their size, each with its accumulate launch.
hipError_t frame_path_batches(RtContext* c, PersistFrame& p) {
    const Route& r = c->route;
    FrameSlot& fs = *p.fs;
    const uint32_t spp = (uint32_t)c->cfg.spp, B = c->persist_batch;
    hipError_t e = hipSuccess;
    if (p.nl == 2 && spp > B) e = hipEventRecord(fs.ev_prepass, p.st0);   // launches on the other lane wait for the prepass
    for (uint32_t s0 = 0; s0 < spp && e == hipSuccess; s0 += B) {
        const uint32_t ns = spp - s0 < B ? spp - s0 : B;
        // the sample batches of a frame alternate between the lanes: batch b + 1 starts on the CUs batch b's workgroups leave
        Lane* L = &c->lanes[p.one_lane ? 0u : c->path_launches % (uint64_t)p.nl];
        const hipStream_t st = L->stream;
        if (!p.one_lane) c->path_launches++;
        if (st != p.st0 && s0 == B) e = hipStreamWaitEvent(st, fs.ev_prepass, 0);   // (later batches on that lane follow by stream order)
        if (e == hipSuccess && !L->cursor_clean) e = hipMemsetAsync(L->cursor, 0, kCursorWords * sizeof(uint32_t), st);
        L->cursor_clean = false;
        const bool to_paths = r.on_paths(ns);
        rtd::PersistArgs pa{};
        pa.cursor = L->cursor; pa.worklist = fs.worklist; pa.wl_count = p.wlc; pa.direct = r.direct ? 1u : 0u;
        pa.npix_pad = c->npix_pad; pa.sample0 = s0; pa.nsamples = ns; pa.rmin = c->persist_rmin; pa.chunk = c->persist_chunk;
        pa.threshold = to_paths ? r.threshold_paths : r.threshold_persist;
        pa.nthreads = (uint32_t)c->num_cus * 1024u; pa.stack = L->pstack;
        pa.phit = fs.phit;
        pa.sun_lut = c->sun_lut; pa.dif_lut = c->dif_lut;
        pa.pl = L->ppl; pa.counters = c->d_counters;
        // light records of this launch: streamed past the caches when there are more of them than would stay there until the
        // accumulate launch reads them (the Infinity Cache holds 256 MB; RT_PL_STREAM = 0 / 1 / 2 / 3 forces never / stores /
        // loads / both)
        const uint64_t record_bytes = (uint64_t)c->npix_pad * ns * sizeof(rtd::PathLight);
        const bool big_records = record_bytes > kStreamRecordBytes;
        const bool stream_st = c->pl_stream_mode < 0 ? big_records : (c->pl_stream_mode & 1) != 0;
        const bool stream_ld = c->pl_stream_mode < 0 ? big_records : (c->pl_stream_mode & 2) != 0;
        pa.pl_stream = stream_st ? 1u : 0u;
        if (e == hipSuccess) {
            LaunchTimer t(c, 0, st);
            e = to_paths ? rtd::launch_paths(scene_of(c), p.f, p.pl, pa, p.count, c->num_cus, st)
                         : rtd::launch_persist(scene_of(c), p.f, p.pl, pa, p.count, p.cache, 1, c->num_cus, st);
        }
        if (e == hipSuccess && !r.direct) {
            // a pixel's samples are added in sample order: batch b's accumulate follows batch b - 1's, whichever lane that ran on
            if (p.nl == 2 && s0 != 0) e = hipStreamWaitEvent(st, fs.ev_acc, 0);
            // (with cached primaries the prepass, which came first, has waited for the previous frame's running sums)
            if (e == hipSuccess && p.accum_multi && !p.cache && s0 == 0) e = accum_wait(c, st);
            {
                LaunchTimer t(c, 1, st);
                if (e == hipSuccess)
                    e = rtd::launch_accumulate_paths(p.f, p.pl, L->ppl, fs.worklist, p.wlc, c->npix_pad, ns, s0 == 0, s0 + B >= spp, p.cache,
                                                     stream_ld, fs.pacc, p.accum_multi, p.accum_cont, (int)p.accum_n, L->cursor,
                                                     (uint32_t)kCursorWords, st);
                // (it has cleared the lane's path cursors behind the path launch: the lane's next one needs no memset)
                if (e == hipSuccess && c->npix_pad != 0) L->cursor_clean = true;
            }
            if (e == hipSuccess && p.nl == 2 && s0 + B < spp) e = hipEventRecord(fs.ev_acc, st);
        }
        p.tail = st;
    }
    return e;
}

// RT_FLAG_ACCUMULATE after the frame's launches: a one-sample frame adds its light to the running sum; with two lanes, ev_accum
// marks the last step that touched the sum.  (No resolve launch: the prepass and the frame's last accumulate store the lighting.)
hipError_t frame_accumulate_tail(RtContext* c, PersistFrame& p) {
    hipError_t e = hipSuccess;
    if (c->cfg.spp == 1) {
        e = accum_wait(c, p.tail);
        LaunchTimer t(c, 1, p.tail);
        if (e == hipSuccess && !c->reproject)
            e = rtd::launch_accumulate_frame(p.f, p.pl, c->d_accum, c->npix_pad, p.accum_cont, (int)p.accum_n, 1, false, p.tail);
        if (e == hipSuccess && c->reproject) {
            // the pass reads the set the previous frame's pass wrote (ordered by accum_wait / stream order) and writes the other
            rtd::TemporalArgs ta{};
            const int prev = c->hist_cur, next = prev ^ 1;
            ta.prev_sum = c->d_hist_sum[prev]; ta.prev_rec = c->d_hist_rec[prev];
            ta.next_sum = c->d_hist_sum[next]; ta.next_rec = c->d_hist_rec[next];
            memcpy(ta.origin, &c->accum_key[1], 12); memcpy(ta.forward, &c->accum_key[4], 12);
            memcpy(ta.up, &c->accum_key[7], 12); memcpy(ta.right, &c->accum_key[10], 12);
            ta.cap = c->history_cap;
            e = rtd::launch_temporal_frame(p.f, p.pl, ta, p.temporal_mode, p.tail);
            c->hist_cur = next;
        }
    }
    if (e == hipSuccess && p.nl == 2) {
        e = hipEventRecord(c->ev_accum, p.tail);
        c->accum_recorded = e == hipSuccess;
        c->accum_stream = p.tail;
    }
    return e;
}

// The frame ends on `tail`: post passes, gather and readback of THIS frame follow it there; its planes are the context's.
void frame_publish(RtContext* c, const PersistFrame& p, hipError_t e) {
    if (e != hipSuccess) invalidate_prepass(c);
    if (p.accum) {
        c->accum_valid = e == hipSuccess;
        c->accum_frames = p.accum_cont ? c->accum_frames + 1u : 1u;
        c->accum_samples = p.accum_n;
        memcpy(c->accum_key, p.key, sizeof(p.key));
    }
    c->stream = p.tail;
    c->cur_slot = p.si;
    c->gbuffer = p.fs->gbuffer;
    for (int b = 0; b < RT_BUF_COUNT; b++) c->planes[b] = p.fs->planes[b];
    c->frames_drawn++;
}

int draw_persistent(RtContext* c, const rtd::Frame& f, const RtUniforms* u, bool frame_events) {
    PersistFrame p{f};
    hipError_t e = frame_begin(c, p, u, frame_events);
    if (e == hipSuccess && p.cache && !c->route.frame && !p.reuse) e = frame_prepass(c, p);
    if (e == hipSuccess) e = frame_tables(c, p);
    if (e == hipSuccess && c->route.frame) e = frame_one_launch(c, p);
    else if (e == hipSuccess && (!p.cache || c->cfg.depth >= 1)) e = frame_path_batches(c, p);   // (cached depth 0: the prepass is the frame)
    if (e == hipSuccess && p.accum) e = frame_accumulate_tail(c, p);
    frame_publish(c, p, e);
    return e == hipSuccess ? RT_OK : fail(c, RT_ERR_HIP, std::string("persistent path: ") + hipGetErrorString(e));
}

}  // namespace

// Light-record budget of a context (all lanes together): RT_PERSIST_LIGHT_GIB, else min(kDefaultLightBytes, a tenth of the free
// device memory): a context is one tenant of the GPU.  Pure function of its inputs apart from hipMemGetInfo.
constexpr uint64_t kDefaultLightBytes = 16ull << 30;
uint64_t rt_light_budget_bytes(const char* env_gib) {
    uint64_t light_bytes = kDefaultLightBytes;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) { if ((uint64_t)free_b / 10u < light_bytes) light_bytes = (uint64_t)free_b / 10u; }
    else (void)hipGetLastError();
    if (env_gib) { long long v = atoll(env_gib); if (v >= 1 && v <= 128) light_bytes = (uint64_t)v << 30; }
    return light_bytes;
}
// Samples of every pixel one launch covers: what `lane_bytes` of 12-byte records hold for `npix` worklist slots, at most 2^31
// paths (path indices are 32-bit), at most spp, at least 1; RT_PERSIST_BATCH may only lower it.  (tests/test_abi.py pins it.)
extern "C" uint64_t rt_samples_per_launch(uint64_t lane_bytes, uint64_t npix, uint64_t spp, const char* env_batch) {
    if (npix == 0) npix = 1;
    uint64_t B = lane_bytes / (sizeof(rtd::PathLight) * npix);
    if (B > (1ull << 31) / npix) B = (1ull << 31) / npix;
    if (env_batch) { long long v = atoll(env_batch); if (v > 0 && (uint64_t)v < B) B = (uint64_t)v; }
    if (B < 1) B = 1;
    if (B > spp) B = spp;
    return B;
}

namespace {
// rt_create's steps, in allocation order: each reports a failure through c->err; rt_create hands it on and destroys the context

// the device, the context's stream and frame events, and the scene
int create_device(RtContext* c) {
    RT_HIP(c, hipSetDevice(c->device));
    hipDeviceProp_t prop;
    RT_HIP(c, hipGetDeviceProperties(&prop, c->device));
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // RT_RESERVE_CUS=n: the persistent kernels (one workgroup per CU) leave n CUs free, e.g. for an RCCL kernel running
    // beside them (bench.py's overlapped gather)
    if (const char* s = getenv("RT_RESERVE_CUS")) { int v = atoi(s); if (v > 0 && v < c->num_cus) c->num_cus -= v; }
    RT_HIP(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    c->lanes[0].stream = c->own_stream;
    RT_HIP(c, hipEventCreate(&c->ev_frame0));
    RT_HIP(c, hipEventCreate(&c->ev_frame1));
    RT_HIP(c, dev_alloc(c, &c->d_mine_sw, c->vox)); RT_HIP(c, dev_alloc(c, &c->d_mat_sw, c->vox));
    RT_HIP(c, dev_alloc(c, &c->d_coarse, (size_t)rtd::kCoarseWords));
    // (the per-brick map of a -DRT_PATHS_BRICK_MAP=1 build of k_paths: an experiment that lost, profiles/r4_c5_brick_map.txt)
    if (c->logr > 8 && getenv("RT_BRICK_MAP")) RT_HIP(c, dev_alloc(c, &c->d_brick, c->vox / 128u / 4u));
    RT_HIP(c, dev_alloc(c, &c->d_noise, (size_t)RT_NOISE_SIZE * RT_NOISE_SIZE));
    RT_HIP(c, dev_alloc(c, &c->d_flag, 4));
    RT_HIP(c, dev_alloc(c, &c->d_counters, 1));
    RT_HIP(c, hipMemset(c->d_counters, 0, sizeof(rtd::DevCounters)));
    return RT_OK;
}

// the lanes' second stream and events, and the frame slots' planes and events
int create_slots(RtContext* c) {
    if (c->nlanes == 2) RT_HIP(c, hipStreamCreateWithFlags(&c->lanes[1].stream, hipStreamNonBlocking));
    for (int l = 0; l < c->nlanes; l++) RT_HIP(c, hipEventCreateWithFlags(&c->lanes[l].ev_join, hipEventDisableTiming));
    RT_HIP(c, hipEventCreateWithFlags(&c->ev_fence, hipEventDisableTiming));
    RT_HIP(c, hipEventCreateWithFlags(&c->ev_world, hipEventDisableTiming));
    RT_HIP(c, hipEventCreateWithFlags(&c->ev_query, hipEventDisableTiming));
    RT_HIP(c, hipEventCreateWithFlags(&c->ev_gather, hipEventDisableTiming));
    // the six reference-format planes of a slot live in ONE block (each padded to 256 B) so a multi-GPU host can gather them
    // with a single collective; the other planes are separate allocations
    size_t off = 0;
    for (int b = 0; b <= RT_BUF_FOG_RGBA8; b++) {
        c->gbuffer_offset[b] = off;
        off += (c->plane_pixels * kBytesPerPixel[b] + 255) / 256 * 256;
    }
    c->gbuffer_bytes = off;
    for (int sl = 0; sl < c->nslots; sl++) {
        FrameSlot& fs = c->slots[sl];
        uint8_t* block = nullptr;
        RT_HIP(c, dev_alloc(c, &block, off));
        RT_HIP(c, hipMemset(block, 0, off));
        fs.gbuffer = block;
        for (int b = 0; b <= RT_BUF_FOG_RGBA8; b++) fs.planes[b] = block + c->gbuffer_offset[b];
        for (int b = RT_BUF_FOG_RGBA8 + 1; b < RT_BUF_COUNT; b++) {
            uint8_t* p = nullptr;
            RT_HIP(c, dev_alloc(c, &p, c->plane_pixels * kBytesPerPixel[b]));
            RT_HIP(c, hipMemset(p, 0, c->plane_pixels * kBytesPerPixel[b]));
            fs.planes[b] = p;
        }
        RT_HIP(c, hipEventCreateWithFlags(&fs.ev_prepass, hipEventDisableTiming));
        RT_HIP(c, hipEventCreateWithFlags(&fs.ev_acc, hipEventDisableTiming));
        RT_HIP(c, hipEventCreateWithFlags(&fs.ev_tail, hipEventDisableTiming));
    }
    c->cur_slot = 0;
    c->gbuffer = c->slots[0].gbuffer;
    for (int b = 0; b < RT_BUF_COUNT; b++) c->planes[b] = c->slots[0].planes[b];
    return RT_OK;
}

// the persistent family's per-lane and per-slot buffers, tables and light records (sets persist_batch)
int create_persistent(RtContext* c) {
    const RtConfig& cfg = c->cfg;
    const size_t stack_words = (size_t)4 * c->num_cus * 1024 * (size_t)(cfg.depth > 1 ? cfg.depth - 1 : 1);   // up to 3 paths per lane
    for (int l = 0; l < c->nlanes; l++) {
        Lane& ln = c->lanes[l];
        RT_HIP(c, dev_alloc(c, &ln.cursor, kCursorWords));
        RT_HIP(c, hipMemset(ln.cursor, 0, kCursorWords * sizeof(uint32_t)));
        ln.cursor_clean = true;
        RT_HIP(c, dev_alloc(c, &ln.pstack, stack_words));
    }
    for (int sl = 0; sl < c->nslots; sl++) {
        FrameSlot& fs = c->slots[sl];
        RT_HIP(c, dev_alloc(c, &fs.wl_count, 2 * kWlSetWords));   // two sets: counter and tile cursor, 128 bytes apart
        RT_HIP(c, hipMemset(fs.wl_count, 0, 2 * kWlSetWords * sizeof(uint32_t)));
        fs.wl_clean[0] = fs.wl_clean[1] = true;
        RT_HIP(c, dev_alloc(c, &fs.worklist, (size_t)c->npix_pad));
        RT_HIP(c, dev_alloc(c, &fs.phit, (size_t)c->npix_pad));
        RT_HIP(c, dev_alloc(c, &fs.pacc, (size_t)c->npix_pad));
    }
    RT_HIP(c, dev_alloc(c, &c->sphere_lut, (size_t)65536));
    RT_HIP(c, dev_alloc(c, &c->sun_lut, (size_t)2 * 65536));
    RT_HIP(c, dev_alloc(c, &c->dif_lut, (size_t)4 * 6 * 65536));
    // Samples per path-kernel launch: bounded by 2^31 work items and by the memory given to the per-path light records, which is
    // split between the lanes (a launch's records live until its accumulate launch has read them, and two launches are in flight).
    // Round 3 sized one launch for 16 GiB because every launch paid its ramp-up and its drain (3840x2160 spp 256 depth 8: 114.1 ms
    // per frame with 1 GiB, 109.3 with 2, 107.0 with 4, 105.6 with 8 and beyond); with the next launch taking the CUs the draining
    // one frees, a launch's size matters far less (see kDefaultLightBytes).  Halved until the allocation succeeds.
    const uint64_t np = c->npix_pad ? c->npix_pad : 1;
    c->light_budget_bytes = rt_light_budget_bytes(getenv("RT_PERSIST_LIGHT_GIB"));
    uint64_t B = rt_samples_per_launch(c->light_budget_bytes / (uint64_t)c->nlanes, np, (uint64_t)cfg.spp, getenv("RT_PERSIST_BATCH"));
    for (int l = 0; l < c->nlanes; l++) {
        for (;;) {
            const hipError_t e = dev_alloc(c, &c->lanes[l].ppl, (size_t)np * B);
            if (e == hipSuccess) break;
            if (e != hipErrorOutOfMemory || B == 1 || l > 0) RT_HIP(c, e);   // (the lanes' buffers have one size)
            (void)hipGetLastError();
            B = (B + 1) / 2;
        }
    }
    c->persist_batch = (uint32_t)B;
    if (cfg.flags & RT_FLAG_ACCUMULATE) {
        RT_HIP(c, dev_alloc(c, &c->d_accum, (size_t)c->npix_pad));
        RT_HIP(c, hipEventCreateWithFlags(&c->ev_accum, hipEventDisableTiming));
    }
    if (c->reproject) {
        c->d_hist_sum[0] = c->d_accum;
        RT_HIP(c, dev_alloc(c, &c->d_hist_sum[1], (size_t)c->npix_pad));
        for (int h = 0; h < 2; h++) {
            RT_HIP(c, dev_alloc(c, &c->d_hist_rec[h], (size_t)c->npix_pad));
            RT_HIP(c, hipMemset(c->d_hist_rec[h], 0, (size_t)c->npix_pad * sizeof(uint2)));   // rt_read_history before the first frame
        }
    }
    RT_HIP(c, rtd::launch_sphere_lut(c->sphere_lut, c->own_stream));
    RT_HIP(c, rtd::launch_dif_lut(c->sphere_lut, c->dif_lut, c->own_stream));
    RT_HIP(c, hipStreamSynchronize(c->own_stream));
    return RT_OK;
}

// the wavefront baseline's queues
int create_wavefront(RtContext* c) {
    uint64_t target = 4u << 20;   // paths per batch
    if (const char* s = getenv("RT_BATCH_PATHS")) { long long v = atoll(s); if (v > 0) target = (uint64_t)v; }
    uint64_t B = c->npix_pad ? target / c->npix_pad : 1;
    if (B < 1) B = 1;
    if (B > (uint64_t)c->cfg.spp) B = (uint64_t)c->cfg.spp;
    c->batch_samples = (uint32_t)B;
    uint64_t cap64 = (uint64_t)c->npix_pad * B;
    if (cap64 >= (1ull << 31)) return fail(c, RT_ERR_INVALID_ARG, "rt_create: batch too large");
    c->cap = (uint32_t)cap64;
    const size_t cap = c->cap;
    RT_HIP(c, dev_alloc(c, &c->qox, cap)); RT_HIP(c, dev_alloc(c, &c->qoy, cap)); RT_HIP(c, dev_alloc(c, &c->qoz, cap));
    RT_HIP(c, dev_alloc(c, &c->qdx, 2 * cap)); RT_HIP(c, dev_alloc(c, &c->qdy, 2 * cap)); RT_HIP(c, dev_alloc(c, &c->qdz, 2 * cap));
    RT_HIP(c, dev_alloc(c, &c->qid, cap));
    RT_HIP(c, dev_alloc(c, &c->hx, cap)); RT_HIP(c, dev_alloc(c, &c->hy, cap)); RT_HIP(c, dev_alloc(c, &c->hz, cap));
    RT_HIP(c, dev_alloc(c, &c->hinfo, cap));
    RT_HIP(c, dev_alloc(c, &c->sunres, cap)); RT_HIP(c, dev_alloc(c, &c->pnormal, cap)); RT_HIP(c, dev_alloc(c, &c->pstate, cap));
    RT_HIP(c, dev_alloc(c, &c->pdx, cap)); RT_HIP(c, dev_alloc(c, &c->pdy, cap)); RT_HIP(c, dev_alloc(c, &c->pdz, cap));
    RT_HIP(c, dev_alloc(c, &c->plx, cap)); RT_HIP(c, dev_alloc(c, &c->ply, cap)); RT_HIP(c, dev_alloc(c, &c->plz, cap));
    RT_HIP(c, dev_alloc(c, &c->sunbits, cap));
    RT_HIP(c, dev_alloc(c, &c->stack, cap * (size_t)(c->cfg.depth > 1 ? c->cfg.depth - 1 : 1)));
    RT_HIP(c, dev_alloc(c, &c->acc, (size_t)c->npix_pad));
    RT_HIP(c, dev_alloc(c, &c->ctrl, (size_t)2 * (RT_MAX_DEPTH + 2)));
    return RT_OK;
}
}  // namespace

extern "C" {

uint32_t rt_abi_version(void) { return ((uint32_t)RT_ABI_VERSION_MAJOR << 16) | (uint32_t)RT_ABI_VERSION_MINOR; }

const char* rt_last_error(RtContext* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int rt_create(const RtConfig* cfg, RtContext** out) {
    if (out) *out = nullptr;
    if (!cfg || !out) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: null argument");
    if (cfg->struct_size != sizeof(RtConfig)) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: RtConfig.struct_size mismatch");
    if (cfg->width <= 0 || cfg->height <= 0 || cfg->width > 16384 || cfg->height > 16384)
        return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: width/height out of range");
    if (cfg->region != 256 && cfg->region != 512 && cfg->region != 1024)
        return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: region must be 256 (the reference), 512 or 1024");
    if (cfg->region != 256 && cfg->kernel == RT_KERNEL_WAVEFRONT)
        return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: the split wavefront baseline supports region 256 only");
    if (cfg->spp < 1 || cfg->spp > RT_NOISE_BYTES) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: spp out of range");
    if (cfg->depth < 0 || cfg->depth > RT_MAX_DEPTH) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: depth out of range");
    if (cfg->tile_world < 1 || cfg->tile_rank < 0 || cfg->tile_rank >= cfg->tile_world)
        return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: bad tile_rank/tile_world");
    if (cfg->kernel < RT_KERNEL_DEFAULT || cfg->kernel > RT_KERNEL_FRAME || cfg->kernel == 4 /* RT_KERNEL_PERSISTENT2, retired in round 3 */ ||
        cfg->kernel == 6 /* RT_KERNEL_SEQ, retired in round 4 */)
        return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: unknown kernel");
    if ((cfg->flags & RT_FLAG_ACCUMULATE) && (cfg->kernel == RT_KERNEL_MEGA || cfg->kernel == RT_KERNEL_WAVEFRONT))
        return fail(nullptr, RT_ERR_UNIMPLEMENTED, "rt_create: RT_FLAG_ACCUMULATE needs RT_KERNEL_DEFAULT, FRAME, PATHS or PERSISTENT (not the baselines)");
    if (cfg->flags & RT_FLAG_REPROJECT) {
        if (!(cfg->flags & RT_FLAG_ACCUMULATE))
            return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: RT_FLAG_REPROJECT needs RT_FLAG_ACCUMULATE");
        if (cfg->history_cap < 0 || cfg->history_cap > 65535)
            return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: history_cap must be 0 (the default, 32) or 1..65535");
        if (cfg->spp != 1 || cfg->tile_world != 1)
            return fail(nullptr, RT_ERR_UNIMPLEMENTED, "rt_create: RT_FLAG_REPROJECT needs one-sample whole frames (spp == 1, tile_world == 1)");
    }

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, RT_ERR_NO_DEVICE, std::string("rt_create: no HIP device (") + hipGetErrorString(e) + ")");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: device ordinal out of range");

    RtContext* c = new (std::nothrow) RtContext();
    if (!c) return fail(nullptr, RT_ERR_OOM, "rt_create: host allocation failed");
    c->cfg = *cfg;
    c->device = cfg->device;
    c->region = cfg->region;
    c->logr = cfg->region == 256 ? 8 : (cfg->region == 512 ? 9 : 10);
    c->vox = (size_t)cfg->region * cfg->region * cfg->region;
    // RT_KERNEL_DEFAULT, FRAME, PATHS and PERSISTENT all run the persistent family (k_frame, k_persist, k_paths): resolve_route
    // decides which kernel takes what once the samples per launch are known
    c->route.family = (cfg->kernel == RT_KERNEL_MEGA || cfg->kernel == RT_KERNEL_WAVEFRONT) ? cfg->kernel : RT_KERNEL_PERSISTENT;
    const bool persistent = c->route.family == RT_KERNEL_PERSISTENT;
    c->reproject = (cfg->flags & RT_FLAG_REPROJECT) != 0;
    c->history_cap = cfg->history_cap > 0 ? (uint32_t)cfg->history_cap : 32u;

    // tiling: 8x8-pixel tiles dealt round-robin over tile_world contexts
    c->tiles_x = (cfg->width + 7) / 8; c->tiles_y = (cfg->height + 7) / 8;
    c->ntiles_total = c->tiles_x * c->tiles_y;
    c->tile_capacity = (c->ntiles_total + cfg->tile_world - 1) / cfg->tile_world;
    c->ntiles_local = (c->ntiles_total - cfg->tile_rank + cfg->tile_world - 1) / cfg->tile_world;
    if (c->ntiles_local < 0) c->ntiles_local = 0;
    c->npix_pad = (uint32_t)c->ntiles_local * 64u;
    c->plane_pixels = cfg->tile_world == 1 ? (size_t)cfg->width * cfg->height : (size_t)c->tile_capacity * 64;

    // lanes and frame slots (see Lane / FrameSlot).  Two lanes for the persistent kernels; two slots when the host asks for two
    // frames in flight.
    c->nlanes = persistent ? 2 : 1;
    c->nslots = (persistent && (cfg->flags & RT_FLAG_FRAMES_IN_FLIGHT_2)) ? 2 : 1;
    // environment knobs (experiments, A/B timing); those that size allocations are read where the allocation is made
    if (const char* s = getenv("RT_LANES")) { int v = atoi(s); if (v == 1 || (v == 2 && persistent)) c->nlanes = v; }
    if (const char* s = getenv("RT_FRAMES_IN_FLIGHT")) { int v = atoi(s); if (v == 1 || (v == 2 && persistent)) c->nslots = v; }
    if (c->nlanes < 2) c->nslots = 1;
    if (const char* s = getenv("RT_FRAME_CROSSOVER")) { long long v = atoll(s); if (v >= 0) c->frame_crossover = (uint64_t)v; }
    if (const char* s = getenv("RT_FRAME_CROSSOVER_MULTI")) { long long v = atoll(s); if (v >= 0) c->frame_crossover_multi = (uint64_t)v; }
    if (const char* s = getenv("RT_FRAME_THRESHOLD")) { int v = atoi(s); if (v >= 1 && v <= 64) c->frame_threshold = (uint32_t)v; }
    if (const char* s = getenv("RT_FRAME_TILES")) { int v = atoi(s); if (v >= 1 && v <= 4) c->frame_tiles = 4u * (uint32_t)v; }           // per wave
    if (const char* s = getenv("RT_FRAME_GROUP_TILES")) { int v = atoi(s); if (v >= 1 && v <= 16) c->frame_tiles = (uint32_t)v; }     // per four-wave workgroup
    if (const char* s = getenv("RT_REFILL_THRESHOLD")) { int v = atoi(s); if (v >= 1 && v <= 64) c->refill_threshold = (uint32_t)v; }
    if (const char* s = getenv("RT_PREPASS_REUSE")) { if (atoi(s) == 0) c->prepass_reuse = false; }
    if (const char* s = getenv("RT_PRIMARY_V")) { int v = atoi(s); if (v == 1 || v == 2) c->primary_version = v; }
    if (const char* s = getenv("RT_PERSIST_THRESHOLD")) { int v = atoi(s); if (v >= 1 && v <= 64) c->persist_threshold = (uint32_t)v; }
    if (const char* s = getenv("RT_PL_STREAM")) { int v = atoi(s); if (v >= 0 && v <= 3) c->pl_stream_mode = v; }
    if (const char* s = getenv("RT_PERSIST_CHUNK")) { int v = atoi(s); if (v >= 64 && v <= 4096) c->persist_chunk = (uint32_t)v & ~63u; }
    if (const char* s = getenv("RT_PERSIST_RMIN")) { int v = atoi(s); if (v >= 1 && v <= 128) c->persist_rmin = (uint32_t)v; }

    int rc = create_device(c);
    if (rc == RT_OK) rc = create_slots(c);
    if (rc == RT_OK && persistent) rc = create_persistent(c);
    if (rc == RT_OK && c->route.family == RT_KERNEL_WAVEFRONT) rc = create_wavefront(c);
    if (rc != RT_OK) {
        g_create_error = c->err;
        rt_destroy(c);
        return rc;
    }
    resolve_route(c);
    *out = c;
    return RT_OK;
}

void rt_destroy(RtContext* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->own_stream) (void)hipStreamSynchronize(ctx->own_stream);
    if (ctx->stream && ctx->stream != ctx->own_stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->lanes[1].stream) { (void)hipStreamSynchronize(ctx->lanes[1].stream); (void)hipStreamDestroy(ctx->lanes[1].stream); }
    for (Lane& ln : ctx->lanes) if (ln.ev_join) (void)hipEventDestroy(ln.ev_join);
    for (FrameSlot& fs : ctx->slots) for (hipEvent_t e : {fs.ev_prepass, fs.ev_acc, fs.ev_tail}) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {ctx->ev_fence, ctx->ev_gather, ctx->ev_accum}) if (e) (void)hipEventDestroy(e);
    if (ctx->upload_stream) { (void)hipStreamSynchronize(ctx->upload_stream); (void)hipStreamDestroy(ctx->upload_stream); }
    if (ctx->query_stream) { (void)hipStreamSynchronize(ctx->query_stream); (void)hipStreamDestroy(ctx->query_stream); }
    for (hipEvent_t e : {ctx->ev_world, ctx->ev_query}) if (e) (void)hipEventDestroy(e);
    if (ctx->q_host) (void)hipHostFree(ctx->q_host);
    if (ctx->q_dev) (void)hipFree(ctx->q_dev);
    for (StagingSet* s : {&ctx->slab_sets[0], &ctx->slab_sets[1], &ctx->edit_sets[0], &ctx->edit_sets[1]}) {
        for (hipEvent_t e : {s->ev_copied, s->ev_applied}) if (e) (void)hipEventDestroy(e);
        if (s->host) (void)hipHostFree(s->host);
        if (s->dev) (void)hipFree(s->dev);
    }
    for (void* p : ctx->allocs) (void)hipFree(p);
    for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->gather_ev) (void)hipEventDestroy(e);
    if (ctx->ev_frame0) (void)hipEventDestroy(ctx->ev_frame0);
    if (ctx->ev_frame1) (void)hipEventDestroy(ctx->ev_frame1);
    if (ctx->gather_stream) { (void)hipStreamSynchronize(ctx->gather_stream); (void)hipStreamDestroy(ctx->gather_stream); }
    for (int i = 0; i < 2; i++) { if (ctx->ev_ready[i]) (void)hipEventDestroy(ctx->ev_ready[i]); if (ctx->ev_free[i]) (void)hipEventDestroy(ctx->ev_free[i]); }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

int rt_set_stream(RtContext* ctx, void* hip_stream) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, sync_lanes(ctx));
    // NULL selects the context's own (non-blocking) stream, NOT the legacy null stream: work a caller enqueues on the null
    // stream is not ordered against the context's frames — pass an explicit stream handle to share one.
    // On a caller's stream EVERYTHING the context does runs on that stream, in order: no second lane, one frame slot (the
    // caller's own work on the stream is ordered against the frames by the stream alone).
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    ctx->lanes[0].stream = ctx->stream;
    ctx->user_stream = hip_stream != nullptr;
    ctx->accum_recorded = false;   // (everything before has finished)
    invalidate_prepass(ctx);       // (lanes and slots in use change with the stream)
    return RT_OK;
}

int rt_upload_world(RtContext* ctx, const uint32_t* materials, const uint8_t* minefield) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!materials || !minefield) return fail(ctx, RT_ERR_INVALID_ARG, "rt_upload_world: null pointer");
    ctx->accum_valid = false;
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
    ctx->world_recorded = false;   // (the region is complete on the device: reflatten synchronised)
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
    ctx->accum_valid = false;
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
    RT_HIP(ctx, staging_send(ctx, s, 5 * n));
    {
        LaunchTimer t(ctx, 1);
        RT_HIP(ctx, rtd::launch_flatten_slab(s.dev + 4 * n, reinterpret_cast<const uint32_t*>(s.dev), ctx->d_mine_sw, ctx->d_mat_sw,
                                             ctx->d_coarse, ctx->d_brick, ctx->logr, axis, texel_offset, ctx->stream));
    }
    RT_HIP(ctx, staging_applied(ctx, s));
    return RT_OK;
}

// ---- terrain on the device (rt_generate_world, rt_generate_slice) -------------------------------------------------------------
namespace {
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
    c->accum_valid = false;
    invalidate_prepass(c);
    RT_HIP(c, world_change_begin(c));
    {
        LaunchTimer t(c, 1);
        RT_HIP(c, rtd::launch_terrain(c->d_mine_sw, c->d_mat_sw, c->d_coarse, c->d_brick, c->d_heights, c->logr, seed, lo, axis, c->stream));
    }
    RT_HIP(c, world_change_end(c));
    return RT_OK;
}
}  // namespace

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

namespace {
size_t align16(size_t n) { return (n + 15u) & ~(size_t)15u; }
}  // namespace

int rt_edit_voxels(RtContext* ctx, const RtVoxelEdit* edits, uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (count > (1u << 24)) return fail(ctx, RT_ERR_INVALID_ARG, "rt_edit_voxels: more than 2^24 edits in one call; nothing was applied");
    if (count == 0) return RT_OK;
    if (!edits) return fail(ctx, RT_ERR_INVALID_ARG, "rt_edit_voxels: null edits");
    if (!ctx->world_resident) return fail(ctx, RT_ERR_NOT_READY, "rt_edit_voxels: upload the full region first");
    // Binning on the host, all of it before anything is enqueued: validate every edit, then one stable counting pass by chunk.
    const uint32_t R = (uint32_t)ctx->region;
    const int nl = ctx->logr - 6;
    const uint32_t nchunks = 1u << (3 * nl);
    std::vector<uint32_t>& chunk = ctx->edit_chunk;
    std::vector<uint32_t>& start = ctx->edit_start;
    chunk.resize(count);
    start.assign((size_t)nchunks + 1u, 0u);
    for (uint32_t i = 0; i < count; i++) {
        const RtVoxelEdit& e = edits[i];
        if (e.x >= R || e.y >= R || e.z >= R || e.reserved != 0u)
            return fail(ctx, RT_ERR_INVALID_ARG, "rt_edit_voxels: edit " + std::to_string(i) +
                                                     " has a coordinate outside the region or reserved != 0; nothing was applied");
        const uint32_t c = ((uint32_t)(e.z >> 6) << (2 * nl)) | ((uint32_t)(e.y >> 6) << nl) | (uint32_t)(e.x >> 6);
        chunk[i] = c;
        start[c + 1u]++;
    }
    uint32_t touched = 0;
    for (uint32_t c = 0; c < nchunks; c++) { touched += start[c + 1u] != 0u; start[c + 1u] += start[c]; }
    std::vector<uint32_t>& order = ctx->edit_order;   // edit indices grouped by chunk, batch order within a chunk
    order.resize(count);
    for (uint32_t i = 0; i < count; i++) order[start[chunk[i]]++] = i;   // afterwards start[c] = end of chunk c's range
    const size_t off_offs = align16((size_t)touched * 4u), off_recs = off_offs + align16(((size_t)touched + 1u) * 4u);
    const size_t need = off_recs + (size_t)count * 8u;

    RT_HIP(ctx, hipSetDevice(ctx->device));
    StagingSet& s = ctx->edit_sets[ctx->edit_batches & 1u];
    size_t cap = need < ((size_t)64 << 10) ? ((size_t)64 << 10) : need;   // (if the set must grow)
    if (cap < need + need / 2u) cap = align16(need + need / 2u);
    RT_HIP(ctx, staging_claim(ctx, s, need, cap));
    // Staging: touched chunk ids, their edit ranges, and per chunk one record per edited voxel — its last edit in the batch (the
    // range is walked backwards; edit_stamp marks the voxels a chunk's run has kept).
    uint8_t* h = s.host;
    uint32_t* h_chunks = reinterpret_cast<uint32_t*>(h);
    uint32_t* h_offs = reinterpret_cast<uint32_t*>(h + off_offs);
    uint32_t* h_recs = reinterpret_cast<uint32_t*>(h + off_recs);
    std::vector<uint32_t>& stamp = ctx->edit_stamp;
    if (stamp.size() != (size_t)RT_CHUNK_SIZE * RT_CHUNK_SIZE * RT_CHUNK_SIZE) stamp.assign((size_t)RT_CHUNK_SIZE * RT_CHUNK_SIZE * RT_CHUNK_SIZE, 0u);
    uint32_t t = 0, nrec = 0;
    for (uint32_t c = 0; c < nchunks; c++) {
        const uint32_t b = c ? start[c - 1u] : 0u, e = start[c];
        if (b == e) continue;
        if (++ctx->edit_gen == 0u) { std::fill(stamp.begin(), stamp.end(), 0u); ctx->edit_gen = 1u; }
        const uint32_t gen = ctx->edit_gen;
        h_chunks[t] = c;
        h_offs[t++] = nrec;
        for (uint32_t j = e; j-- > b;) {
            const RtVoxelEdit& ed = edits[order[j]];
            const uint32_t local = ((uint32_t)(ed.z & 63u) << 12) | ((uint32_t)(ed.y & 63u) << 6) | (uint32_t)(ed.x & 63u);
            if (stamp[local] == gen) continue;
            stamp[local] = gen;
            h_recs[2u * nrec] = local | (ed.solid ? 1u << 18 : 0u);
            h_recs[2u * nrec + 1u] = ed.material;
            nrec++;
        }
    }
    h_offs[t] = nrec;
    // Transfer on the upload stream, then the rebuild on the render stream after the frames already submitted (every lane), and
    // later frames after the rebuild — the ordering of rt_upload_slice.
    ctx->edit_batches++;
    ctx->accum_valid = false;
    invalidate_prepass(ctx);
    RT_HIP(ctx, staging_send(ctx, s, off_recs + (size_t)nrec * 8u));
    const uint32_t* d_chunks = reinterpret_cast<const uint32_t*>(s.dev);
    const uint32_t* d_offs = reinterpret_cast<const uint32_t*>(s.dev + off_offs);
    const uint2* d_recs = reinterpret_cast<const uint2*>(s.dev + off_recs);
    {
        LaunchTimer lt(ctx, 1);
        RT_HIP(ctx, rtd::launch_rebuild_chunks(ctx->d_mine_sw, ctx->d_mat_sw, d_chunks, d_offs, d_recs, touched, ctx->logr, ctx->stream));
    }
    {
        LaunchTimer lt(ctx, 1);
        RT_HIP(ctx, rtd::launch_rebuild_chunk_maps(ctx->d_mine_sw, ctx->d_coarse, ctx->d_brick, d_chunks, touched, ctx->logr, ctx->stream));
    }
    RT_HIP(ctx, staging_applied(ctx, s));
    return RT_OK;
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

// ---- ray queries ----------------------------------------------------------------------------------------------------------------
namespace {
constexpr uint32_t kMaxQueryRays = 1u << 26;

// checks shared by the three calls; returns RT_OK when there is work to enqueue, 1 for count == 0
int query_check(RtContext* c, const char* fn, uint32_t count, const void* in, const void* more, const void* out) {
    if (count > kMaxQueryRays) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": more than 2^26 rays in one call");
    if (count == 0) return 1;
    if (!in || !more || !out) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": null pointer");
    if (!c->world_resident) return fail(c, RT_ERR_NOT_READY, std::string(fn) + ": upload the full region first");
    return RT_OK;
}

// The stream a query runs on, after the world changes before it: the context's query stream (not ordered after the frames), or the
// caller's stream after rt_set_stream(non-NULL).
int query_stream_of(RtContext* c, hipStream_t* st) {
    RT_HIP(c, hipSetDevice(c->device));
    if (!c->query_stream) {
        int least = 0, greatest = 0;
        RT_HIP(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
        RT_HIP(c, hipStreamCreateWithPriority(&c->query_stream, hipStreamNonBlocking, greatest));
    }
    if (c->user_stream) { *st = c->stream; return RT_OK; }
    *st = c->query_stream;
    if (c->world_recorded) RT_HIP(c, hipStreamWaitEvent(*st, c->ev_world, 0));
    return RT_OK;
}

int query_launch(RtContext* c, hipStream_t st, const rtd::Frame& f, const void* rays_dev, const void* xy_dev, void* hits_dev, uint32_t count) {
    rtd::QueryArgs a;
    a.rays = reinterpret_cast<const float4*>(rays_dev);
    a.xy = reinterpret_cast<const int2*>(xy_dev);
    a.hits = reinterpret_cast<uint4*>(hits_dev);
    a.count = count;
    RT_HIP(c, rtd::launch_query(scene_of(c), f, a, st));
    if (!c->user_stream) { RT_HIP(c, hipEventRecord(c->ev_query, st)); c->query_recorded = true; }   // (a caller's stream orders itself)
    return RT_OK;
}

// rt_trace_rays_async's pointers: 16-byte aligned (the kernel's float4 / uint4 accesses) and memory of the context's device (or
// managed memory).  A host address would fault the kernel: pageable memory is not mapped for the device with XNACK off.
bool query_device_ptr(const RtContext* c, const void* p) {
    if (((uintptr_t)p & 15u) != 0u) return false;
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // (clears the error it set)
    if (a.type == hipMemoryTypeManaged || a.isManaged) return true;
    return a.type == hipMemoryTypeDevice && a.device == c->device;
}

rtd::Frame query_frame(const RtContext* c, const int32_t lr[3]) {
    RtUniforms u{};
    for (int k = 0; k < 3; k++) u.lr[k] = lr[k];
    return frame_of(c, &u);
}

// The synchronous calls: `in_bytes` of input through pinned and device staging, the launch, the hits back; waits for them.
int query_sync(RtContext* c, const rtd::Frame& f, const void* in, size_t in_bytes, bool picks, RtRayHit* hits, uint32_t count) {
    hipStream_t st;
    int rc = query_stream_of(c, &st);
    if (rc != RT_OK) return rc;
    const size_t off = align16(in_bytes), need = off + (size_t)count * sizeof(RtRayHit);
    if (need > c->q_cap) {   // the previous synchronous call has finished with the staging (it waited for its hits)
        if (c->q_host) { (void)hipHostFree(c->q_host); c->q_host = nullptr; }
        if (c->q_dev) { (void)hipFree(c->q_dev); c->q_dev = nullptr; c->device_bytes -= c->q_cap; }
        c->q_cap = 0;
        const size_t cap = need < ((size_t)64 << 10) ? ((size_t)64 << 10) : align16(need + need / 2u);
        RT_HIP(c, hipHostMalloc((void**)&c->q_host, cap, hipHostMallocDefault));
        RT_HIP(c, hipMalloc((void**)&c->q_dev, cap));
        c->q_cap = cap;
        c->device_bytes += cap;
    }
    memcpy(c->q_host, in, in_bytes);
    RT_HIP(c, hipMemcpyAsync(c->q_dev, c->q_host, in_bytes, hipMemcpyHostToDevice, st));
    rc = query_launch(c, st, f, picks ? nullptr : c->q_dev, picks ? c->q_dev : nullptr, c->q_dev + off, count);
    if (rc != RT_OK) return rc;
    RT_HIP(c, hipMemcpyAsync(c->q_host + off, c->q_dev + off, (size_t)count * sizeof(RtRayHit), hipMemcpyDeviceToHost, st));
    RT_HIP(c, hipStreamSynchronize(st));
    memcpy(hits, c->q_host + off, (size_t)count * sizeof(RtRayHit));
    return RT_OK;
}
}  // namespace

int rt_trace_rays(RtContext* ctx, const RtRay* rays, uint32_t count, const int32_t lr[3], RtRayHit* hits) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = query_check(ctx, "rt_trace_rays", count, rays, lr, hits);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    return query_sync(ctx, query_frame(ctx, lr), rays, (size_t)count * sizeof(RtRay), false, hits, count);
}

int rt_trace_rays_async(RtContext* ctx, const RtRay* rays_dev, uint32_t count, const int32_t lr[3], RtRayHit* hits_dev) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = query_check(ctx, "rt_trace_rays_async", count, rays_dev, lr, hits_dev);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!query_device_ptr(ctx, rays_dev) || !query_device_ptr(ctx, hits_dev))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_trace_rays_async: rays and hits must be 16-byte aligned memory of the context's device");
    hipStream_t st;
    rc = query_stream_of(ctx, &st);
    if (rc != RT_OK) return rc;
    return query_launch(ctx, st, query_frame(ctx, lr), rays_dev, nullptr, hits_dev, count);
}

int rt_pick_pixels(RtContext* ctx, const RtUniforms* u, const int32_t* xy, uint32_t count, RtRayHit* hits) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = query_check(ctx, "rt_pick_pixels", count, u, xy, hits);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    for (uint32_t i = 0; i < count; i++)
        if (xy[2 * i] < 0 || xy[2 * i] >= ctx->cfg.width || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= ctx->cfg.height)
            return fail(ctx, RT_ERR_INVALID_ARG, "rt_pick_pixels: pixel " + std::to_string(i) + " is outside the frame");
    return query_sync(ctx, frame_of(ctx, u), xy, (size_t)count * 8u, true, hits, count);
}

int rt_upload_noise(RtContext* ctx, const uint8_t* rgba8) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!rgba8) return fail(ctx, RT_ERR_INVALID_ARG, "rt_upload_noise: null pointer");
    ctx->accum_valid = false;
    invalidate_prepass(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, sync_lanes(ctx));
    RT_HIP(ctx, hipMemcpy(ctx->d_noise, rgba8, RT_NOISE_BYTES, hipMemcpyHostToDevice));
    ctx->has_noise = true;
    return RT_OK;
}

int rt_draw_frame(RtContext* ctx, const RtUniforms* u) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!u) return fail(ctx, RT_ERR_INVALID_ARG, "rt_draw_frame: null uniforms");
    if (!ctx->has_world || !ctx->has_noise) return fail(ctx, RT_ERR_NOT_READY, "rt_draw_frame: world and noise must be uploaded first");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const rtd::Frame f = frame_of(ctx, u);
    const bool count = (ctx->cfg.flags & RT_FLAG_COUNTERS) != 0;
    // frame_ms of rt_get_timing: two events per frame, recorded only for a context that asked for every timing — an event between
    // the last kernel of one frame and the first of the next is 4-5 us during which the GPU idles (profiles/r3_frame_timeline.txt)
    const bool frame_events = (ctx->cfg.flags & RT_FLAG_TIMING_ALL) == RT_FLAG_TIMING_ALL;
    int rc = RT_OK;
    if (ctx->route.family == RT_KERNEL_MEGA) {
        if (frame_events) RT_HIP(ctx, hipEventRecord(ctx->ev_frame0, ctx->stream));
        LaunchTimer t(ctx, 0);
        hipError_t e = rtd::launch_mega(scene_of(ctx), f, planes_of(ctx), ctx->d_counters, count, ctx->stream);
        if (e != hipSuccess) rc = fail(ctx, RT_ERR_HIP, std::string("launch_mega: ") + hipGetErrorString(e));
    } else if (ctx->route.family == RT_KERNEL_PERSISTENT) {
        rc = draw_persistent(ctx, f, u, frame_events);
    } else {
        if (frame_events) RT_HIP(ctx, hipEventRecord(ctx->ev_frame0, ctx->stream));
        rc = draw_wavefront(ctx, f);
    }
    if (frame_events) RT_HIP(ctx, hipEventRecord(ctx->ev_frame1, ctx->stream));
    ctx->frame_recorded = true;
    if (rc == RT_OK) ctx->drawn = true;
    if (count) { ctx->host_noise_base += (uint64_t)ctx->cfg.spp; ctx->host_frames++; }
    return rc;
}

int rt_reset_accumulation(RtContext* ctx) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    ctx->accum_valid = false;
    return RT_OK;
}

int rt_get_accumulation(RtContext* ctx, uint32_t* frames, uint32_t* samples) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!frames || !samples) return fail(ctx, RT_ERR_INVALID_ARG, "rt_get_accumulation: null pointer");
    if (!ctx->drawn) { *frames = 0; *samples = 0; }
    else if (ctx->d_accum) { *frames = (uint32_t)ctx->accum_frames; *samples = (uint32_t)ctx->accum_samples; }
    else { *frames = 1; *samples = (uint32_t)ctx->cfg.spp; }
    return RT_OK;
}

int rt_read_history(RtContext* ctx, uint32_t* counts, size_t bytes) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!ctx->reproject) return fail(ctx, RT_ERR_INVALID_ARG, "rt_read_history: the context was created without RT_FLAG_REPROJECT");
    const size_t npix = (size_t)ctx->cfg.width * (size_t)ctx->cfg.height;
    if (!counts || bytes != npix * sizeof(uint32_t)) return fail(ctx, RT_ERR_INVALID_ARG, "rt_read_history: null destination or size mismatch");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, sync_lanes(ctx));
    std::vector<uint2> rec(npix);
    RT_HIP(ctx, hipMemcpy(rec.data(), ctx->d_hist_rec[ctx->hist_cur], npix * sizeof(uint2), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < npix; i++) counts[i] = rec[i].y & ((1u << 27) - 1u);
    return RT_OK;
}

int rt_sync(RtContext* ctx) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, sync_lanes(ctx));
    if (ctx->gather_stream) RT_HIP(ctx, hipStreamSynchronize(ctx->gather_stream));
    return RT_OK;
}

size_t rt_buffer_bytes(RtContext* ctx, int id) {
    if (!ctx || id < 0 || id >= RT_BUF_COUNT) return 0;
    return ctx->plane_pixels * kBytesPerPixel[id];
}

void* rt_device_ptr(RtContext* ctx, int id) {
    if (!ctx || id < 0 || id >= RT_BUF_COUNT) return nullptr;
    return ctx->planes[id];
}

int rt_readback(RtContext* ctx, int id, void* dst, size_t bytes) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (id < 0 || id >= RT_BUF_COUNT || !dst) return fail(ctx, RT_ERR_INVALID_ARG, "rt_readback: bad buffer id or null destination");
    if (bytes != rt_buffer_bytes(ctx, id)) return fail(ctx, RT_ERR_INVALID_ARG, "rt_readback: size mismatch");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RT_HIP(ctx, hipMemcpy(dst, ctx->planes[id], bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_tile_count(RtContext* ctx) { return ctx ? ctx->ntiles_local : RT_ERR_INVALID_ARG; }
int rt_tile_capacity(RtContext* ctx) { return ctx ? ctx->tile_capacity : RT_ERR_INVALID_ARG; }

int rt_untile(RtContext* ctx, int id, const void* gathered_dev, int world, void* frame_dev) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (id < 0 || id >= RT_BUF_COUNT || !gathered_dev || !frame_dev || world < 1)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_untile: bad argument");
    plane_written(ctx, frame_dev);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const int capacity = (ctx->ntiles_total + world - 1) / world;
    RT_HIP(ctx, rtd::launch_untile(gathered_dev, frame_dev, world, capacity, ctx->tiles_x, ctx->tiles_y, ctx->cfg.width,
                                   ctx->cfg.height, (int)kBytesPerPixel[id], ctx->stream));
    return RT_OK;
}

int rt_denoise_planes(RtContext* ctx, void* lighting, const void* depth, const void* normal, int faithful) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!lighting || !depth || !normal) return fail(ctx, RT_ERR_INVALID_ARG, "rt_denoise_planes: null plane");
    plane_written(ctx, lighting);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const int sizes[6] = {1, 2, 4, 8, 8, 16};                         // pipeline.rs:103
    const int W = ctx->cfg.width, H = ctx->cfg.height;
    void** work = ctx->slots[ctx->cur_slot].denoise_work;   // per slot: the post passes of two frames in flight may overlap
    for (int i = 0; i < 2; i++)
        if (!work[i]) { uint4* p = nullptr; RT_HIP(ctx, dev_alloc(ctx, &p, (size_t)W * H)); work[i] = p; }
    {
        LaunchTimer t(ctx, 1);
        RT_HIP(ctx, rtd::launch_denoise_prepare(lighting, depth, normal, W, H, work[0], ctx->stream));
    }
    for (int pass = 0; pass < 6; pass++) {
        // pipeline.rs:104-108: the ping descriptor set on even dispatches, the pong set (normal/depth bindings swapped,
        // descriptor_sets.rs:38-39) on odd ones; the sixth dispatch writes the lighting image finalize.comp reads
        const bool odd = pass % 2 == 1;
        LaunchTimer t(ctx, 1);
        RT_HIP(ctx, rtd::launch_denoise(work[pass & 1], W, H, sizes[pass], odd && faithful != 0, pass == 5,
                                        work[(pass & 1) ^ 1], lighting, ctx->stream));
    }
    return RT_OK;
}

int rt_finalize_planes(RtContext* ctx, const void* albedo, const void* emission, const void* fog, const void* lighting,
                       const void* depth, void* out_bgra8) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!albedo || !emission || !fog || !lighting || !depth || !out_bgra8) return fail(ctx, RT_ERR_INVALID_ARG, "rt_finalize_planes: null plane");
    if (!ctx->has_noise) return fail(ctx, RT_ERR_NOT_READY, "rt_finalize_planes: noise must be uploaded first");
    plane_written(ctx, out_bgra8);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    LaunchTimer t(ctx, 1);
    RT_HIP(ctx, rtd::launch_finalize(albedo, emission, fog, lighting, depth, ctx->d_noise, ctx->cfg.width, ctx->cfg.height, out_bgra8,
                                     ctx->stream));
    return RT_OK;
}

int rt_denoise(RtContext* ctx, int faithful) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (ctx->cfg.tile_world != 1) return fail(ctx, RT_ERR_UNIMPLEMENTED, "rt_denoise: whole-frame contexts only (gather the tiles, then rt_denoise_planes)");
    if (!ctx->frame_recorded) return fail(ctx, RT_ERR_NOT_READY, "rt_denoise: no frame drawn yet");
    return rt_denoise_planes(ctx, ctx->planes[RT_BUF_LIGHTING_RGBA16], ctx->planes[RT_BUF_DEPTH_R16UI], ctx->planes[RT_BUF_NORMAL_R8UI], faithful);
}

int rt_finalize(RtContext* ctx) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (ctx->cfg.tile_world != 1) return fail(ctx, RT_ERR_UNIMPLEMENTED, "rt_finalize: whole-frame contexts only (gather the tiles, then rt_finalize_planes)");
    if (!ctx->frame_recorded) return fail(ctx, RT_ERR_NOT_READY, "rt_finalize: no frame drawn yet");
    return rt_finalize_planes(ctx, ctx->planes[RT_BUF_ALBEDO_RGBA8], ctx->planes[RT_BUF_EMISSION_RGBA8], ctx->planes[RT_BUF_FOG_RGBA8],
                              ctx->planes[RT_BUF_LIGHTING_RGBA16], ctx->planes[RT_BUF_DEPTH_R16UI], ctx->planes[RT_BUF_FINAL_BGRA8]);
}

void* rt_gbuffer_ptr(RtContext* ctx) { return ctx ? ctx->gbuffer : nullptr; }
size_t rt_gbuffer_bytes(RtContext* ctx) { return ctx ? ctx->gbuffer_bytes : 0; }
size_t rt_gbuffer_offset(RtContext* ctx, int id) {
    if (!ctx || id < 0 || id > RT_BUF_FOG_RGBA8) return 0;
    return ctx->gbuffer_offset[id];
}

int rt_untile_gbuffer(RtContext* ctx, const void* gathered_dev, int world, void* const* frames_dev) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!gathered_dev || !frames_dev || world < 1) return fail(ctx, RT_ERR_INVALID_ARG, "rt_untile_gbuffer: bad argument");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    // the per-rank block layout (plane offsets, block size) is this context's own: only valid for its own split
    if (world != ctx->cfg.tile_world || world < 2)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_untile_gbuffer: world must equal the context's tile_world (>= 2)");
    const int capacity = (ctx->ntiles_total + world - 1) / world;
    for (int b = 0; b <= RT_BUF_FOG_RGBA8; b++) {
        if (!frames_dev[b]) continue;
        RT_HIP(ctx, rtd::launch_untile_strided((const uint8_t*)gathered_dev + ctx->gbuffer_offset[b], ctx->gbuffer_bytes, frames_dev[b], world,
                                               capacity, ctx->tiles_x, ctx->tiles_y, ctx->cfg.width, ctx->cfg.height,
                                               (int)kBytesPerPixel[b], ctx->stream));
    }
    return RT_OK;
}


// ---- multi-GPU: RCCL gather of the tile-split G-buffer ------------------------------------------------------
namespace {
struct Rccl {
    void* handle = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string error;
};
Rccl g_rccl;
std::once_flag g_rccl_once;

// librccl is 0.5 GB: loaded on first use only.  A copy the process already holds (e.g. the one PyTorch ships) is reused,
// so a communicator created by the host's own RCCL stays valid here.
bool rccl_load() {
    std::call_once(g_rccl_once, [] {
        const char* names[] = {"librccl.so.1", "librccl.so"};
        for (const char* n : names) { if (!g_rccl.handle) g_rccl.handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD); }
        for (const char* n : names) { if (!g_rccl.handle) g_rccl.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL); }
        if (!g_rccl.handle) { g_rccl.error = std::string("cannot load librccl: ") + dlerror(); return; }
#define RT_RCCL_SYM(name) g_rccl.name = (decltype(g_rccl.name))dlsym(g_rccl.handle, "nccl" #name); if (!g_rccl.name) g_rccl.error = "librccl lacks nccl" #name;
        RT_RCCL_SYM(GetUniqueId) RT_RCCL_SYM(CommInitRank) RT_RCCL_SYM(CommInitAll) RT_RCCL_SYM(CommDestroy) RT_RCCL_SYM(GroupStart)
        RT_RCCL_SYM(GroupEnd) RT_RCCL_SYM(Send) RT_RCCL_SYM(Recv) RT_RCCL_SYM(GetErrorString)
#undef RT_RCCL_SYM
    });
    return g_rccl.error.empty();
}
#define RT_NCCL(ctx, call)                                                                                   \
    do { ncclResult_t r_ = (call); if (r_ != ncclSuccess)                                                    \
        return fail(ctx, RT_ERR_HIP, std::string(#call) + ": " + g_rccl.GetErrorString(r_)); } while (0)
}  // namespace

int rt_comm_unique_id(void* id_out, size_t bytes) {
    if (!id_out || bytes != NCCL_UNIQUE_ID_BYTES) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_comm_unique_id: need a 128-byte buffer");
    if (!rccl_load()) return fail(nullptr, RT_ERR_UNIMPLEMENTED, g_rccl.error);
    ncclUniqueId id;
    RT_NCCL(nullptr, g_rccl.GetUniqueId(&id));
    memcpy(id_out, &id, sizeof(id));
    return RT_OK;
}

int rt_comm_init_rank(RtContext* ctx, const void* id, size_t bytes, void** comm_out) {
    if (comm_out) *comm_out = nullptr;
    if (!ctx || !id || bytes != NCCL_UNIQUE_ID_BYTES || !comm_out) return fail(ctx, RT_ERR_INVALID_ARG, "rt_comm_init_rank: bad argument");
    if (!rccl_load()) return fail(ctx, RT_ERR_UNIMPLEMENTED, g_rccl.error);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    ncclComm_t comm = nullptr;
    RT_NCCL(ctx, g_rccl.CommInitRank(&comm, ctx->cfg.tile_world, uid, ctx->cfg.tile_rank));
    *comm_out = comm;
    return RT_OK;
}

int rt_comm_init_all(int ndev, const int* devices, void** comms_out) {
    if (ndev < 1 || !comms_out) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_comm_init_all: bad argument");
    if (!rccl_load()) return fail(nullptr, RT_ERR_UNIMPLEMENTED, g_rccl.error);
    std::vector<ncclComm_t> comms((size_t)ndev, nullptr);
    RT_NCCL(nullptr, g_rccl.CommInitAll(comms.data(), ndev, devices));
    for (int i = 0; i < ndev; i++) comms_out[i] = comms[(size_t)i];
    return RT_OK;
}

int rt_comm_destroy(void* comm) {
    if (!comm) return RT_OK;
    if (!rccl_load()) return fail(nullptr, RT_ERR_UNIMPLEMENTED, g_rccl.error);
    RT_NCCL(nullptr, g_rccl.CommDestroy((ncclComm_t)comm));
    return RT_OK;
}

int rt_gather_gbuffer(RtContext* ctx, void* comm_, int root, void* const* frames_dev, int overlapped) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const int world = ctx->cfg.tile_world, rank = ctx->cfg.tile_rank;
    if (root < 0 || root >= world) return fail(ctx, RT_ERR_INVALID_ARG, "rt_gather_gbuffer: root out of range");
    if (!ctx->frame_recorded) return fail(ctx, RT_ERR_NOT_READY, "rt_gather_gbuffer: no frame drawn yet");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (rank == root && !frames_dev) {
        // no caller-owned planes: assemble into the library's own (allocated once; rt_frame_ptr / rt_frame_readback)
        for (int b = 0; b <= RT_BUF_FOG_RGBA8; b++)
            if (!ctx->frame_planes[b]) {
                uint8_t* p = nullptr;
                RT_HIP(ctx, dev_alloc(ctx, &p, (size_t)ctx->cfg.width * ctx->cfg.height * kBytesPerPixel[b]));
                ctx->frame_planes[b] = p;
            }
        frames_dev = ctx->frame_planes;
    }
    if (world == 1 && !comm_) {
        // one context holds the whole frame, row-major already: plain copies on the stream the frame ended on, after the previous
        // frame's copies (which sit on the other lane's stream when two frames are in flight)
        if (ctx->gather_recorded) RT_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_gather, 0));
        for (int b = 0; b <= RT_BUF_FOG_RGBA8; b++)
            if (frames_dev[b]) RT_HIP(ctx, hipMemcpyAsync(frames_dev[b], ctx->planes[b], ctx->plane_pixels * kBytesPerPixel[b], hipMemcpyDeviceToDevice, ctx->stream));
        RT_HIP(ctx, hipEventRecord(ctx->ev_gather, ctx->stream)); ctx->gather_recorded = true;
        return RT_OK;
    }
    if (!comm_) return fail(ctx, RT_ERR_INVALID_ARG, "rt_gather_gbuffer: null communicator");
    if (!rccl_load()) return fail(ctx, RT_ERR_UNIMPLEMENTED, g_rccl.error);
    ncclComm_t comm = (ncclComm_t)comm_;
    const size_t gb = ctx->gbuffer_bytes;
    const int s = overlapped ? (int)(ctx->gathers & 1u) : 0;
    if (rank == root && !ctx->gathered[s]) RT_HIP(ctx, dev_alloc(ctx, &ctx->gathered[s], gb * (size_t)world));
    hipStream_t gs = ctx->stream;
    const uint8_t* src = (const uint8_t*)ctx->gbuffer;
    // gathers share the root's staging and the communicator: with two frames in flight the previous frame's gather sits on the
    // other lane's stream — this one follows it (the frames' rendering still overlaps)
    if (!overlapped && ctx->gather_recorded) RT_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_gather, 0));
    if (overlapped) {
        // The frame's block is copied to one of two staging buffers on the render stream (so the next frame may overwrite the
        // planes), everything else runs on a second stream: frame k's send/recv + un-tile overlap frame k+1's kernels.
        if (!ctx->gather_stream) RT_HIP(ctx, hipStreamCreateWithFlags(&ctx->gather_stream, hipStreamNonBlocking));
        for (int i = 0; i < 2; i++) {
            if (!ctx->ev_ready[i]) RT_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_ready[i], hipEventDisableTiming));
            if (!ctx->ev_free[i]) RT_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_free[i], hipEventDisableTiming));
        }
        if (!ctx->stage[s]) RT_HIP(ctx, dev_alloc(ctx, &ctx->stage[s], gb));
        if (ctx->ev_free_recorded[s]) RT_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_free[s], 0));   // gather k-2 has left stage[s]
        RT_HIP(ctx, hipMemcpyAsync(ctx->stage[s], ctx->gbuffer, gb, hipMemcpyDeviceToDevice, ctx->stream));
        RT_HIP(ctx, hipEventRecord(ctx->ev_ready[s], ctx->stream));
        RT_HIP(ctx, hipStreamWaitEvent(ctx->gather_stream, ctx->ev_ready[s], 0));
        gs = ctx->gather_stream;
        src = ctx->stage[s];
    }
    // RT_FLAG_TIMING: events round the transfer + un-tile on the stream they run on (rt_get_gather_timing)
    size_t gev = (size_t)-1;
    if ((ctx->cfg.flags & RT_FLAG_TIMING) != 0 && ctx->gather_ev_used + 2 <= 2 * 4096) {
        while (ctx->gather_ev.size() < ctx->gather_ev_used + 2) { hipEvent_t ev; RT_HIP(ctx, hipEventCreate(&ev)); ctx->gather_ev.push_back(ev); }
        gev = ctx->gather_ev_used; ctx->gather_ev_used += 2;
        RT_HIP(ctx, hipEventRecord(ctx->gather_ev[gev], gs));
    }
    // every rank sends its block to the root; the root posts one receive per rank (its own block included).  Each peer uses
    // its own xGMI link into the root, so the transfers run in parallel.
    RT_NCCL(ctx, g_rccl.GroupStart());
    {   // a failing call must not leave the group open: the group is always closed, the first error is reported
        ncclResult_t first = ncclSuccess;
        const char* what = "";
        if (rank == root)
            for (int r = 0; r < world && first == ncclSuccess; r++) {
                first = g_rccl.Recv(ctx->gathered[s] + (size_t)r * gb, gb, ncclUint8, r, comm, gs);
                what = "ncclRecv";
            }
        if (first == ncclSuccess) { first = g_rccl.Send(src, gb, ncclUint8, root, comm, gs); what = "ncclSend"; }
        const ncclResult_t end = g_rccl.GroupEnd();
        if (first == ncclSuccess && end != ncclSuccess) { first = end; what = "ncclGroupEnd"; }
        if (first != ncclSuccess) return fail(ctx, RT_ERR_HIP, std::string("rt_gather_gbuffer: ") + what + ": " + g_rccl.GetErrorString(first));
    }
    if (rank == root) {
        const int capacity = (ctx->ntiles_total + world - 1) / world;
        for (int b = 0; b <= RT_BUF_FOG_RGBA8; b++) {
            if (!frames_dev[b]) continue;
            if (world == 1) {   // a one-rank communicator (the transfer went to itself): the block holds row-major planes
                RT_HIP(ctx, hipMemcpyAsync(frames_dev[b], ctx->gathered[s] + ctx->gbuffer_offset[b], ctx->plane_pixels * kBytesPerPixel[b],
                                           hipMemcpyDeviceToDevice, gs));
                continue;
            }
            RT_HIP(ctx, rtd::launch_untile_strided(ctx->gathered[s] + ctx->gbuffer_offset[b], gb, frames_dev[b], world, capacity, ctx->tiles_x,
                                                   ctx->tiles_y, ctx->cfg.width, ctx->cfg.height, (int)kBytesPerPixel[b], gs));
        }
    }
    if (gev != (size_t)-1) RT_HIP(ctx, hipEventRecord(ctx->gather_ev[gev + 1], gs));
    if (overlapped) { RT_HIP(ctx, hipEventRecord(ctx->ev_free[s], gs)); ctx->ev_free_recorded[s] = true; }
    else { RT_HIP(ctx, hipEventRecord(ctx->ev_gather, gs)); ctx->gather_recorded = true; }
    ctx->gathers++;
    return RT_OK;
}

int rt_get_gather_timing(RtContext* ctx, float* ms_sum, uint32_t* calls) {
    if (!ctx || !ms_sum || !calls) return RT_ERR_INVALID_ARG;
    *ms_sum = 0.0f; *calls = 0;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, sync_lanes(ctx));
    if (ctx->gather_stream) RT_HIP(ctx, hipStreamSynchronize(ctx->gather_stream));
    for (size_t i = 0; i + 1 < ctx->gather_ev_used; i += 2) {
        float ms = 0.0f;
        RT_HIP(ctx, hipEventElapsedTime(&ms, ctx->gather_ev[i], ctx->gather_ev[i + 1]));
        *ms_sum += ms; (*calls)++;
    }
    ctx->gather_ev_used = 0;
    return RT_OK;
}

int rt_selftest(RtContext* ctx, int which, uint64_t* result) {
    if (!ctx || !result) return RT_ERR_INVALID_ARG;
    if (which != RT_SELFTEST_DENOISE_DIVISION && which != RT_SELFTEST_SCENE_MAPS) return fail(ctx, RT_ERR_INVALID_ARG, "rt_selftest: unknown test");
    if (which == RT_SELFTEST_SCENE_MAPS && !ctx->world_resident) return fail(ctx, RT_ERR_NOT_READY, "rt_selftest: no region uploaded");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->d_selftest) RT_HIP(ctx, dev_alloc(ctx, &ctx->d_selftest, 1));   // one word, allocated once
    unsigned long long* d = ctx->d_selftest;
    RT_HIP(ctx, hipMemsetAsync(d, 0, sizeof(*d), ctx->stream));
    if (which == RT_SELFTEST_DENOISE_DIVISION) RT_HIP(ctx, rtd::launch_selftest_dn_div(d, ctx->stream));
    else RT_HIP(ctx, rtd::launch_check_maps(ctx->d_mine_sw, ctx->d_coarse, ctx->d_brick, ctx->logr, d, ctx->stream));
    unsigned long long h = 0;
    RT_HIP(ctx, hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *result = h;
    return RT_OK;
}

void* rt_frame_ptr(RtContext* ctx, int id) {
    if (!ctx || id < 0 || id > RT_BUF_FOG_RGBA8) return nullptr;
    return ctx->frame_planes[id];
}

int rt_frame_readback(RtContext* ctx, int id, void* dst, size_t bytes) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (id < 0 || id > RT_BUF_FOG_RGBA8 || !dst) return fail(ctx, RT_ERR_INVALID_ARG, "rt_frame_readback: bad buffer id or null destination");
    if (!ctx->frame_planes[id]) return fail(ctx, RT_ERR_NOT_READY, "rt_frame_readback: no frame assembled by rt_gather_gbuffer(frames_dev = NULL) yet");
    if (bytes != (size_t)ctx->cfg.width * ctx->cfg.height * kBytesPerPixel[id]) return fail(ctx, RT_ERR_INVALID_ARG, "rt_frame_readback: size mismatch");
    int rc = rt_sync(ctx);
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipMemcpy(dst, ctx->frame_planes[id], bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_get_info(RtContext* ctx, RtInfo* out) {
    if (!ctx || !out) return RT_ERR_INVALID_ARG;
    if (out->struct_size != sizeof(RtInfo)) return fail(ctx, RT_ERR_INVALID_ARG, "rt_get_info: RtInfo.struct_size mismatch");
    out->num_cus = ctx->num_cus;
    const bool persistent = ctx->route.family == RT_KERNEL_PERSISTENT;
    out->samples_per_launch = persistent ? ctx->persist_batch : ctx->batch_samples;
    out->launches_in_flight = (uint16_t)(ctx->user_stream ? 1 : ctx->nlanes);
    out->frames_in_flight = (uint16_t)(ctx->user_stream ? 1 : ctx->nslots);
    out->light_record_budget_bytes = ctx->light_budget_bytes;
    out->light_record_bytes = persistent
        ? (uint64_t)sizeof(rtd::PathLight) * (ctx->npix_pad ? ctx->npix_pad : 1) * ctx->persist_batch * (uint64_t)ctx->nlanes : 0;
    out->device_bytes = ctx->device_bytes;
    return RT_OK;
}

int rt_kernel_in_use(RtContext* ctx) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    return ctx->route.in_use;
}

int rt_get_counters(RtContext* ctx, RtCounters* out) {
    if (!ctx || !out) return RT_ERR_INVALID_ARG;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, sync_lanes(ctx));
    rtd::DevCounters d;
    RT_HIP(ctx, hipMemcpy(&d, ctx->d_counters, sizeof(d), hipMemcpyDeviceToHost));
    out->rays = d.rays; out->rays_primary = d.rays_primary; out->rays_shadow = d.rays_shadow; out->rays_diffuse = d.rays_diffuse;
    out->iterations = d.iterations; out->minefield_fetches = d.minefield_fetches; out->material_fetches = d.material_fetches;
    out->noise_fetches = d.noise_fetches + ctx->host_noise_base;   // + the seed-base texel of each sample (raytrace.comp:302-303)
    out->hits = d.hits; out->sky_exits = d.sky_exits; out->limit_exits = d.limit_exits; out->border_fetches = d.border_fetches;
    out->pixels = d.pixels; out->frames = ctx->host_frames;
    if (const char* path = getenv("RT_DEBUG_WAVE_DUMP")) {   // -DRT_DIAG_WAVE_TIMES builds of k_paths: per-wave (start, out of paths, end, workgroup)
        if (ctx->lanes[0].pstack) {
            std::vector<unsigned long long> rec(ctx->route.frame ? ((size_t)ctx->ntiles_local + 3u) / 4u * 16u : (size_t)ctx->num_cus * 16u * 4u);
            if (hipMemcpy(rec.data(), ctx->lanes[0].pstack, rec.size() * sizeof(rec[0]), hipMemcpyDeviceToHost) == hipSuccess)
                if (FILE* fp = fopen(path, "wb")) { fwrite(rec.data(), sizeof(rec[0]), rec.size(), fp); fclose(fp); }
        }
    }
    if (getenv("RT_DEBUG_STATS"))
        fprintf(stderr, "[rt] wave loop iters %llu | S block execs %llu (avg lanes %.1f) | F block execs %llu (avg lanes %.1f) | passes %llu "
                        "(avg lanes %.1f, sky lanes %.1f)\n", d.dbg_loop_iters, d.dbg_s_execs, d.dbg_s_execs ? (double)d.dbg_s_lanes / d.dbg_s_execs : 0.0,
                d.dbg_f_execs, d.dbg_f_execs ? (double)d.dbg_f_lanes / d.dbg_f_execs : 0.0, d.dbg_passes,
                d.dbg_passes ? (double)d.dbg_pass_lanes / d.dbg_passes : 0.0, d.dbg_passes ? (double)d.dbg_sky_lanes / d.dbg_passes : 0.0),
        fprintf(stderr, "[rt] raw: loop_iters %llu s_lanes %llu f_lanes %llu passes %llu pass_lanes %llu s_execs %llu f_execs %llu\n", d.dbg_loop_iters, d.dbg_s_lanes,
                d.dbg_f_lanes, d.dbg_passes, d.dbg_pass_lanes, d.dbg_s_execs, d.dbg_f_execs),
        fprintf(stderr, "[rt] raw2: sky_lanes %llu\n", d.dbg_sky_lanes);
    return RT_OK;
}

int rt_reset_counters(RtContext* ctx) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, sync_lanes(ctx));
    RT_HIP(ctx, hipMemset(ctx->d_counters, 0, sizeof(rtd::DevCounters)));
    ctx->host_noise_base = 0; ctx->host_frames = 0;
    return RT_OK;
}

int rt_get_timing(RtContext* ctx, RtTiming* out) {
    if (!ctx || !out) return RT_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    if (!ctx->frame_recorded) return fail(ctx, RT_ERR_NOT_READY, "rt_get_timing: no frame drawn yet");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, sync_lanes(ctx));
    if ((ctx->cfg.flags & RT_FLAG_TIMING_ALL) == RT_FLAG_TIMING_ALL)   // 0 for a context created without RT_FLAG_TIMING_ALL
        RT_HIP(ctx, hipEventElapsedTime(&out->frame_ms, ctx->ev_frame0, ctx->ev_frame1));
    // per-launch events accumulate over every frame drawn since the previous rt_get_timing (no per-frame sync needed)
    for (size_t i = 0; i + 1 < ctx->ev_used; i += 2) {
        float ms = 0.0f;
        RT_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_pool[i], ctx->ev_pool[i + 1]));
        if (ctx->ev_kind[i / 2] == 0) { out->trace_ms += ms; out->trace_launches++; }
        else { out->shade_ms += ms; out->other_launches++; }
    }
    ctx->ev_used = 0;
    return RT_OK;
}

}  // extern "C"
