// api_context.hip — the life of a context: rt_create and its steps, rt_destroy, the stream it runs on, what it reports about
// itself (info, counters, timing, plane accessors), and the ordering between its lanes that every other file builds on.
#include <new>

#include "rt_context.hpp"

using namespace rta;

namespace rta __attribute__((visibility("hidden"))) {

thread_local std::string g_create_error = "";

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

}  // namespace rta

// Light-record budget of a context (all lanes together): RT_PERSIST_LIGHT_GIB, else min(kDefaultLightBytes, a tenth of the free
// device memory): a context is one tenant of the GPU.  Pure function of its inputs apart from hipMemGetInfo.
constexpr uint64_t kDefaultLightBytes = 16ull << 30;
uint64_t rt_light_budget_bytes(const char* env_gib) {
    uint64_t light_bytes = kDefaultLightBytes;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) { if ((uint64_t)free_b / 10u < light_bytes) light_bytes = (uint64_t)free_b / 10u; }
    else (void)hipGetLastError();
    uint64_t gib = 0;
    if (parse_knob(env_gib, 1, 128, &gib)) light_bytes = gib << 30;
    return light_bytes;
}
// Samples of every pixel one launch covers: what `lane_bytes` of 12-byte records hold for `npix` worklist slots, at most 2^31
// paths (path indices are 32-bit), at most spp, at least 1; RT_PERSIST_BATCH may only lower it.  (tests/test_abi.py pins it.)
extern "C" uint64_t rt_samples_per_launch(uint64_t lane_bytes, uint64_t npix, uint64_t spp, const char* env_batch) {
    if (npix == 0) npix = 1;
    uint64_t B = lane_bytes / (sizeof(rtd::PathLight) * npix);
    if (B > (1ull << 31) / npix) B = (1ull << 31) / npix;
    parse_knob(env_batch, 1, (long long)B - 1, &B);
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
    int reserve = 0;
    if (env_int("RT_RESERVE_CUS", 1, c->num_cus - 1, &reserve)) c->num_cus -= reserve;
    RT_HIP(c, new_stream(c, &c->own_stream));
    c->stream = c->own_stream;
    c->lanes[0].stream = c->own_stream;
    for (hipEvent_t* ev : {&c->ev_frame0, &c->ev_frame1}) RT_HIP(c, new_event(c, ev, hipEventDefault));
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
    if (c->nlanes == 2) RT_HIP(c, new_stream(c, &c->lanes[1].stream));
    for (int l = 0; l < c->nlanes; l++) RT_HIP(c, new_event(c, &c->lanes[l].ev_join));
    for (hipEvent_t* ev : {&c->ev_fence, &c->ev_world.ev, &c->ev_query.ev, &c->ev_gather.ev}) RT_HIP(c, new_event(c, ev));
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
        for (hipEvent_t* ev : {&fs.ev_prepass, &fs.ev_acc, &fs.ev_tail.ev}) RT_HIP(c, new_event(c, ev));
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
        RT_HIP(c, new_event(c, &c->ev_accum.ev));
    }
    if (c->reproject) {
        c->d_hist_sum[0] = c->d_accum;
        RT_HIP(c, dev_alloc(c, &c->d_hist_sum[1], (size_t)c->npix_pad));
        for (int h = 0; h < 2; h++) {
            RT_HIP(c, dev_alloc(c, &c->d_hist_rec[h], (size_t)c->npix_pad));
            RT_HIP(c, hipMemset(c->d_hist_rec[h], 0, (size_t)c->npix_pad * sizeof(uint2)));   // rt_read_history before the first frame
        }
    }
    if (c->stream_history) {
        RT_HIP(c, dev_alloc(c, &c->d_slab_masks, (size_t)rtd::kSlabSlots * rtd::kSlabSlotWords));
        RT_HIP(c, dev_alloc(c, &c->d_slab_boxes, 1));
        RT_HIP(c, hipMemset(c->d_slab_boxes, 0, sizeof(rtd::SlabBoxes)));
    }
    RT_HIP(c, rtd::launch_sphere_lut(c->sphere_lut, c->own_stream));
    RT_HIP(c, rtd::launch_dif_lut(c->sphere_lut, c->dif_lut, c->own_stream));
    RT_HIP(c, hipStreamSynchronize(c->own_stream));
    return RT_OK;
}

// the wavefront baseline's queues, and the launch arguments that name them
int create_wavefront(RtContext* c) {
    WavefrontState& w = c->wave;
    uint64_t target = 4u << 20;   // paths per batch
    env_int("RT_BATCH_PATHS", 1, LLONG_MAX, &target);
    uint64_t B = c->npix_pad ? target / c->npix_pad : 1;
    if (B < 1) B = 1;
    if (B > (uint64_t)c->cfg.spp) B = (uint64_t)c->cfg.spp;
    w.batch_samples = (uint32_t)B;
    uint64_t cap64 = (uint64_t)c->npix_pad * B;
    if (cap64 >= (1ull << 31)) return fail(c, RT_ERR_INVALID_ARG, "rt_create: batch too large");
    w.cap = (uint32_t)cap64;
    const size_t cap = w.cap;
    rtd::ShadeArgs& sa = w.shade;
    RT_HIP(c, dev_alloc(c, &sa.qox, cap)); RT_HIP(c, dev_alloc(c, &sa.qoy, cap)); RT_HIP(c, dev_alloc(c, &sa.qoz, cap));
    RT_HIP(c, dev_alloc(c, &sa.qdx, 2 * cap)); RT_HIP(c, dev_alloc(c, &sa.qdy, 2 * cap)); RT_HIP(c, dev_alloc(c, &sa.qdz, 2 * cap));
    RT_HIP(c, dev_alloc(c, &sa.qid, cap));
    rtd::TraceArgs& ta = w.trace;
    RT_HIP(c, dev_alloc(c, &ta.hx, cap)); RT_HIP(c, dev_alloc(c, &ta.hy, cap)); RT_HIP(c, dev_alloc(c, &ta.hz, cap));
    RT_HIP(c, dev_alloc(c, &ta.hinfo, cap));
    RT_HIP(c, dev_alloc(c, &ta.sunres, cap)); RT_HIP(c, dev_alloc(c, &sa.pnormal, cap)); RT_HIP(c, dev_alloc(c, &sa.pstate, cap));
    RT_HIP(c, dev_alloc(c, &sa.pdx, cap)); RT_HIP(c, dev_alloc(c, &sa.pdy, cap)); RT_HIP(c, dev_alloc(c, &sa.pdz, cap));
    RT_HIP(c, dev_alloc(c, &sa.plx, cap)); RT_HIP(c, dev_alloc(c, &sa.ply, cap)); RT_HIP(c, dev_alloc(c, &sa.plz, cap));
    RT_HIP(c, dev_alloc(c, &sa.sunbits, cap));
    RT_HIP(c, dev_alloc(c, &sa.stack, cap * (size_t)(c->cfg.depth > 1 ? c->cfg.depth - 1 : 1)));
    RT_HIP(c, dev_alloc(c, &w.acc, (size_t)c->npix_pad));
    RT_HIP(c, dev_alloc(c, &w.ctrl, (size_t)2 * (RT_MAX_DEPTH + 2)));
    // the trace stage reads the queues the shade stages write, and writes the hits they read
    ta.qox = sa.qox; ta.qoy = sa.qoy; ta.qoz = sa.qoz; ta.qdx = sa.qdx; ta.qdy = sa.qdy; ta.qdz = sa.qdz; ta.qid = sa.qid;
    sa.hx = ta.hx; sa.hy = ta.hy; sa.hz = ta.hz; sa.hinfo = ta.hinfo; sa.sunres = ta.sunres;
    ta.qcap = sa.qcap = sa.npaths_cap = w.cap;
    ta.npix_pad = sa.npix_pad = c->npix_pad;
    ta.refill_threshold = w.refill_threshold;
    ta.counters = sa.counters = c->d_counters;
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
        if (cfg->edit_radius < 0 || cfg->edit_radius > 64)
            return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: edit_radius must be 0 (an edit restarts the history) or 1..64");
        if (cfg->stream_history != 0 && cfg->stream_history != 1)
            return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: stream_history must be 0 (a slab restarts the history) or 1");
        if (cfg->stream_history == 1 && cfg->edit_radius < 1)
            return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: stream_history = 1 needs edit_radius in 1..64 (its near test uses it)");
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
    c->edit_radius = c->reproject ? (uint32_t)cfg->edit_radius : 0u;   // (ignored without the flag, like history_cap)
    c->stream_history = c->reproject && cfg->stream_history == 1;      // (likewise)

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
    env_int("RT_LANES", 1, persistent ? 2 : 1, &c->nlanes);
    env_int("RT_FRAMES_IN_FLIGHT", 1, persistent ? 2 : 1, &c->nslots);
    if (c->nlanes < 2) c->nslots = 1;
    env_int("RT_FRAME_CROSSOVER", 0, LLONG_MAX, &c->frame_crossover);
    env_int("RT_FRAME_CROSSOVER_MULTI", 0, LLONG_MAX, &c->frame_crossover_multi);
    env_int("RT_FRAME_THRESHOLD", 1, 64, &c->frame_threshold);
    if (env_int("RT_FRAME_TILES", 1, 4, &c->frame_tiles)) c->frame_tiles *= 4u;   // per wave
    env_int("RT_FRAME_GROUP_TILES", 1, 16, &c->frame_tiles);                      // per four-wave workgroup
    env_int("RT_REFILL_THRESHOLD", 1, 64, &c->wave.refill_threshold);
    env_int("RT_PREPASS_REUSE", 0, 0, &c->prepass_reuse);
    env_int("RT_PROBE_PAIR", 0, 1, &c->probe_pair);
    env_int("RT_PRIMARY_V", 1, 2, &c->primary_version);
    env_int("RT_PERSIST_THRESHOLD", 1, 64, &c->persist_threshold);
    env_int("RT_PL_STREAM", 0, 3, &c->pl_stream_mode);
    if (env_int("RT_PERSIST_CHUNK", 64, 4096, &c->persist_chunk)) c->persist_chunk &= ~63u;

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

// Nothing is destroyed before every stream that may still reference it has drained.
void rt_destroy(RtContext* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    for (hipStream_t st : ctx->streams) (void)hipStreamSynchronize(st);
    if (ctx->user_stream && ctx->stream) (void)hipStreamSynchronize(ctx->stream);   // (the caller's: not ours to destroy)
    for (hipEvent_t e : ctx->events) (void)hipEventDestroy(e);
    for (TimingPool* t : {&ctx->launch_times, &ctx->gather_times}) for (hipEvent_t e : t->ev) (void)hipEventDestroy(e);
    for (StagingSet* s : {&ctx->slab_sets[0], &ctx->slab_sets[1], &ctx->edit_sets[0], &ctx->edit_sets[1], &ctx->draw_sets[0], &ctx->draw_sets[1]}) s->release();
    ctx->query_block.release();
    for (StampEntry& e : ctx->stamps.slots) {   // the stamps nobody destroyed
        if (e.mats) (void)hipFree(reinterpret_cast<void*>(e.mats));
        if (e.state) (void)hipFree(reinterpret_cast<void*>(e.state));
    }
    for (NavEntry& e : ctx->navs.slots)      // the navigation fields nobody destroyed
        if (e.block) (void)hipFree(reinterpret_cast<void*>(e.block));
    for (void* p : ctx->allocs) (void)hipFree(p);
    for (hipStream_t st : ctx->streams) (void)hipStreamDestroy(st);
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
    ctx->ev_accum.forget();        // (everything before has finished)
    invalidate_prepass(ctx);       // (lanes and slots in use change with the stream)
    return RT_OK;
}

int rt_sync(RtContext* ctx) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, sync_lanes(ctx));
    if (ctx->gather_stream) RT_HIP(ctx, hipStreamSynchronize(ctx->gather_stream));
    return RT_OK;
}

int rt_upload_noise(RtContext* ctx, const uint8_t* rgba8) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!rgba8) return fail(ctx, RT_ERR_INVALID_ARG, "rt_upload_noise: null pointer");
    restart_history(ctx);
    invalidate_prepass(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, sync_lanes(ctx));
    RT_HIP(ctx, hipMemcpy(ctx->d_noise, rgba8, RT_NOISE_BYTES, hipMemcpyHostToDevice));
    ctx->has_noise = true;
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

void* rt_gbuffer_ptr(RtContext* ctx) { return ctx ? ctx->gbuffer : nullptr; }
size_t rt_gbuffer_bytes(RtContext* ctx) { return ctx ? ctx->gbuffer_bytes : 0; }
size_t rt_gbuffer_offset(RtContext* ctx, int id) {
    if (!ctx || id < 0 || id > RT_BUF_FOG_RGBA8) return 0;
    return ctx->gbuffer_offset[id];
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

int rt_get_info(RtContext* ctx, RtInfo* out) {
    if (!ctx || !out) return RT_ERR_INVALID_ARG;
    if (out->struct_size != sizeof(RtInfo)) return fail(ctx, RT_ERR_INVALID_ARG, "rt_get_info: RtInfo.struct_size mismatch");
    out->num_cus = ctx->num_cus;
    const bool persistent = ctx->route.family == RT_KERNEL_PERSISTENT;
    out->samples_per_launch = persistent ? ctx->persist_batch : ctx->wave.batch_samples;
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
    RT_HIP(ctx, ctx->launch_times.drain([&](size_t pair, float ms) {
        if (ctx->launch_kind[pair] == 0) { out->trace_ms += ms; out->trace_launches++; }
        else { out->shade_ms += ms; out->other_launches++; }
    }));
    return RT_OK;
}

}  // extern "C"
