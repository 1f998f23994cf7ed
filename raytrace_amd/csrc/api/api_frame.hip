// api_frame.hip — rt_draw_frame: the route (which kernel takes which launch), a frame of the persistent family over lanes and
// frame slots, the wavefront baseline's frame, and the accumulation / history calls.
#include "rt_context.hpp"

using namespace rta;

namespace rta __attribute__((visibility("hidden"))) {

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

// raytrace.comp:317-318 — uniform over the frame, so evaluated once here with the same rt_math.h the kernels use.
static void sun_constants(float a, float* sunangle, float* sunlight) {
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

}  // namespace rta

namespace {

// RT_FLAG_ACCUMULATE: the uniforms a frame continues the accumulation under — every live field but seed, bit for bit
void accum_key_of(const RtUniforms* u, uint32_t key[16]) {
    memcpy(&key[0], &u->sun_angle, 4);
    memcpy(&key[1], u->origin, 12); memcpy(&key[4], u->forward, 12); memcpy(&key[7], u->up, 12); memcpy(&key[10], u->right, 12);
    memcpy(&key[13], u->lr, 12);
}

int draw_wavefront(RtContext* c, const rtd::Frame& f) {
    const WavefrontState& w = c->wave;
    const bool count = (c->cfg.flags & RT_FLAG_COUNTERS) != 0;
    const rtd::Scene sc = scene_of(c);
    const rtd::Planes pl = planes_of(c);
    const int D = c->cfg.depth;
    const uint32_t spp = (uint32_t)c->cfg.spp;
    const uint32_t B = w.batch_samples;
    const uint32_t ctrl_words = 2 * (RT_MAX_DEPTH + 2);
    uint32_t batch = 0;
    for (uint32_t s0 = 0; s0 < spp; s0 += B, batch++) {
        const uint32_t ns = spp - s0 < B ? spp - s0 : B;
        const uint32_t npaths = c->npix_pad * ns;
        uint32_t* counts = w.ctrl;
        uint32_t* cursors = w.ctrl + (RT_MAX_DEPTH + 2);
        RT_HIP(c, hipMemsetAsync(w.ctrl, 0, ctrl_words * sizeof(uint32_t), c->stream));

        rtd::TraceArgs ta = w.trace;
        ta.nprimary = npaths;
        rtd::ShadeArgs sa = w.shade;
        sa.npaths = npaths; sa.sample0 = s0;

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
        { LaunchTimer t(c, 1); RT_HIP(c, rtd::launch_accumulate(sa.plx, sa.ply, sa.plz, w.acc, c->npix_pad, ns, batch == 0, c->stream)); }
    }
    { LaunchTimer t(c, 1); RT_HIP(c, rtd::launch_resolve(f, w.acc, pl, c->npix_pad, c->stream)); }
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
    uint32_t nbox = 0;                  // RtConfig.edit_radius > 0: the edited boxes this frame consumed, in world coordinates
    rtd::TemporalBox boxes[rtd::kTemporalMaxBoxes];
    uint32_t nslab = 0;                 // RtConfig.stream_history: the pending slabs this frame consumed (mask slots 0 .. nslab - 1)
    int32_t lr_prev[3] = {}, lr[3] = {};   // ... and the lr that places what left (the previous frame's) and what arrived (this one's)
};

// A pending texel box in the world coordinates of a frame with render offset lr: w = lr - R/2 + (t - lr) mod R per axis
// (render.texel_to_world), the box [w(min), w(max) + 1].  Where the window's seam cuts the box (w(min) > w(max)) it covers the
// whole window on that axis, which is conservative.
rtd::TemporalBox world_box(const EditBox& b, const int32_t lr[3], int region) {
    rtd::TemporalBox w;
    const int64_t R = region;
    for (int k = 0; k < 3; k++) {
        const int64_t base = (int64_t)lr[k] - R / 2;
        const int64_t lo = base + ((((int64_t)b.lo[k] - lr[k]) % R) + R) % R, hi = base + ((((int64_t)b.hi[k] - lr[k]) % R) + R) % R;
        w.lo[k] = (float)(lo <= hi ? lo : base);
        w.hi[k] = (float)(lo <= hi ? hi + 1 : base + R);
    }
    return w;
}

// The frame's slot and first lane, its accumulation key; then the slot's previous frame has finished with the slot.
hipError_t frame_begin(RtContext* c, PersistFrame& p, const RtUniforms* u, bool frame_events) {
    p.count = (c->cfg.flags & RT_FLAG_COUNTERS) != 0;
    p.cache = (c->cfg.flags & RT_FLAG_CACHE_PRIMARY) != 0;
    p.nl = c->user_stream ? 1 : c->nlanes;
    p.nsl = c->user_stream ? 1 : c->nslots;
    hipError_t e = hipSuccess;
    // What the host put behind the previous frame since (post passes, gather, a slab) belongs to that frame's use of its slot.
    if (c->frame_recorded) e = c->slots[c->cur_slot].ev_tail.record(c->stream);
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
    // (edit boxes belong to the next frame drawn: this one consumes them, whatever it makes of them; an overflowed set restarts it)
    if (c->edit_overflow) c->accum_valid = false;
    p.nbox = c->edit_nbox;
    for (uint32_t b = 0; b < p.nbox; b++) p.boxes[b] = world_box(c->edit_boxes[b], u->lr, c->region);
    c->edit_nbox = 0;
    c->edit_overflow = false;
    // (pending slabs likewise; their boxes are made on the device, in front of the pass)
    if (c->slab_overflow) c->accum_valid = false;
    p.nslab = c->slab_pending;
    memcpy(p.lr_prev, &c->accum_key[13], 12); memcpy(p.lr, u->lr, 12);
    c->slab_pending = 0;
    c->slab_overflow = false;
    c->slab_boxes_drawn = false;
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
        // pending boxes and a history that goes on: the moved pass with the box test — also under an unchanged camera, where it
        // projects into the same camera.  (A frame that restarts anyway drops them.)
        if (p.temporal_mode != rtd::TEMPORAL_RESTART && p.nbox > 0u) p.temporal_mode = rtd::TEMPORAL_MOVED_BOXES;
        // pending slabs and a history that goes on: the same, with the slab boxes behind the edit boxes (of which there may be none)
        if (p.temporal_mode != rtd::TEMPORAL_RESTART && p.nslab > 0u) p.temporal_mode = rtd::TEMPORAL_MOVED_SLABS;
        if (p.temporal_mode != rtd::TEMPORAL_RESTART && p.temporal_mode != rtd::TEMPORAL_STILL) {
            p.accum_cont = true;
            p.accum_n = (c->accum_samples < c->history_cap ? c->accum_samples : (uint64_t)c->history_cap) + 1u;
        }
    }
    // the frame that used the slot before (frame k - 2 with two slots, k - 1 with one) has finished with it
    if (e == hipSuccess) e = p.fs->ev_tail.wait(p.st0);
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
    if (e == hipSuccess && p.accum_multi) e = c->ev_accum.wait_elsewhere(p.st0);
    if (e == hipSuccess && p.accum_multi)
        e = rtd::launch_accumulate_frame(p.f, p.pl, c->d_accum, c->npix_pad, p.accum_cont, (int)p.accum_n, c->cfg.spp, true, p.st0);
    if (prepass_clears && e == hipSuccess) { fs.wl_clean[fs.wl_parity ^ 1] = true; p.L0->cursor_clean = true; }
    fs.wl_parity ^= 1;   // (whatever happened: the frame counts in the set p.wlc names)
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
        rtd::PersistArgs pa{};   // (rmin stays 0: it was k_seq's re-arm threshold, no kernel reads it)
        pa.cursor = L->cursor; pa.worklist = fs.worklist; pa.wl_count = p.wlc; pa.direct = r.direct ? 1u : 0u;
        pa.npix_pad = c->npix_pad; pa.sample0 = s0; pa.nsamples = ns; pa.chunk = c->persist_chunk;
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
            if (e == hipSuccess && p.accum_multi && !p.cache && s0 == 0) e = c->ev_accum.wait_elsewhere(st);
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
        e = c->ev_accum.wait_elsewhere(p.tail);
        LaunchTimer t(c, 1, p.tail);
        if (e == hipSuccess && !c->reproject)
            e = rtd::launch_accumulate_frame(p.f, p.pl, c->d_accum, c->npix_pad, p.accum_cont, (int)p.accum_n, 1, false, p.tail);
        if (e == hipSuccess && c->reproject) {
            // the pass reads the set the previous frame's pass wrote (ordered by ev_accum / stream order) and writes the other
            rtd::TemporalArgs ta{};
            const int prev = c->hist_cur, next = prev ^ 1;
            ta.prev_sum = c->d_hist_sum[prev]; ta.prev_rec = c->d_hist_rec[prev];
            ta.next_sum = c->d_hist_sum[next]; ta.next_rec = c->d_hist_rec[next];
            memcpy(ta.origin, &c->accum_key[1], 12); memcpy(ta.forward, &c->accum_key[4], 12);
            memcpy(ta.up, &c->accum_key[7], 12); memcpy(ta.right, &c->accum_key[10], 12);
            ta.cap = c->history_cap;
            if (p.temporal_mode == rtd::TEMPORAL_MOVED_SLABS) {
                // (behind the previous frame's pass, which read the boxes of ITS slabs: ev_accum above, or stream order)
                e = rtd::launch_place_slab_boxes(c->d_slab_masks, p.nslab, p.lr_prev, p.lr, c->logr, c->d_slab_boxes, p.tail);
                ta.slab = c->d_slab_boxes;
                c->slab_boxes_drawn = e == hipSuccess;
            }
            if (p.temporal_mode == rtd::TEMPORAL_MOVED_BOXES || p.temporal_mode == rtd::TEMPORAL_MOVED_SLABS) {
                ta.nbox = p.nbox;
                memcpy(ta.box, p.boxes, sizeof(ta.box));
                ta.r2 = (float)(c->edit_radius * c->edit_radius);
                for (int k = 0; k < 3; k++) { ta.sun[k] = p.f.sunangle[k]; ta.inv_sun[k] = 1.0f / p.f.sunangle[k]; }
            }
            if (e == hipSuccess) e = rtd::launch_temporal_frame(p.f, p.pl, ta, p.temporal_mode, p.tail);
            c->hist_cur = next;
        }
    }
    if (e == hipSuccess && p.nl == 2) e = c->ev_accum.record(p.tail);
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

extern "C" {

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
    restart_history(ctx);
    return RT_OK;
}

int rt_edit_boxes_pending(RtContext* ctx, uint32_t* boxes, uint32_t* overflowed) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!boxes || !overflowed) return fail(ctx, RT_ERR_INVALID_ARG, "rt_edit_boxes_pending: null pointer");
    *boxes = ctx->edit_nbox;
    *overflowed = ctx->edit_overflow ? 1u : 0u;
    return RT_OK;
}

int rt_slabs_pending(RtContext* ctx, uint32_t* slabs, uint32_t* overflowed) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!slabs || !overflowed) return fail(ctx, RT_ERR_INVALID_ARG, "rt_slabs_pending: null pointer");
    *slabs = ctx->slab_pending;
    *overflowed = ctx->slab_overflow ? 1u : 0u;
    return RT_OK;
}

int rt_read_slab_boxes(RtContext* ctx, float* boxes, uint32_t* count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!ctx->stream_history) return fail(ctx, RT_ERR_INVALID_ARG, "rt_read_slab_boxes: the context was created without RtConfig.stream_history");
    if (!boxes || !count) return fail(ctx, RT_ERR_INVALID_ARG, "rt_read_slab_boxes: null pointer");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, sync_lanes(ctx));
    *count = 0;
    if (!ctx->slab_boxes_drawn) return RT_OK;   // (the frame drawn last had no pending slab, or restarted)
    rtd::SlabBoxes b;
    RT_HIP(ctx, hipMemcpy(&b, ctx->d_slab_boxes, sizeof(b), hipMemcpyDeviceToHost));
    *count = b.count <= rtd::kSlabMaxBoxes ? b.count : rtd::kSlabMaxBoxes;
    memcpy(boxes, b.box, (size_t)*count * sizeof(rtd::TemporalBox));
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

}  // extern "C"
