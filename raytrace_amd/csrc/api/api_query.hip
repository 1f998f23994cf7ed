// api_query.hip — queries against the resident world: ray queries (rt_trace_rays, rt_trace_rays_async, rt_pick_pixels), light
// probes (rt_probe_light, rt_probe_light_async), box sweeps (rt_sweep_boxes, rt_sweep_boxes_async), the particle simulation built on
// them (rt_step_particles, rt_step_particles_async) and entity queries (rt_trace_entities, rt_trace_entities_async,
// rt_pick_entities) and entity sweeps (rt_sweep_entities, rt_sweep_entities_async), which share their checks, stream and staging, and
// the particle emitters (rt_emit_particles, rt_emit_particles_async), whose world, stream and ordering are the sweeps'.  An entity
// set's models reach the device through api_passes.hip's models_send (a ModelBatch: the ev_capture wait before the launch, applied()
// behind it); a sweep's domain and a pick's pixels are tested by the check headers' one definition each.
#include "emit_check.hpp"
#include "entity_query_check.hpp"
#include "particle_step_check.hpp"
#include "sweep_entities_check.hpp"
#include "rt_context.hpp"

using namespace rta;

namespace rta {
// rt_trace_rays_async's pointers: 16-byte aligned (the kernel's float4 / uint4 accesses) and memory of the context's device (or
// managed memory).  A host address would fault the kernel: pageable memory is not mapped for the device with XNACK off.
bool query_device_ptr(const RtContext* c, const void* p) {
    if (((uintptr_t)p & 15u) != 0u) return false;
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // (clears the error it set)
    if (a.type == hipMemoryTypeManaged || a.isManaged) return true;
    return a.type == hipMemoryTypeDevice && a.device == c->device;
}
}  // namespace rta

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
        RT_HIP(c, new_stream(c, &c->query_stream, &greatest));
    }
    if (c->user_stream) { *st = c->stream; return RT_OK; }
    *st = c->query_stream;
    RT_HIP(c, c->ev_world.wait(*st));
    return RT_OK;
}

int query_launch(RtContext* c, hipStream_t st, const rtd::Frame& f, const void* rays_dev, const void* xy_dev, void* hits_dev, uint32_t count) {
    rtd::QueryArgs a;
    a.rays = reinterpret_cast<const float4*>(rays_dev);
    a.xy = reinterpret_cast<const int2*>(xy_dev);
    a.hits = reinterpret_cast<uint4*>(hits_dev);
    a.count = count;
    RT_HIP(c, rtd::launch_query(scene_of(c), f, a, st));
    if (!c->user_stream) RT_HIP(c, c->ev_query.record(st));   // (a caller's stream orders itself)
    return RT_OK;
}

rtd::Frame query_frame(const RtContext* c, const int32_t lr[3]) {
    RtUniforms u{};
    for (int k = 0; k < 3; k++) u.lr[k] = lr[k];
    return frame_of(c, &u);
}

// The end of a synchronous call: the `bytes` its launches left at `dev` (a part of stage_sync's) back to `out`; waits for them.
int fetch_sync(RtContext* c, hipStream_t st, const uint8_t* dev, void* out, size_t bytes) {
    uint8_t* host = c->query_block.host + (dev - c->query_block.dev);
    RT_HIP(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
    RT_HIP(c, hipStreamSynchronize(st));
    memcpy(out, host, bytes);
    return RT_OK;
}

// The synchronous calls: `in_bytes` of input through pinned and device staging, the launch, the hits back.
int query_sync(RtContext* c, const rtd::Frame& f, const void* in, size_t in_bytes, bool picks, RtRayHit* hits, uint32_t count) {
    hipStream_t st;
    int rc = query_stream_of(c, &st);
    if (rc != RT_OK) return rc;
    const size_t out_bytes = (size_t)count * sizeof(RtRayHit);
    uint8_t* dev[2];
    rc = stage_sync(c, st, {{in, in_bytes}, {nullptr, out_bytes}}, dev);
    if (rc != RT_OK) return rc;
    rc = query_launch(c, st, f, picks ? nullptr : dev[0], picks ? dev[0] : nullptr, dev[1], count);
    if (rc != RT_OK) return rc;
    return fetch_sync(c, st, dev[1], hits, out_bytes);
}

// ---- light probes -------------------------------------------------------------------------------------------------------------
constexpr uint32_t kMaxProbeSamples = 4096;
constexpr size_t kProbeScratchBytes = (size_t)64 << 20;   // the most path records a launch leaves in the context's scratch

// checks shared by the two calls (query_check's, and the probe's own); RT_OK when there is work to enqueue, 1 for count == 0
int probe_check(RtContext* c, const char* fn, const RtUniforms* u, const void* probes, uint32_t count, uint32_t samples, int32_t depth,
                const void* out) {
    if (samples < 1u || samples > kMaxProbeSamples) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": samples must be 1..4096");
    if (depth < 1 || depth > RT_MAX_DEPTH) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": depth must be 1..RT_MAX_DEPTH");
    if ((uint64_t)count * samples > rtd::kProbeMaxPaths) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": more than 2^26 paths in one call");
    const int rc = query_check(c, fn, count, probes, u, out);
    if (rc != RT_OK) return rc;
    if (!c->has_noise) return fail(c, RT_ERR_NOT_READY, std::string(fn) + ": upload the blue-noise table first");
    return RT_OK;
}

// The launches of one call on `st`: all probes at once when a workgroup adds its probes' samples itself, else whole probes in
// pieces whose path records fit the scratch (the pieces follow each other on the stream, so they share it).
int probe_launch(RtContext* c, hipStream_t st, const RtUniforms* u, const void* probes_dev, void* out_dev, uint32_t count, uint32_t samples,
                 int32_t depth) {
    rtd::Frame f = frame_of(c, u);
    f.depth = depth;
    f.spp = (int)samples;
    uint32_t per_launch = count;
    if (!rtd::probe_sums_in_lds(samples)) {
        per_launch = (uint32_t)(kProbeScratchBytes / sizeof(float4)) / samples;   // >= 1024 probes: samples <= 4096
        if (per_launch > count) per_launch = count;
        const size_t need = (size_t)per_launch * samples * sizeof(float4);
        if (need > c->probe_scratch_bytes) {
            if (c->probe_scratch) {
                RT_HIP(c, hipStreamSynchronize(st));   // (an earlier call's launches may still use it)
                for (size_t i = 0; i < c->allocs.size(); i++)
                    if (c->allocs[i] == c->probe_scratch) { c->allocs.erase(c->allocs.begin() + (long)i); break; }
                (void)hipFree(c->probe_scratch);
                c->device_bytes -= c->probe_scratch_bytes;
                c->probe_scratch = nullptr;
                c->probe_scratch_bytes = 0;
            }
            const size_t bytes = (need + (((size_t)1 << 20) - 1u)) & ~(((size_t)1 << 20) - 1u);
            RT_HIP(c, dev_alloc(c, &c->probe_scratch, bytes / sizeof(float4)));
            c->probe_scratch_bytes = bytes;
        }
    }
    for (uint32_t first = 0; first < count; first += per_launch) {
        rtd::ProbeArgs a;
        a.probes = reinterpret_cast<const uint4*>(probes_dev) + 2u * (size_t)first;
        a.out = reinterpret_cast<uint4*>(out_dev) + first;
        a.scratch = c->probe_scratch;
        a.count = count - first < per_launch ? count - first : per_launch;
        a.samples = samples;
        RT_HIP(c, rtd::launch_probe(scene_of(c), f, a, c->probe_pair, st));
    }
    if (!c->user_stream) RT_HIP(c, c->ev_query.record(st));   // (a caller's stream orders itself)
    return RT_OK;
}

// ---- box sweeps ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t kMaxSweeps = 1u << 24;
static_assert(sizeof(RtBoxSweep) == 48 && sizeof(RtSweepHit) == 64, "the kernel reads three and writes four 16-byte words per sweep");

// checks shared by the two calls; RT_OK when there is work to enqueue, 1 for count == 0
int sweep_check(RtContext* c, const char* fn, uint32_t count, const void* sweeps, const void* lr, const void* hits) {
    if (count > kMaxSweeps) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": more than 2^24 sweeps in one call");
    return query_check(c, fn, count, sweeps, lr, hits);
}

int sweep_launch(RtContext* c, hipStream_t st, const int32_t lr[3], const void* sweeps_dev, void* hits_dev, uint32_t count) {
    rtd::SweepArgs a;
    a.sweeps = reinterpret_cast<const uint4*>(sweeps_dev);
    a.hits = reinterpret_cast<uint4*>(hits_dev);
    a.count = count;
    for (int k = 0; k < 3; k++) a.lr[k] = lr[k];
    RT_HIP(c, rtd::launch_sweep(scene_of(c), c->logr, a, st));
    if (!c->user_stream) RT_HIP(c, c->ev_query.record(st));   // (a caller's stream orders itself)
    return RT_OK;
}

// ---- particle simulation: the sweeps' world, stream and ordering ---------------------------------------------------------------
static_assert(sizeof(RtParticleState) == 64 && sizeof(RtParticleStep) == 48 && sizeof(RtParticle) == 32,
              "the kernel reads and writes four 16-byte words per state and writes two per draw record");
static_assert(kMaxStepParticles == rtd::kMaxParticles, "a tick's draw records are one rt_draw_particles call");

// checks shared by the two calls; RT_OK when there is work to enqueue, 1 for count == 0
int step_check(RtContext* c, const char* fn, const RtParticleStep* p, const void* in, const void* out, const void* draw, uint32_t count) {
    const char* e = particle_step_args_error(p, in, out, draw, count);
    if (e) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": " + e);
    if (count == 0) return 1;
    e = particle_step_params_error(*p);
    if (e) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": " + e);
    if (!c->world_resident) return fail(c, RT_ERR_NOT_READY, std::string(fn) + ": upload the full region first");
    return RT_OK;
}

int step_launch(RtContext* c, hipStream_t st, const RtParticleStep& p, const void* in_dev, void* out_dev, void* draw_dev, uint32_t count) {
    rtd::StepParticlesArgs a;
    a.in = reinterpret_cast<const uint4*>(in_dev);
    a.out = reinterpret_cast<uint4*>(out_dev);
    a.draw = reinterpret_cast<uint4*>(draw_dev);
    a.count = count;
    a.sweeps = p.sweeps;
    a.dt = p.dt; a.damping = p.damping; a.restitution = p.restitution; a.friction = p.friction; a.rest_speed = p.rest_speed;
    for (int k = 0; k < 3; k++) { a.lr[k] = p.lr[k]; a.accel[k] = p.accel[k]; }
    RT_HIP(c, rtd::launch_step_particles(scene_of(c), c->logr, a, st));
    if (!c->user_stream) RT_HIP(c, c->ev_query.record(st));   // (a caller's stream orders itself)
    return RT_OK;
}

// ---- particle emitters: the sweeps' world, stream and ordering; host emitters through a staging set as the models of a draw -----
static_assert(sizeof(RtParticleEmit) == 96 && sizeof(RtEmitCursor) == 16, "the kernels read six 16-byte words per emitter and one per cursor");
static_assert(kMaxEmitters == rtd::kMaxEmitRecords && kMaxEmitBricks == rtd::kMaxEmitItems && kMaxEmitCapacity == rtd::kMaxParticles,
              "the host's limits are the kernels'");

// checks shared by the two calls, and the plan; RT_OK when there is work to enqueue, 1 for a call that enqueues nothing
int emit_check(RtContext* c, const char* fn, const RtParticleEmit* emitters, uint32_t count, const int32_t lr[3], const void* states,
               uint32_t capacity, uint32_t max_emit, const RtEmitCursor* host_cursor, const void* cursor, EmitPlan* plan) {
    const char* e = emit_args_error(emitters, count, lr, states, capacity, max_emit, cursor);
    if (e) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": " + e);
    if (count == 0) return 1;
    const uint32_t bad = first_invalid_emitter(emitters, count, c->logr);
    if (bad != count) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": emitter " + std::to_string(bad) + " is not a valid emitter");
    if (!emit_window_valid(lr, c->logr)) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": |lr| must not exceed 2^22 - R");
    if (host_cursor && !emit_cursor_valid(*host_cursor, capacity))
        return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": the cursor's next must be below capacity and its reserved word 0");
    *plan = emit_plan(emitters, count, c->logr);
    if (plan->items > kMaxEmitBricks) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": the bounding boxes cover more than 2^18 bricks");
    if (!c->world_resident) return fail(c, RT_ERR_NOT_READY, std::string(fn) + ": upload the full region first");
    return plan->recs.empty() ? 1 : RT_OK;
}

// The plan's records to the device for `st` to read, the three launches there, and what waits for them: the staging set's next
// transfer (ev_applied), the scratch's next user on another stream (ev_emit), later world changes (ev_query).
int emit_launch(RtContext* c, hipStream_t st, const EmitPlan& plan, const int32_t lr[3], void* states_dev, uint32_t capacity, uint32_t max_emit,
                void* cursor_dev) {
    rtd::EmitParticlesArgs a;
    a.nrecs = (uint32_t)plan.recs.size();
    a.items = (uint32_t)plan.items;
    int rc = emit_scratch_reserve(c, rtd::emit_scratch_words(a.items));
    if (rc != RT_OK) return rc;
    ModelBatch b;
    rc = upload_models(c, nullptr, 0u, plan.recs.data(), plan.recs.size() * sizeof(EmitRecord), st, &b);
    if (rc != RT_OK) return rc;
    a.recs = b.recs();
    a.states = reinterpret_cast<uint4*>(states_dev);
    a.cursor = reinterpret_cast<uint4*>(cursor_dev);
    a.scratch = c->emit_scratch;
    a.capacity = capacity;
    a.max_emit = max_emit;
    for (int k = 0; k < 3; k++) a.lr[k] = lr[k];
    RT_HIP(c, c->ev_emit.wait_elsewhere(st));   // the scratch is the previous call's until its write pass has run
    RT_HIP(c, rtd::launch_emit_particles(scene_of(c), c->logr, a, st));
    RT_HIP(c, b.applied(st));
    RT_HIP(c, c->ev_emit.record(st));
    if (!c->user_stream) RT_HIP(c, c->ev_query.record(st));   // (a caller's stream orders itself)
    return RT_OK;
}

// ---- entity queries: device rays (or pixels) and boxes, host models as rt_draw_stamps' ------------------------------------------
static_assert(sizeof(RtEntityHit) == 48 && sizeof(RtRayHit) == 48, "the kernel writes three 16-byte words per record of either kind");

// checks shared by the three calls; RT_OK when there is work to enqueue, 1 for count == 0
int entity_check(RtContext* c, const char* fn, uint32_t count, const void* in, const void* more, const void* entity_hits, const void* boxes,
                 uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels) {
    const char* e = entity_query_args_error(count, in, more, entity_hits, boxes, nboxes, models, nmodels);
    if (e) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": " + e);
    if (count == 0) return 1;
    if (!c->world_resident) return fail(c, RT_ERR_NOT_READY, std::string(fn) + ": upload the full region first");
    return models_check(c, fn, models, nmodels, "nothing was answered");
}

// The models to the device for `st` to read (models_send: behind the latest rt_stamp_capture), the launch there, and what waits for
// it: the staging set's next transfer and rt_stamp_destroy (ev_applied), later world changes (ev_query).
int entity_launch(RtContext* c, hipStream_t st, const rtd::Frame& f, const void* rays_dev, const void* xy_dev, uint32_t count, const void* boxes_dev,
                  uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels, void* world_dev, void* entity_dev) {
    ModelBatch b;
    const int rc = models_send(c, models, nmodels, st, &b);
    if (rc != RT_OK) return rc;
    rtd::EntityQueryArgs a;
    a.rays = reinterpret_cast<const float4*>(rays_dev);
    a.xy = reinterpret_cast<const int2*>(xy_dev);
    a.world_hits = reinterpret_cast<uint4*>(world_dev);
    a.entity_hits = reinterpret_cast<uint4*>(entity_dev);
    a.boxes = reinterpret_cast<const uint4*>(boxes_dev);
    a.recs = b.recs();
    a.count = count; a.nboxes = nboxes; a.nmodels = nmodels;
    RT_HIP(c, rtd::launch_entity_query(scene_of(c), f, a, st));
    RT_HIP(c, b.applied(st));
    if (!c->user_stream) RT_HIP(c, c->ev_query.record(st));   // (a caller's stream orders itself)
    return RT_OK;
}

// The synchronous calls against an entity set: the input records, the boxes and both outputs through one staging block on the query
// stream, `launch(st, in, boxes, world, entity)` on the parts' device addresses (null for boxes or world hits the call does without),
// one or two blocks back.
template <typename Launch>
int entity_set_sync(RtContext* c, const void* in, size_t in_bytes, const RtDrawBox* boxes, uint32_t nboxes, void* world_hits, size_t world_bytes,
                    void* entity_hits, size_t entity_bytes, Launch&& launch) {
    hipStream_t st;
    int rc = query_stream_of(c, &st);
    if (rc != RT_OK) return rc;
    if (!world_hits) world_bytes = 0u;
    uint8_t* dev[4];
    rc = stage_sync(c, st, {{in, in_bytes}, {nboxes ? boxes : nullptr, (size_t)nboxes * sizeof(RtDrawBox)}, {nullptr, world_bytes}, {nullptr, entity_bytes}}, dev);
    if (rc != RT_OK) return rc;
    rc = launch(st, dev[0], nboxes ? dev[1] : nullptr, world_hits ? dev[2] : nullptr, dev[3]);
    if (rc != RT_OK) return rc;
    if (world_hits) {
        rc = fetch_sync(c, st, dev[2], world_hits, world_bytes);
        if (rc != RT_OK) return rc;
    }
    return fetch_sync(c, st, dev[3], entity_hits, entity_bytes);
}

// rt_trace_entities and rt_pick_entities: rays, or pixels
int entity_sync(RtContext* c, const rtd::Frame& f, const void* in, size_t in_bytes, bool picks, uint32_t count, const RtDrawBox* boxes, uint32_t nboxes,
                const RtDrawStamp* models, uint32_t nmodels, RtRayHit* world_hits, RtEntityHit* entity_hits) {
    const size_t out_bytes = (size_t)count * sizeof(RtEntityHit);   // (of either output)
    return entity_set_sync(c, in, in_bytes, boxes, nboxes, world_hits, out_bytes, entity_hits, out_bytes,
                           [&](hipStream_t st, uint8_t* in_dev, uint8_t* boxes_dev, uint8_t* world_dev, uint8_t* entity_dev) {
                               return entity_launch(c, st, f, picks ? nullptr : in_dev, picks ? in_dev : nullptr, count, boxes_dev, nboxes, models, nmodels,
                                                    world_dev, entity_dev);
                           });
}

// ---- entity sweeps: device sweeps and boxes, host models as rt_draw_stamps'; the entity queries' stream, staging and waits ----------
// checks shared by the two calls; RT_OK when there is work to enqueue, 1 for count == 0
int sweep_entities_check(RtContext* c, const char* fn, uint32_t count, const void* sweeps, const void* lr, const void* entity_hits, const void* boxes,
                         uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels) {
    const char* e = sweep_entities_args_error(count, sweeps, lr, entity_hits, boxes, nboxes, models, nmodels);
    if (e) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": " + e);
    if (count == 0) return 1;
    if (!c->world_resident) return fail(c, RT_ERR_NOT_READY, std::string(fn) + ": upload the full region first");
    return models_check(c, fn, models, nmodels, "nothing was answered");
}

// entity_launch's steps with the sweep kernel in place of the query kernel.
int sweep_entities_launch(RtContext* c, hipStream_t st, const int32_t lr[3], const void* sweeps_dev, uint32_t count, const void* boxes_dev,
                          uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels, void* world_dev, void* entity_dev) {
    ModelBatch b;
    const int rc = models_send(c, models, nmodels, st, &b);
    if (rc != RT_OK) return rc;
    rtd::SweepEntitiesArgs a;
    a.sweeps = reinterpret_cast<const uint4*>(sweeps_dev);
    a.world_hits = reinterpret_cast<uint4*>(world_dev);
    a.entity_hits = reinterpret_cast<uint4*>(entity_dev);
    a.boxes = reinterpret_cast<const uint4*>(boxes_dev);
    a.recs = b.recs();
    a.count = count; a.nboxes = nboxes; a.nmodels = nmodels;
    for (int k = 0; k < 3; k++) a.lr[k] = lr[k];
    RT_HIP(c, rtd::launch_sweep_entities(scene_of(c), c->logr, a, st));
    RT_HIP(c, b.applied(st));
    if (!c->user_stream) RT_HIP(c, c->ev_query.record(st));   // (a caller's stream orders itself)
    return RT_OK;
}
}  // namespace

extern "C" {

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
    const uint32_t out = first_pixel_outside(xy, count, ctx->cfg.width, ctx->cfg.height);
    if (out != count) return fail(ctx, RT_ERR_INVALID_ARG, "rt_pick_pixels: pixel " + std::to_string(out) + " is outside the frame");
    return query_sync(ctx, frame_of(ctx, u), xy, (size_t)count * 8u, true, hits, count);
}

int rt_probe_light(RtContext* ctx, const RtUniforms* u, const RtLightProbe* probes, uint32_t count, uint32_t samples, int32_t depth,
                   RtProbeLight* out) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = probe_check(ctx, "rt_probe_light", u, probes, count, samples, depth, out);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    for (uint32_t i = 0; i < count; i++) {
        if (probes[i].normal > (uint32_t)RT_PROBE_SPHERE)
            return fail(ctx, RT_ERR_INVALID_ARG, "rt_probe_light: probe " + std::to_string(i) + " has a normal above RT_PROBE_SPHERE");
        if (probes[i].reserved[0] || probes[i].reserved[1] || probes[i].reserved[2])
            return fail(ctx, RT_ERR_INVALID_ARG, "rt_probe_light: probe " + std::to_string(i) + " has a non-zero reserved word");
    }
    hipStream_t st;
    rc = query_stream_of(ctx, &st);
    if (rc != RT_OK) return rc;
    // the probes through pinned and device staging, the launches, the results back
    const size_t out_bytes = (size_t)count * sizeof(RtProbeLight);
    uint8_t* dev[2];
    rc = stage_sync(ctx, st, {{probes, (size_t)count * sizeof(RtLightProbe)}, {nullptr, out_bytes}}, dev);
    if (rc != RT_OK) return rc;
    rc = probe_launch(ctx, st, u, dev[0], dev[1], count, samples, depth);
    if (rc != RT_OK) return rc;
    return fetch_sync(ctx, st, dev[1], out, out_bytes);
}

int rt_probe_light_async(RtContext* ctx, const RtUniforms* u, const RtLightProbe* probes_dev, uint32_t count, uint32_t samples,
                         int32_t depth, RtProbeLight* out_dev) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = probe_check(ctx, "rt_probe_light_async", u, probes_dev, count, samples, depth, out_dev);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!query_device_ptr(ctx, probes_dev) || !query_device_ptr(ctx, out_dev))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_probe_light_async: probes and out must be 16-byte aligned memory of the context's device");
    hipStream_t st;
    rc = query_stream_of(ctx, &st);
    if (rc != RT_OK) return rc;
    return probe_launch(ctx, st, u, probes_dev, out_dev, count, samples, depth);
}

int rt_sweep_boxes(RtContext* ctx, const RtBoxSweep* sweeps, uint32_t count, const int32_t lr[3], RtSweepHit* hits) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = sweep_check(ctx, "rt_sweep_boxes", count, sweeps, lr, hits);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    const uint32_t bad = first_invalid_sweep(sweeps, count);   // (sweep_entities_check.hpp: the one host definition of the domain)
    if (bad != count) return fail(ctx, RT_ERR_INVALID_ARG, "rt_sweep_boxes: sweep " + std::to_string(bad) + " is outside the validated domain");
    hipStream_t st;
    rc = query_stream_of(ctx, &st);
    if (rc != RT_OK) return rc;
    // the sweeps through pinned and device staging, the launch, the hits back
    const size_t out_bytes = (size_t)count * sizeof(RtSweepHit);
    uint8_t* dev[2];
    rc = stage_sync(ctx, st, {{sweeps, (size_t)count * sizeof(RtBoxSweep)}, {nullptr, out_bytes}}, dev);
    if (rc != RT_OK) return rc;
    rc = sweep_launch(ctx, st, lr, dev[0], dev[1], count);
    if (rc != RT_OK) return rc;
    return fetch_sync(ctx, st, dev[1], hits, out_bytes);
}

int rt_sweep_boxes_async(RtContext* ctx, const RtBoxSweep* sweeps_dev, uint32_t count, const int32_t lr[3], RtSweepHit* hits_dev) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = sweep_check(ctx, "rt_sweep_boxes_async", count, sweeps_dev, lr, hits_dev);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!query_device_ptr(ctx, sweeps_dev) || !query_device_ptr(ctx, hits_dev))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_sweep_boxes_async: sweeps and hits must be 16-byte aligned memory of the context's device");
    hipStream_t st;
    rc = query_stream_of(ctx, &st);
    if (rc != RT_OK) return rc;
    return sweep_launch(ctx, st, lr, sweeps_dev, hits_dev, count);
}

int rt_step_particles(RtContext* ctx, const RtParticleStep* params, const RtParticleState* in, RtParticleState* out, RtParticle* draw,
                      uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = step_check(ctx, "rt_step_particles", params, in, out, draw, count);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    const uint32_t bad = first_invalid_particle_state(in, count);
    if (bad != count) return fail(ctx, RT_ERR_INVALID_ARG, "rt_step_particles: particle " + std::to_string(bad) + " is not a valid record");
    hipStream_t st;
    rc = query_stream_of(ctx, &st);
    if (rc != RT_OK) return rc;
    // the states through pinned and device staging, the launch in place there, the states and the draw records back
    const size_t state_bytes = (size_t)count * sizeof(RtParticleState), draw_bytes = draw ? (size_t)count * sizeof(RtParticle) : 0u;
    uint8_t* dev[2];
    rc = stage_sync(ctx, st, {{in, state_bytes}, {nullptr, draw_bytes}}, dev);
    if (rc != RT_OK) return rc;
    rc = step_launch(ctx, st, *params, dev[0], dev[0], draw ? dev[1] : nullptr, count);
    if (rc != RT_OK) return rc;
    if (draw) {
        rc = fetch_sync(ctx, st, dev[1], draw, draw_bytes);
        if (rc != RT_OK) return rc;
    }
    return fetch_sync(ctx, st, dev[0], out, state_bytes);
}

int rt_step_particles_async(RtContext* ctx, const RtParticleStep* params, const RtParticleState* in_dev, RtParticleState* out_dev,
                            RtParticle* draw_dev, uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = step_check(ctx, "rt_step_particles_async", params, in_dev, out_dev, draw_dev, count);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!query_device_ptr(ctx, in_dev) || !query_device_ptr(ctx, out_dev) || (draw_dev && !query_device_ptr(ctx, draw_dev)))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_step_particles_async: in, out and draw must be 16-byte aligned memory of the context's device");
    hipStream_t st;
    rc = query_stream_of(ctx, &st);
    if (rc != RT_OK) return rc;
    return step_launch(ctx, st, *params, in_dev, out_dev, draw_dev, count);
}

int rt_emit_particles(RtContext* ctx, const RtParticleEmit* emitters, uint32_t count, const int32_t lr[3], RtParticleState* states,
                      uint32_t capacity, uint32_t max_emit, RtEmitCursor* cursor) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    EmitPlan plan;
    int rc = emit_check(ctx, "rt_emit_particles", emitters, count, lr, states, capacity, max_emit, cursor, cursor, &plan);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    hipStream_t st;
    rc = query_stream_of(ctx, &st);
    if (rc != RT_OK) return rc;
    // A device ring with a cursor of its own at slot 0: particle j lands in slot j there, and comes back into the caller's ring at
    // (next + j) mod capacity.  It holds what the call can emit at the most: max_emit, or 64 per brick of the plan if that is less
    // (N cannot exceed it, so n and the dropped count are what max_emit would give).
    const uint64_t most = 64u * plan.items;
    const uint32_t staged = most < max_emit ? (uint32_t)most : max_emit;
    const RtEmitCursor zero{0u, 0u, 0u, 0u};
    uint8_t* dev[2];
    rc = stage_sync(ctx, st, {{&zero, sizeof zero}, {nullptr, (size_t)staged * sizeof(RtParticleState)}}, dev);
    if (rc != RT_OK) return rc;
    rc = emit_launch(ctx, st, plan, lr, dev[1], staged, staged, dev[0]);
    if (rc != RT_OK) return rc;
    RtEmitCursor got;
    rc = fetch_sync(ctx, st, dev[0], &got, sizeof got);
    if (rc != RT_OK) return rc;
    EmitRun runs[2];
    const uint32_t nruns = emit_ring_runs(cursor->next, got.emitted, capacity, runs);
    for (uint32_t i = 0; i < nruns; i++) {
        rc = fetch_sync(ctx, st, dev[1] + (size_t)runs[i].first * sizeof(RtParticleState), states + runs[i].slot,
                        (size_t)runs[i].count * sizeof(RtParticleState));
        if (rc != RT_OK) return rc;
    }
    cursor->next = (uint32_t)(((uint64_t)cursor->next + got.emitted) % capacity);
    cursor->emitted += got.emitted;
    cursor->dropped += got.dropped;
    return RT_OK;
}

int rt_emit_particles_async(RtContext* ctx, const RtParticleEmit* emitters, uint32_t count, const int32_t lr[3], RtParticleState* states_dev,
                            uint32_t capacity, uint32_t max_emit, RtEmitCursor* cursor_dev) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    EmitPlan plan;
    int rc = emit_check(ctx, "rt_emit_particles_async", emitters, count, lr, states_dev, capacity, max_emit, nullptr, cursor_dev, &plan);
    if (rc != RT_OK && rc != 1) return rc;
    if (count == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!query_device_ptr(ctx, states_dev) || !query_device_ptr(ctx, cursor_dev))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_emit_particles_async: states and cursor must be 16-byte aligned memory of the context's device");
    if (rc == 1) return RT_OK;
    hipStream_t st;
    rc = query_stream_of(ctx, &st);
    if (rc != RT_OK) return rc;
    return emit_launch(ctx, st, plan, lr, states_dev, capacity, max_emit, cursor_dev);
}

int rt_trace_entities(RtContext* ctx, const RtRay* rays, uint32_t count, const int32_t lr[3], const RtDrawBox* boxes, uint32_t nboxes,
                      const RtDrawStamp* models, uint32_t nmodels, RtRayHit* world_hits, RtEntityHit* entity_hits) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const int rc = entity_check(ctx, "rt_trace_entities", count, rays, lr, entity_hits, boxes, nboxes, models, nmodels);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    const uint32_t bad = first_invalid_draw_box(boxes, nboxes);
    if (bad != nboxes) return fail(ctx, RT_ERR_INVALID_ARG, "rt_trace_entities: box " + std::to_string(bad) + " is not a valid box");
    return entity_sync(ctx, query_frame(ctx, lr), rays, (size_t)count * sizeof(RtRay), false, count, boxes, nboxes, models, nmodels, world_hits,
                       entity_hits);
}

int rt_trace_entities_async(RtContext* ctx, const RtRay* rays_dev, uint32_t count, const int32_t lr[3], const RtDrawBox* boxes_dev,
                            uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels, RtRayHit* world_hits_dev,
                            RtEntityHit* entity_hits_dev) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = entity_check(ctx, "rt_trace_entities_async", count, rays_dev, lr, entity_hits_dev, boxes_dev, nboxes, models, nmodels);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!query_device_ptr(ctx, rays_dev) || !query_device_ptr(ctx, entity_hits_dev) || (nboxes > 0u && !query_device_ptr(ctx, boxes_dev)) ||
        (world_hits_dev && !query_device_ptr(ctx, world_hits_dev)))
        return fail(ctx, RT_ERR_INVALID_ARG,
                    "rt_trace_entities_async: rays, boxes and both hits must be 16-byte aligned memory of the context's device");
    hipStream_t st;
    rc = query_stream_of(ctx, &st);
    if (rc != RT_OK) return rc;
    return entity_launch(ctx, st, query_frame(ctx, lr), rays_dev, nullptr, count, nboxes ? boxes_dev : nullptr, nboxes, models, nmodels,
                         world_hits_dev, entity_hits_dev);
}

int rt_pick_entities(RtContext* ctx, const RtUniforms* u, const int32_t* xy, uint32_t count, const RtDrawBox* boxes, uint32_t nboxes,
                     const RtDrawStamp* models, uint32_t nmodels, RtRayHit* world_hits, RtEntityHit* entity_hits) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const int rc = entity_check(ctx, "rt_pick_entities", count, xy, u, entity_hits, boxes, nboxes, models, nmodels);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    const uint32_t out = first_pixel_outside(xy, count, ctx->cfg.width, ctx->cfg.height);
    if (out != count) return fail(ctx, RT_ERR_INVALID_ARG, "rt_pick_entities: pixel " + std::to_string(out) + " is outside the frame");
    const uint32_t bad = first_invalid_draw_box(boxes, nboxes);
    if (bad != nboxes) return fail(ctx, RT_ERR_INVALID_ARG, "rt_pick_entities: box " + std::to_string(bad) + " is not a valid box");
    return entity_sync(ctx, frame_of(ctx, u), xy, (size_t)count * 8u, true, count, boxes, nboxes, models, nmodels, world_hits, entity_hits);
}

int rt_sweep_entities(RtContext* ctx, const RtBoxSweep* sweeps, uint32_t count, const int32_t lr[3], const RtDrawBox* boxes, uint32_t nboxes,
                      const RtDrawStamp* models, uint32_t nmodels, RtSweepHit* world_hits, RtEntitySweepHit* entity_hits) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = sweep_entities_check(ctx, "rt_sweep_entities", count, sweeps, lr, entity_hits, boxes, nboxes, models, nmodels);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    uint32_t bad = first_invalid_sweep(sweeps, count);
    if (bad != count) return fail(ctx, RT_ERR_INVALID_ARG, "rt_sweep_entities: sweep " + std::to_string(bad) + " is outside the validated domain");
    bad = first_invalid_draw_box(boxes, nboxes);
    if (bad != nboxes) return fail(ctx, RT_ERR_INVALID_ARG, "rt_sweep_entities: box " + std::to_string(bad) + " is not a valid box");
    return entity_set_sync(ctx, sweeps, (size_t)count * sizeof(RtBoxSweep), boxes, nboxes, world_hits, (size_t)count * sizeof(RtSweepHit), entity_hits,
                           (size_t)count * sizeof(RtEntitySweepHit),
                           [&](hipStream_t st, uint8_t* sweeps_dev, uint8_t* boxes_dev, uint8_t* world_dev, uint8_t* entity_dev) {
                               return sweep_entities_launch(ctx, st, lr, sweeps_dev, count, boxes_dev, nboxes, models, nmodels, world_dev, entity_dev);
                           });
}

int rt_sweep_entities_async(RtContext* ctx, const RtBoxSweep* sweeps_dev, uint32_t count, const int32_t lr[3], const RtDrawBox* boxes_dev,
                            uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels, RtSweepHit* world_hits_dev,
                            RtEntitySweepHit* entity_hits_dev) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = sweep_entities_check(ctx, "rt_sweep_entities_async", count, sweeps_dev, lr, entity_hits_dev, boxes_dev, nboxes, models, nmodels);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!query_device_ptr(ctx, sweeps_dev) || !query_device_ptr(ctx, entity_hits_dev) || (nboxes > 0u && !query_device_ptr(ctx, boxes_dev)) ||
        (world_hits_dev && !query_device_ptr(ctx, world_hits_dev)))
        return fail(ctx, RT_ERR_INVALID_ARG,
                    "rt_sweep_entities_async: sweeps, boxes and both hits must be 16-byte aligned memory of the context's device");
    hipStream_t st;
    rc = query_stream_of(ctx, &st);
    if (rc != RT_OK) return rc;
    return sweep_entities_launch(ctx, st, lr, sweeps_dev, count, nboxes ? boxes_dev : nullptr, nboxes, models, nmodels, world_hits_dev,
                                 entity_hits_dev);
}

}  // extern "C"
