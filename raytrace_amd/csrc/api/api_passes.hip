// api_passes.hip — the passes over the frame drawn last, each one launch on the stream that frame ended on: entity boxes
// (rt_draw_boxes[_async]), voxel-model entities (rt_draw_stamps[_async]) and particles (rt_draw_particles[_async]: a chain of
// launches over the context's binning scratch) between the frame and its post passes, entity shadows
// (rt_shadow_entities[_async]) behind the entity draws, point lights (rt_add_lights[_async], and rt_add_lights_occluded[_async] with the
// entities as occluders) behind those.  What the passes share is
// here once: the prologue (pass_begin), the verdict on a batch of models (models_check), the models' way to the device
// (upload_models, a caller of rt_context.hpp's staging_claim and staging_send; models_send for the optional models of an entity set,
// which api_query.hip uses too) and the planes a pass writes (planes_written); the synchronous calls' staging is rt_context.hpp's
// stage_sync.
//
// Every launch follows the queries enqueued so far (ev_query): their results may be its records or face lights.  The passes that
// read the region (lights, shadows) find it on their stream: every world change runs there too, the earlier ones in front, and a
// later one — whichever lane's stream it finds as the context's by then — first joins every lane (world_change_begin).
#include "light_shadows_check.hpp"
#include "lights_check.hpp"
#include "particles_check.hpp"
#include "rt_context.hpp"
#include "shadows_check.hpp"

using namespace rta;

namespace rta {
static_assert(sizeof(RtDrawStamp) == 32 && sizeof(DrawStampRecord) == 64, "one 32-byte record per model from the caller, four 16-byte words to the kernels");

// The models of a call, resolved against the live stamps before anything is enqueued; `nothing` ends the refusal.
int models_check(RtContext* c, const std::string& fn, const RtDrawStamp* models, uint32_t n, const char* nothing) {
    const uint32_t bad = draw_stamps_validate(c->stamps, models, n);
    if (bad == n) return RT_OK;
    return fail(c, RT_ERR_INVALID_ARG, fn + ": model " + std::to_string(bad) +
                                           " has an unknown stamp id, orient >= 48, a non-zero reserved field, a scale outside"
                                           " [2^-8, 64] or a corner beyond 2^22; " + nothing);
}

// The device records of `n` (valid) models, and `extra_bytes` of the caller's behind them, through the next of the two staging sets
// (the entity draws, shadows, queries and sweeps and the emitters take turns over the same two, in call order); `reader` — the
// stream whose launch will read the records: the context's for a pass, the query stream for a query — waits for the transfer.  The
// caller launches there and then calls batch->applied(reader).
int upload_models(RtContext* c, const RtDrawStamp* models, uint32_t n, const void* extra_host, size_t extra_bytes, hipStream_t reader, ModelBatch* batch) {
    const size_t rec_bytes = (size_t)n * sizeof(DrawStampRecord), need = rec_bytes + extra_bytes;
    StagingSet& s = c->draw_sets[c->draw_batches & 1u];
    RT_HIP(c, staging_claim(c, s, need, staging_alloc(need)));
    draw_stamp_fill_records(c->stamps, models, n, reinterpret_cast<DrawStampRecord*>(s.host));
    if (extra_bytes) memcpy(s.host + rec_bytes, extra_host, extra_bytes);
    for (uint32_t i = 0; i < n; i++) c->stamps.find(models[i].stamp)->used = true;   // rt_stamp_destroy waits for the launch
    c->draw_batches++;
    RT_HIP(c, staging_send(c, s, need, reader));
    *batch = ModelBatch{&s, s.dev};
    return RT_OK;
}

// The models of an entity set (device boxes plus host models), which may be none.  A stamp made by rt_stamp_capture is written on the
// render stream: a reader that is not the render stream (the query stream) follows the latest capture; on the render stream, a
// caller's included, stream order and the capture's lane fence do it.
int models_send(RtContext* c, const RtDrawStamp* models, uint32_t n, hipStream_t reader, ModelBatch* batch) {
    *batch = ModelBatch{};
    if (n == 0u) return RT_OK;
    const int rc = upload_models(c, models, n, nullptr, 0u, reader, batch);
    if (rc != RT_OK) return rc;
    if (reader != c->stream) RT_HIP(c, c->ev_capture.wait(reader));
    return RT_OK;
}
}  // namespace rta

namespace {
constexpr uint32_t kMaxDrawBoxes = 4096;
static_assert(sizeof(RtDrawBox) == 32 && sizeof(RtProbeLight) == 16, "the kernels read two 16-byte words per box and one per face light");
static_assert(sizeof(RtPointLight) == 32, "the kernel reads two 16-byte words per light");

// What is wrong with the plain arguments of a pass with one batch, or nullptr (shadow_args_error is the form with two batches).
const char* batch_args_error(const void* u, const char* too_many, bool null_pointer) {
    if (!u) return "null uniforms";
    if (too_many) return too_many;
    return null_pointer ? "null pointer" : nullptr;
}

// The prologue of every pass: the verdict on its plain arguments, then the context's state.  RT_OK with *work = false: a valid call
// with no record, which enqueues nothing.
int pass_begin(RtContext* c, const std::string& fn, const char* args_error, bool reads_world, uint32_t records, bool* work) {
    *work = false;
    if (args_error) return fail(c, RT_ERR_INVALID_ARG, fn + ": " + args_error);
    if (c->cfg.tile_world != 1) return fail(c, RT_ERR_UNIMPLEMENTED, fn + ": whole-frame contexts only");
    if (!c->frame_recorded) return fail(c, RT_ERR_NOT_READY, fn + ": no frame drawn yet");
    if (reads_world && !c->world_resident) return fail(c, RT_ERR_NOT_READY, fn + ": upload the full region first");
    *work = records > 0u;
    return RT_OK;
}

// The slot's prepass no longer describes the planes a pass writes: a still camera must not carry entity pixels, light or shadow into
// the next frame.  The draws write the geometry planes too, the lighting passes the two lighting planes only.
void planes_written(RtContext* c, bool geometry_too) {
    if (geometry_too)
        for (int b : {RT_BUF_DEPTH_F32, RT_BUF_DEPTH_R16UI, RT_BUF_NORMAL_R8UI, RT_BUF_ALBEDO_RGBA8, RT_BUF_EMISSION_RGBA8}) plane_written(c, c->planes[b]);
    for (int b : {RT_BUF_LIGHTING_F32, RT_BUF_LIGHTING_RGBA16}) plane_written(c, c->planes[b]);
}

// the camera of the frame the planes hold (DrawBoxesArgs, DrawStampsArgs)
template <typename Args>
void set_camera(Args& a, const RtUniforms* u, const RtConfig& cfg) {
    a.width = cfg.width; a.height = cfg.height;
    for (int k = 0; k < 3; k++) { a.origin[k] = u->origin[k]; a.forward[k] = u->forward[k]; a.up[k] = u->up[k]; a.right[k] = u->right[k]; }
}

// ---- entity boxes ---------------------------------------------------------------------------------------------------------------
int draw_boxes_begin(RtContext* c, const char* fn, const RtUniforms* u, const void* boxes, const void* lights, uint32_t count, bool* work) {
    return pass_begin(c, fn, batch_args_error(u, count > kMaxDrawBoxes ? "more than 4096 boxes in one call" : nullptr, count > 0u && (!boxes || !lights)),
                      false, count, work);
}

int draw_boxes_launch(RtContext* c, const RtUniforms* u, const void* boxes_dev, const void* lights_dev, uint32_t count) {
    planes_written(c, true);
    RT_HIP(c, c->ev_query.wait_elsewhere(c->stream));
    rtd::DrawBoxesArgs a;
    a.boxes = reinterpret_cast<const uint4*>(boxes_dev);
    a.lights = reinterpret_cast<const float4*>(lights_dev);
    a.count = count;
    set_camera(a, u, c->cfg);
    LaunchTimer t(c, 1);
    RT_HIP(c, rtd::launch_draw_boxes(planes_of(c), a, c->stream));
    return RT_OK;
}

// ---- particles ------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(RtParticle) == 32, "the kernels read two 16-byte words per particle");
static_assert(kMaxDrawParticles == rtd::kMaxParticles, "the host's limit is the kernels'");

int draw_particles_begin(RtContext* c, const char* fn, const RtUniforms* u, const void* particles, uint32_t count, const void* lights, uint32_t nlights,
                         bool* work) {
    return pass_begin(c, fn, particle_args_error(u, particles, count, lights, nlights), false, count, work);
}

int draw_particles_launch(RtContext* c, const RtUniforms* u, const void* particles_dev, uint32_t count, const void* lights_dev, uint32_t nlights) {
    const int rc = particle_scratch_reserve(c, rtd::particle_scratch_words(count, c->cfg.width, c->cfg.height));
    if (rc != RT_OK) return rc;
    planes_written(c, true);
    RT_HIP(c, c->ev_query.wait_elsewhere(c->stream));
    RT_HIP(c, c->ev_particles.wait_elsewhere(c->stream));   // the scratch is the previous call's until its draw has run
    rtd::ParticleArgs a;
    a.particles = reinterpret_cast<const uint4*>(particles_dev);
    a.lights = reinterpret_cast<const float4*>(lights_dev);
    a.scratch = c->particle_scratch;
    a.count = count; a.nlights = nlights;
    set_camera(a, u, c->cfg);
    {
        LaunchTimer t(c, 1);
        RT_HIP(c, rtd::launch_draw_particles(planes_of(c), a, c->stream));
    }
    RT_HIP(c, c->ev_particles.record(c->stream));
    return RT_OK;
}

// ---- point lights ---------------------------------------------------------------------------------------------------------------
int add_lights_begin(RtContext* c, const char* fn, const RtUniforms* u, const void* lights, uint32_t count, bool* work) {
    return pass_begin(c, fn, batch_args_error(u, count > kMaxPointLights ? "more than 1024 lights in one call" : nullptr, count > 0u && !lights), true,
                      count, work);
}

int add_lights_launch(RtContext* c, const RtUniforms* u, const void* lights_dev, uint32_t count) {
    planes_written(c, false);
    RT_HIP(c, c->ev_query.wait_elsewhere(c->stream));
    rtd::LightsArgs a;
    a.lights = reinterpret_cast<const uint4*>(lights_dev);
    a.count = count;
    LaunchTimer t(c, 1);
    RT_HIP(c, rtd::launch_add_lights(scene_of(c), frame_of(c, u), planes_of(c), a, c->stream));
    return RT_OK;
}

// ---- voxel-model entities: the models are host records in both calls ------------------------------------------------------------
int draw_stamps_begin(RtContext* c, const char* fn, const RtUniforms* u, const RtDrawStamp* models, const void* lights, uint32_t count, bool* work) {
    const int rc = pass_begin(c, fn, batch_args_error(u, count > kMaxDrawStamps ? "more than 4096 models in one call" : nullptr, count > 0u && (!models || !lights)),
                              false, count, work);
    return rc == RT_OK && *work ? models_check(c, fn, models, count, "nothing was drawn") : rc;
}

// `lights_host` (the synchronous call's 6 * count face lights) travels behind the records; the asynchronous call names `lights_dev`.
int draw_stamps_enqueue(RtContext* c, const RtUniforms* u, const RtDrawStamp* models, const RtProbeLight* lights_host,
                        const RtProbeLight* lights_dev, uint32_t count) {
    RT_HIP(c, hipSetDevice(c->device));
    ModelBatch b;
    const int rc = upload_models(c, models, count, lights_host, lights_host ? (size_t)count * 6u * sizeof(RtProbeLight) : 0u, c->stream, &b);
    if (rc != RT_OK) return rc;
    planes_written(c, true);
    RT_HIP(c, c->ev_query.wait_elsewhere(c->stream));
    rtd::DrawStampsArgs a;
    a.recs = b.recs();
    a.lights = reinterpret_cast<const float4*>(lights_host ? reinterpret_cast<const RtProbeLight*>(b.dev + (size_t)count * sizeof(DrawStampRecord)) : lights_dev);
    a.count = count;
    set_camera(a, u, c->cfg);
    {
        LaunchTimer t(c, 1);
        RT_HIP(c, rtd::launch_draw_stamps(planes_of(c), a, c->stream));
    }
    RT_HIP(c, b.applied(c->stream));
    return RT_OK;
}

// ---- entity shadows: device boxes (staged by the synchronous call), host models as rt_draw_stamps' ------------------------------
int shadow_begin(RtContext* c, const char* fn, const RtUniforms* u, const void* boxes, uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels,
                 float strength, bool* work) {
    const int rc = pass_begin(c, fn, shadow_args_error(u, boxes, nboxes, models, nmodels, strength), true, nboxes + nmodels, work);
    return rc == RT_OK && *work ? models_check(c, fn, models, nmodels, "nothing was changed") : rc;
}

int shadow_enqueue(RtContext* c, const RtUniforms* u, const void* boxes_dev, uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels,
                   float strength) {
    const rtd::Frame f = frame_of(c, u);
    rtd::ShadowArgs a;
    ModelBatch b;
    const int rc = models_send(c, models, nmodels, c->stream, &b);
    if (rc != RT_OK) return rc;
    a.boxes = reinterpret_cast<const uint4*>(boxes_dev);
    a.recs = b.recs();
    a.nboxes = nboxes; a.nmodels = nmodels;
    a.strength = strength;
    planes_written(c, false);
    RT_HIP(c, c->ev_query.wait_elsewhere(c->stream));
    {
        LaunchTimer t(c, 1);
        RT_HIP(c, rtd::launch_shadow_entities(scene_of(c), f, planes_of(c), a, c->stream));
    }
    RT_HIP(c, b.applied(c->stream));
    return RT_OK;
}

// ---- point lights with the entities as occluders: device lights and boxes (staged by the synchronous call), host models ----------
int lights_occluded_begin(RtContext* c, const char* fn, const RtUniforms* u, const void* lights, uint32_t count, const void* boxes, uint32_t nboxes,
                          const RtDrawStamp* models, uint32_t nmodels, bool* work) {
    const int rc = pass_begin(c, fn, light_shadow_args_error(u, lights, count, boxes, nboxes, models, nmodels), true, count, work);
    return rc == RT_OK && *work ? models_check(c, fn, models, nmodels, "nothing was changed") : rc;
}

// With no occluder the call is rt_add_lights, every bit and every side effect.
int lights_occluded_enqueue(RtContext* c, const RtUniforms* u, const void* lights_dev, uint32_t count, const void* boxes_dev, uint32_t nboxes,
                            const RtDrawStamp* models, uint32_t nmodels) {
    if (nboxes + nmodels == 0u) return add_lights_launch(c, u, lights_dev, count);
    const rtd::Frame f = frame_of(c, u);
    rtd::LightShadowArgs a;
    ModelBatch b;
    const int rc = models_send(c, models, nmodels, c->stream, &b);
    if (rc != RT_OK) return rc;
    a.lights = reinterpret_cast<const uint4*>(lights_dev);
    a.boxes = reinterpret_cast<const uint4*>(boxes_dev);
    a.recs = b.recs();
    a.count = count; a.nboxes = nboxes; a.nmodels = nmodels;
    planes_written(c, false);
    RT_HIP(c, c->ev_query.wait_elsewhere(c->stream));
    {
        LaunchTimer t(c, 1);
        RT_HIP(c, rtd::launch_add_lights_occluded(scene_of(c), f, planes_of(c), a, c->stream));
    }
    RT_HIP(c, b.applied(c->stream));
    return RT_OK;
}

// night: the frame has no sun term
bool sun_is_dark(const RtContext* c, const RtUniforms* u) {
    const rtd::Frame f = frame_of(c, u);
    return shadow_sun_is_dark(f.sunlight);
}

// the end of a synchronous call: it waits for its launch
int finish_sync(RtContext* c, int rc) {
    if (rc != RT_OK) return rc;
    RT_HIP(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}
}  // namespace

extern "C" {

int rt_draw_boxes(RtContext* ctx, const RtUniforms* u, const RtDrawBox* boxes, const RtProbeLight* face_lights, uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    bool work;
    int rc = draw_boxes_begin(ctx, "rt_draw_boxes", u, boxes, face_lights, count, &work);
    if (rc != RT_OK || !work) return rc;
    const uint32_t bad = first_invalid_draw_box(boxes, count);
    if (bad != count) return fail(ctx, RT_ERR_INVALID_ARG, "rt_draw_boxes: box " + std::to_string(bad) + " is not a valid box");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    uint8_t* dev[2];
    rc = stage_sync(ctx, ctx->stream, {{boxes, (size_t)count * sizeof(RtDrawBox)}, {face_lights, (size_t)count * 6u * sizeof(RtProbeLight)}}, dev);
    if (rc != RT_OK) return rc;
    return finish_sync(ctx, draw_boxes_launch(ctx, u, dev[0], dev[1], count));
}

int rt_draw_boxes_async(RtContext* ctx, const RtUniforms* u, const RtDrawBox* boxes_dev, const RtProbeLight* face_lights_dev, uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    bool work;
    const int rc = draw_boxes_begin(ctx, "rt_draw_boxes_async", u, boxes_dev, face_lights_dev, count, &work);
    if (rc != RT_OK || !work) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!query_device_ptr(ctx, boxes_dev) || !query_device_ptr(ctx, face_lights_dev))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_draw_boxes_async: boxes and face_lights must be 16-byte aligned memory of the context's device");
    return draw_boxes_launch(ctx, u, boxes_dev, face_lights_dev, count);
}

int rt_draw_particles(RtContext* ctx, const RtUniforms* u, const RtParticle* particles, uint32_t count, const RtProbeLight* lights, uint32_t nlights) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    bool work;
    int rc = draw_particles_begin(ctx, "rt_draw_particles", u, particles, count, lights, nlights, &work);
    if (rc != RT_OK || !work) return rc;
    const uint32_t bad = first_invalid_particle(particles, count, nlights);
    if (bad != count) return fail(ctx, RT_ERR_INVALID_ARG, "rt_draw_particles: particle " + std::to_string(bad) + " is not a valid particle");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    uint8_t* dev[2];
    rc = stage_sync(ctx, ctx->stream, {{particles, (size_t)count * sizeof(RtParticle)}, {lights, (size_t)nlights * sizeof(RtProbeLight)}}, dev);
    if (rc != RT_OK) return rc;
    return finish_sync(ctx, draw_particles_launch(ctx, u, dev[0], count, dev[1], nlights));
}

int rt_draw_particles_async(RtContext* ctx, const RtUniforms* u, const RtParticle* particles_dev, uint32_t count, const RtProbeLight* lights_dev,
                            uint32_t nlights) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    bool work;
    const int rc = draw_particles_begin(ctx, "rt_draw_particles_async", u, particles_dev, count, lights_dev, nlights, &work);
    if (rc != RT_OK || !work) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!query_device_ptr(ctx, particles_dev) || !query_device_ptr(ctx, lights_dev))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_draw_particles_async: particles and lights must be 16-byte aligned memory of the context's device");
    return draw_particles_launch(ctx, u, particles_dev, count, lights_dev, nlights);
}

int rt_add_lights(RtContext* ctx, const RtUniforms* u, const RtPointLight* lights, uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    bool work;
    int rc = add_lights_begin(ctx, "rt_add_lights", u, lights, count, &work);
    if (rc != RT_OK || !work) return rc;
    const uint32_t bad = first_invalid_point_light(lights, count);
    if (bad != count) return fail(ctx, RT_ERR_INVALID_ARG, "rt_add_lights: light " + std::to_string(bad) + " is not a valid light");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    uint8_t* dev;
    rc = stage_sync(ctx, ctx->stream, {{lights, (size_t)count * sizeof(RtPointLight)}}, &dev);
    if (rc != RT_OK) return rc;
    return finish_sync(ctx, add_lights_launch(ctx, u, dev, count));
}

int rt_add_lights_async(RtContext* ctx, const RtUniforms* u, const RtPointLight* lights_dev, uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    bool work;
    const int rc = add_lights_begin(ctx, "rt_add_lights_async", u, lights_dev, count, &work);
    if (rc != RT_OK || !work) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!query_device_ptr(ctx, lights_dev))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_add_lights_async: lights must be 16-byte aligned memory of the context's device");
    return add_lights_launch(ctx, u, lights_dev, count);
}

int rt_draw_stamps(RtContext* ctx, const RtUniforms* u, const RtDrawStamp* models, const RtProbeLight* face_lights, uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    bool work;
    const int rc = draw_stamps_begin(ctx, "rt_draw_stamps", u, models, face_lights, count, &work);
    if (rc != RT_OK || !work) return rc;
    return finish_sync(ctx, draw_stamps_enqueue(ctx, u, models, face_lights, nullptr, count));
}

int rt_draw_stamps_async(RtContext* ctx, const RtUniforms* u, const RtDrawStamp* models, const RtProbeLight* face_lights_dev, uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    bool work;
    const int rc = draw_stamps_begin(ctx, "rt_draw_stamps_async", u, models, face_lights_dev, count, &work);
    if (rc != RT_OK || !work) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!query_device_ptr(ctx, face_lights_dev))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_draw_stamps_async: face_lights_dev must be 16-byte aligned memory of the context's device");
    return draw_stamps_enqueue(ctx, u, models, nullptr, face_lights_dev, count);
}

int rt_shadow_entities(RtContext* ctx, const RtUniforms* u, const RtDrawBox* boxes, uint32_t nboxes, const RtDrawStamp* models,
                       uint32_t nmodels, float strength) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    bool work;
    int rc = shadow_begin(ctx, "rt_shadow_entities", u, boxes, nboxes, models, nmodels, strength, &work);
    if (rc != RT_OK || !work) return rc;
    const uint32_t bad = first_invalid_draw_box(boxes, nboxes);
    if (bad != nboxes) return fail(ctx, RT_ERR_INVALID_ARG, "rt_shadow_entities: box " + std::to_string(bad) + " is not a valid box");
    if (sun_is_dark(ctx, u)) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    uint8_t* boxes_dev = nullptr;
    if (nboxes > 0u) {
        rc = stage_sync(ctx, ctx->stream, {{boxes, (size_t)nboxes * sizeof(RtDrawBox)}}, &boxes_dev);
        if (rc != RT_OK) return rc;
    }
    return finish_sync(ctx, shadow_enqueue(ctx, u, boxes_dev, nboxes, models, nmodels, strength));
}

int rt_shadow_entities_async(RtContext* ctx, const RtUniforms* u, const RtDrawBox* boxes_dev, uint32_t nboxes, const RtDrawStamp* models,
                             uint32_t nmodels, float strength) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    bool work;
    const int rc = shadow_begin(ctx, "rt_shadow_entities_async", u, boxes_dev, nboxes, models, nmodels, strength, &work);
    if (rc != RT_OK || !work) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (nboxes > 0u && !query_device_ptr(ctx, boxes_dev))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_shadow_entities_async: boxes_dev must be 16-byte aligned memory of the context's device");
    if (sun_is_dark(ctx, u)) return RT_OK;
    return shadow_enqueue(ctx, u, boxes_dev, nboxes, models, nmodels, strength);
}

int rt_add_lights_occluded(RtContext* ctx, const RtUniforms* u, const RtPointLight* lights, uint32_t count, const RtDrawBox* boxes, uint32_t nboxes,
                           const RtDrawStamp* models, uint32_t nmodels) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    bool work;
    int rc = lights_occluded_begin(ctx, "rt_add_lights_occluded", u, lights, count, boxes, nboxes, models, nmodels, &work);
    if (rc != RT_OK || !work) return rc;
    uint32_t bad;
    const int which = light_shadow_first_invalid(lights, count, boxes, nboxes, &bad);
    if (which != 0)
        return fail(ctx, RT_ERR_INVALID_ARG, std::string("rt_add_lights_occluded: ") + (which == 1 ? "light " : "box ") + std::to_string(bad) +
                                                 (which == 1 ? " is not a valid light" : " is not a valid box"));
    RT_HIP(ctx, hipSetDevice(ctx->device));
    uint8_t* dev[2];
    rc = stage_sync(ctx, ctx->stream, {{lights, (size_t)count * sizeof(RtPointLight)}, {boxes, (size_t)nboxes * sizeof(RtDrawBox)}}, dev);
    if (rc != RT_OK) return rc;
    return finish_sync(ctx, lights_occluded_enqueue(ctx, u, dev[0], count, dev[1], nboxes, models, nmodels));
}

int rt_add_lights_occluded_async(RtContext* ctx, const RtUniforms* u, const RtPointLight* lights_dev, uint32_t count, const RtDrawBox* boxes_dev,
                                 uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    bool work;
    const int rc = lights_occluded_begin(ctx, "rt_add_lights_occluded_async", u, lights_dev, count, boxes_dev, nboxes, models, nmodels, &work);
    if (rc != RT_OK || !work) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!query_device_ptr(ctx, lights_dev) || (nboxes > 0u && !query_device_ptr(ctx, boxes_dev)))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_add_lights_occluded_async: lights_dev and boxes_dev must be 16-byte aligned memory of the context's device");
    return lights_occluded_enqueue(ctx, u, lights_dev, count, boxes_dev, nboxes, models, nmodels);
}

}  // extern "C"
