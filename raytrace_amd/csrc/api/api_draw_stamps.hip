// api_draw_stamps.hip — voxel-model entities (rt_draw_stamps, rt_draw_stamps_async): one launch on the stream of the frame drawn
// last, between that frame and its post passes, as for the entity boxes.  The models are host records in both calls: their ids,
// extents and orientations are resolved and validated here (draw_stamps.hpp) and one 64-byte record per model travels.
#include "rt_context.hpp"

using namespace rta;

namespace {
static_assert(sizeof(RtDrawStamp) == 32 && sizeof(RtProbeLight) == 16, "one 32-byte record per model, one 16-byte word per face light");

// checks shared by the two calls, all of them before anything is enqueued; RT_OK when there is work to enqueue, 1 for count == 0
int draw_stamps_check(RtContext* c, const char* fn, const RtUniforms* u, const RtDrawStamp* models, const void* lights, uint32_t count) {
    const std::string w(fn);
    if (!u) return fail(c, RT_ERR_INVALID_ARG, w + ": null uniforms");
    if (count > kMaxDrawStamps) return fail(c, RT_ERR_INVALID_ARG, w + ": more than 4096 models in one call");
    if (count > 0u && (!models || !lights)) return fail(c, RT_ERR_INVALID_ARG, w + ": null pointer");
    if (c->cfg.tile_world != 1) return fail(c, RT_ERR_UNIMPLEMENTED, w + ": whole-frame contexts only");
    if (!c->frame_recorded) return fail(c, RT_ERR_NOT_READY, w + ": no frame drawn yet");
    if (count == 0u) return 1;
    const uint32_t bad = draw_stamps_validate(c->stamps, models, count);
    if (bad != count)
        return fail(c, RT_ERR_INVALID_ARG, w + ": model " + std::to_string(bad) +
                                               " has an unknown stamp id, orient >= 48, a non-zero reserved field, a scale outside"
                                               " [2^-8, 64] or a corner beyond 2^22; nothing was drawn");
    return RT_OK;
}

// The records (and, from the synchronous call, `lights` = 6 * count host face lights behind them) through the next staging set, then
// the launch on the stream the frame drawn last ended on, behind the queries enqueued so far (their results may be its face lights).
int draw_stamps_enqueue(RtContext* c, const RtUniforms* u, const RtDrawStamp* models, const RtProbeLight* lights_host,
                        const RtProbeLight* lights_dev, uint32_t count) {
    RT_HIP(c, hipSetDevice(c->device));
    const size_t rec_bytes = (size_t)count * sizeof(DrawStampRecord), light_bytes = lights_host ? (size_t)count * 6u * sizeof(RtProbeLight) : 0u;
    const size_t need = rec_bytes + light_bytes;
    StagingSet& s = c->draw_sets[c->draw_batches & 1u];
    if (!c->upload_stream) RT_HIP(c, new_stream(c, &c->upload_stream));
    for (hipEvent_t* ev : {&s.ev_copied.ev, &s.ev_applied.ev})
        if (!*ev) RT_HIP(c, new_event(c, ev));
    // the set's previous transfer has left the host block; a set that must grow waits for the launch that reads its device block
    RT_HIP(c, s.ev_copied.host_wait());
    s.ev_copied.forget();
    if (need > s.cap) {
        RT_HIP(c, s.ev_applied.host_wait());
        s.ev_applied.forget();
        RT_HIP(c, s.grow(c, need, need < ((size_t)64 << 10) ? ((size_t)64 << 10) : need + need / 2u));
    }
    draw_stamp_fill_records(c->stamps, models, count, reinterpret_cast<DrawStampRecord*>(s.host));
    if (lights_host) memcpy(s.host + rec_bytes, lights_host, light_bytes);
    for (uint32_t i = 0; i < count; i++) c->stamps.find(models[i].stamp)->used = true;   // rt_stamp_destroy waits for this draw
    c->draw_batches++;
    // the slot's prepass no longer describes its planes: a still camera must not carry entity pixels into the next frame
    for (int b : {RT_BUF_DEPTH_F32, RT_BUF_DEPTH_R16UI, RT_BUF_NORMAL_R8UI, RT_BUF_ALBEDO_RGBA8, RT_BUF_EMISSION_RGBA8, RT_BUF_LIGHTING_F32,
                  RT_BUF_LIGHTING_RGBA16})
        plane_written(c, c->planes[b]);
    // the transfer on the upload stream, so that it does not queue behind the frame; it follows the set's previous launch
    RT_HIP(c, s.ev_applied.wait(c->upload_stream));
    RT_HIP(c, hipMemcpyAsync(s.dev, s.host, need, hipMemcpyHostToDevice, c->upload_stream));
    RT_HIP(c, s.ev_copied.record(c->upload_stream));
    RT_HIP(c, hipStreamWaitEvent(c->stream, s.ev_copied.ev, 0));
    RT_HIP(c, c->ev_query.wait_elsewhere(c->stream));
    rtd::DrawStampsArgs a;
    a.recs = reinterpret_cast<const uint4*>(s.dev);
    a.lights = reinterpret_cast<const float4*>(lights_host ? reinterpret_cast<const RtProbeLight*>(s.dev + rec_bytes) : lights_dev);
    a.count = count;
    a.width = c->cfg.width; a.height = c->cfg.height;
    for (int k = 0; k < 3; k++) { a.origin[k] = u->origin[k]; a.forward[k] = u->forward[k]; a.up[k] = u->up[k]; a.right[k] = u->right[k]; }
    {
        LaunchTimer t(c, 1);
        RT_HIP(c, rtd::launch_draw_stamps(planes_of(c), a, c->stream));
    }
    RT_HIP(c, s.ev_applied.record(c->stream));
    return RT_OK;
}
}  // namespace

extern "C" {

int rt_draw_stamps(RtContext* ctx, const RtUniforms* u, const RtDrawStamp* models, const RtProbeLight* face_lights, uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = draw_stamps_check(ctx, "rt_draw_stamps", u, models, face_lights, count);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    rc = draw_stamps_enqueue(ctx, u, models, face_lights, nullptr, count);
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_draw_stamps_async(RtContext* ctx, const RtUniforms* u, const RtDrawStamp* models, const RtProbeLight* face_lights_dev, uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const int rc = draw_stamps_check(ctx, "rt_draw_stamps_async", u, models, face_lights_dev, count);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!query_device_ptr(ctx, face_lights_dev))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_draw_stamps_async: face_lights_dev must be 16-byte aligned memory of the context's device");
    return draw_stamps_enqueue(ctx, u, models, nullptr, face_lights_dev, count);
}

}  // extern "C"
