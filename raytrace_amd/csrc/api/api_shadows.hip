// api_shadows.hip — entity shadows (rt_shadow_entities, rt_shadow_entities_async): one launch on the stream of the frame drawn
// last, behind that frame and its entity draws and in front of the point lights and the post passes.  The boxes are device records
// (staged here by the synchronous call); the models are host records in both calls, resolved and validated here as rt_draw_stamps
// does it (draw_stamps.hpp), and travel through the same staging sets.
#include "rt_context.hpp"
#include "shadows_check.hpp"

using namespace rta;

namespace {
static_assert(sizeof(RtDrawBox) == 32 && sizeof(DrawStampRecord) == 64, "the kernel reads two 16-byte words per box and four per model");

// checks shared by the two calls, all of them before anything is enqueued; RT_OK when there is work to enqueue, 1 when there is none
int shadow_check(RtContext* c, const char* fn, const RtUniforms* u, const void* boxes, uint32_t nboxes, const RtDrawStamp* models,
                 uint32_t nmodels, float strength) {
    const std::string w(fn);
    if (const char* what = shadow_args_error(u, boxes, nboxes, models, nmodels, strength)) return fail(c, RT_ERR_INVALID_ARG, w + ": " + what);
    if (c->cfg.tile_world != 1) return fail(c, RT_ERR_UNIMPLEMENTED, w + ": whole-frame contexts only");
    if (!c->frame_recorded) return fail(c, RT_ERR_NOT_READY, w + ": no frame drawn yet");
    if (!c->world_resident) return fail(c, RT_ERR_NOT_READY, w + ": upload the full region first");
    if (nboxes + nmodels == 0u) return 1;
    const uint32_t bad = draw_stamps_validate(c->stamps, models, nmodels);
    if (bad != nmodels)
        return fail(c, RT_ERR_INVALID_ARG, w + ": model " + std::to_string(bad) +
                                               " has an unknown stamp id, orient >= 48, a non-zero reserved field, a scale outside"
                                               " [2^-8, 64] or a corner beyond 2^22; nothing was changed");
    return RT_OK;
}

// The model records through the next staging set (as rt_draw_stamps'), then the launch on the stream the frame drawn last ended on.
// It reads the region there: every world change runs on that stream too, the earlier ones in front of it, and a later one first
// joins every lane (world_change_begin), this one among them.  Queries enqueued so far may have produced the boxes.
int shadow_enqueue(RtContext* c, const RtUniforms* u, const void* boxes_dev, uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels,
                   float strength) {
    const rtd::Frame f = frame_of(c, u);
    rtd::ShadowArgs a;
    a.boxes = reinterpret_cast<const uint4*>(boxes_dev);
    a.recs = nullptr;
    a.nboxes = nboxes; a.nmodels = nmodels;
    a.strength = strength;
    StagingSet* s = nullptr;
    if (nmodels > 0u) {
        const size_t need = (size_t)nmodels * sizeof(DrawStampRecord);
        s = &c->draw_sets[c->draw_batches & 1u];
        if (!c->upload_stream) RT_HIP(c, new_stream(c, &c->upload_stream));
        for (hipEvent_t* ev : {&s->ev_copied.ev, &s->ev_applied.ev})
            if (!*ev) RT_HIP(c, new_event(c, ev));
        // the set's previous transfer has left the host block; a set that must grow waits for the launch that reads its device block
        RT_HIP(c, s->ev_copied.host_wait());
        s->ev_copied.forget();
        if (need > s->cap) {
            RT_HIP(c, s->ev_applied.host_wait());
            s->ev_applied.forget();
            RT_HIP(c, s->grow(c, need, need < ((size_t)64 << 10) ? ((size_t)64 << 10) : need + need / 2u));
        }
        draw_stamp_fill_records(c->stamps, models, nmodels, reinterpret_cast<DrawStampRecord*>(s->host));
        for (uint32_t i = 0; i < nmodels; i++) c->stamps.find(models[i].stamp)->used = true;   // rt_stamp_destroy waits for this launch
        c->draw_batches++;
        RT_HIP(c, s->ev_applied.wait(c->upload_stream));
        RT_HIP(c, hipMemcpyAsync(s->dev, s->host, need, hipMemcpyHostToDevice, c->upload_stream));
        RT_HIP(c, s->ev_copied.record(c->upload_stream));
        RT_HIP(c, hipStreamWaitEvent(c->stream, s->ev_copied.ev, 0));
        a.recs = reinterpret_cast<const uint4*>(s->dev);
    }
    // the slot's prepass no longer describes its planes: a still camera must not carry the shadow into the next frame
    for (int b : {RT_BUF_LIGHTING_F32, RT_BUF_LIGHTING_RGBA16}) plane_written(c, c->planes[b]);
    RT_HIP(c, c->ev_query.wait_elsewhere(c->stream));
    {
        LaunchTimer t(c, 1);
        RT_HIP(c, rtd::launch_shadow_entities(scene_of(c), f, planes_of(c), a, c->stream));
    }
    if (s) RT_HIP(c, s->ev_applied.record(c->stream));
    return RT_OK;
}

// night: the frame has no sun term
bool sun_is_dark(const RtContext* c, const RtUniforms* u) {
    const rtd::Frame f = frame_of(c, u);
    return shadow_sun_is_dark(f.sunlight);
}
}  // namespace

extern "C" {

int rt_shadow_entities(RtContext* ctx, const RtUniforms* u, const RtDrawBox* boxes, uint32_t nboxes, const RtDrawStamp* models,
                       uint32_t nmodels, float strength) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = shadow_check(ctx, "rt_shadow_entities", u, boxes, nboxes, models, nmodels, strength);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    const uint32_t bad = first_invalid_shadow_box(boxes, nboxes);
    if (bad != nboxes) return fail(ctx, RT_ERR_INVALID_ARG, "rt_shadow_entities: box " + std::to_string(bad) + " is not a valid box");
    if (sun_is_dark(ctx, u)) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const void* boxes_dev = nullptr;
    if (nboxes > 0u) {
        // the boxes through pinned and device staging (the previous synchronous call has finished with the staging: it waited for
        // its launch)
        const size_t need = (size_t)nboxes * sizeof(RtDrawBox);
        StagingBlock& q = ctx->query_block;
        RT_HIP(ctx, q.grow(ctx, need, need < ((size_t)64 << 10) ? ((size_t)64 << 10) : need + need / 2u));
        memcpy(q.host, boxes, need);
        RT_HIP(ctx, hipMemcpyAsync(q.dev, q.host, need, hipMemcpyHostToDevice, ctx->stream));
        boxes_dev = q.dev;
    }
    rc = shadow_enqueue(ctx, u, boxes_dev, nboxes, models, nmodels, strength);
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_shadow_entities_async(RtContext* ctx, const RtUniforms* u, const RtDrawBox* boxes_dev, uint32_t nboxes, const RtDrawStamp* models,
                             uint32_t nmodels, float strength) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const int rc = shadow_check(ctx, "rt_shadow_entities_async", u, boxes_dev, nboxes, models, nmodels, strength);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (nboxes > 0u && !query_device_ptr(ctx, boxes_dev))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_shadow_entities_async: boxes_dev must be 16-byte aligned memory of the context's device");
    if (sun_is_dark(ctx, u)) return RT_OK;
    return shadow_enqueue(ctx, u, boxes_dev, nboxes, models, nmodels, strength);
}

}  // extern "C"
