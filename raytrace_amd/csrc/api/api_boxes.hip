// api_boxes.hip — entity boxes (rt_draw_boxes, rt_draw_boxes_async): one launch on the stream of the frame drawn last, between that
// frame and its post passes.
#include "rt_context.hpp"

using namespace rta;

namespace {
constexpr uint32_t kMaxDrawBoxes = 4096;
static_assert(sizeof(RtDrawBox) == 32 && sizeof(RtProbeLight) == 16, "the kernel reads two 16-byte words per box and one per face light");

// checks shared by the two calls; RT_OK when there is work to enqueue, 1 for count == 0
int draw_boxes_check(RtContext* c, const char* fn, const RtUniforms* u, const void* boxes, const void* lights, uint32_t count) {
    const std::string w(fn);
    if (!u) return fail(c, RT_ERR_INVALID_ARG, w + ": null uniforms");
    if (count > kMaxDrawBoxes) return fail(c, RT_ERR_INVALID_ARG, w + ": more than 4096 boxes in one call");
    if (count > 0u && (!boxes || !lights)) return fail(c, RT_ERR_INVALID_ARG, w + ": null pointer");
    if (c->cfg.tile_world != 1) return fail(c, RT_ERR_UNIMPLEMENTED, w + ": whole-frame contexts only");
    if (!c->frame_recorded) return fail(c, RT_ERR_NOT_READY, w + ": no frame drawn yet");
    return count == 0u ? 1 : RT_OK;
}

// the validated domain of a record, in the kernel's fp32 comparisons (a NaN fails every one)
bool draw_box_valid(const RtDrawBox& b) {
    for (int k = 0; k < 3; k++)
        if (!(fabsf(b.lo[k]) <= 4194304.0f && fabsf(b.hi[k]) <= 4194304.0f && b.lo[k] < b.hi[k])) return false;
    return true;
}

// The launch on the stream the frame drawn last ended on, behind the queries enqueued so far (their results may be its face lights).
int draw_boxes_launch(RtContext* c, const RtUniforms* u, const void* boxes_dev, const void* lights_dev, uint32_t count) {
    // the slot's prepass no longer describes its planes: a still camera must not carry entity pixels into the next frame
    for (int b : {RT_BUF_DEPTH_F32, RT_BUF_DEPTH_R16UI, RT_BUF_NORMAL_R8UI, RT_BUF_ALBEDO_RGBA8, RT_BUF_EMISSION_RGBA8, RT_BUF_LIGHTING_F32,
                  RT_BUF_LIGHTING_RGBA16})
        plane_written(c, c->planes[b]);
    RT_HIP(c, c->ev_query.wait_elsewhere(c->stream));
    rtd::DrawBoxesArgs a;
    a.boxes = reinterpret_cast<const uint4*>(boxes_dev);
    a.lights = reinterpret_cast<const float4*>(lights_dev);
    a.count = count;
    a.width = c->cfg.width; a.height = c->cfg.height;
    for (int k = 0; k < 3; k++) { a.origin[k] = u->origin[k]; a.forward[k] = u->forward[k]; a.up[k] = u->up[k]; a.right[k] = u->right[k]; }
    LaunchTimer t(c, 1);
    RT_HIP(c, rtd::launch_draw_boxes(planes_of(c), a, c->stream));
    return RT_OK;
}
}  // namespace

extern "C" {

int rt_draw_boxes(RtContext* ctx, const RtUniforms* u, const RtDrawBox* boxes, const RtProbeLight* face_lights, uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = draw_boxes_check(ctx, "rt_draw_boxes", u, boxes, face_lights, count);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    for (uint32_t i = 0; i < count; i++)
        if (!draw_box_valid(boxes[i])) return fail(ctx, RT_ERR_INVALID_ARG, "rt_draw_boxes: box " + std::to_string(i) + " is not a valid box");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    // the boxes and lights through pinned and device staging, then the launch (the previous synchronous call has finished with the
    // staging: it waited for its launch)
    const size_t box_bytes = (size_t)count * sizeof(RtDrawBox), light_bytes = (size_t)count * 6u * sizeof(RtProbeLight), need = box_bytes + light_bytes;
    StagingBlock& q = ctx->query_block;
    RT_HIP(ctx, q.grow(ctx, need, need < ((size_t)64 << 10) ? ((size_t)64 << 10) : need + need / 2u));
    memcpy(q.host, boxes, box_bytes);
    memcpy(q.host + box_bytes, face_lights, light_bytes);
    RT_HIP(ctx, hipMemcpyAsync(q.dev, q.host, need, hipMemcpyHostToDevice, ctx->stream));
    rc = draw_boxes_launch(ctx, u, q.dev, q.dev + box_bytes, count);
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_draw_boxes_async(RtContext* ctx, const RtUniforms* u, const RtDrawBox* boxes_dev, const RtProbeLight* face_lights_dev, uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const int rc = draw_boxes_check(ctx, "rt_draw_boxes_async", u, boxes_dev, face_lights_dev, count);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!query_device_ptr(ctx, boxes_dev) || !query_device_ptr(ctx, face_lights_dev))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_draw_boxes_async: boxes and face_lights must be 16-byte aligned memory of the context's device");
    return draw_boxes_launch(ctx, u, boxes_dev, face_lights_dev, count);
}

}  // extern "C"
