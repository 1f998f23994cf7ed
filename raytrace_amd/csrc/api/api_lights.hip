// api_lights.hip — point lights (rt_add_lights, rt_add_lights_async): one launch on the stream of the frame drawn last, behind that
// frame (and its entity boxes) and in front of or behind its post passes.
#include "lights_check.hpp"
#include "rt_context.hpp"

using namespace rta;

namespace {
static_assert(sizeof(RtPointLight) == 32, "the kernel reads two 16-byte words per light");

// checks shared by the two calls; RT_OK when there is work to enqueue, 1 for count == 0
int add_lights_check(RtContext* c, const char* fn, const RtUniforms* u, const void* lights, uint32_t count) {
    const std::string w(fn);
    if (!u) return fail(c, RT_ERR_INVALID_ARG, w + ": null uniforms");
    if (count > kMaxPointLights) return fail(c, RT_ERR_INVALID_ARG, w + ": more than 1024 lights in one call");
    if (count > 0u && !lights) return fail(c, RT_ERR_INVALID_ARG, w + ": null pointer");
    if (c->cfg.tile_world != 1) return fail(c, RT_ERR_UNIMPLEMENTED, w + ": whole-frame contexts only");
    if (!c->frame_recorded) return fail(c, RT_ERR_NOT_READY, w + ": no frame drawn yet");
    if (!c->world_resident) return fail(c, RT_ERR_NOT_READY, w + ": upload the full region first");
    return count == 0u ? 1 : RT_OK;
}

// The launch on the stream the frame drawn last ended on.  It reads the region there: every world change runs on that stream too, the
// earlier ones in front of it, and a later one — whichever lane's stream it finds as the context's by then — first joins every lane
// (world_change_begin), this one among them.  Queries enqueued so far may have produced the records (a device buffer of the caller's).
int add_lights_launch(RtContext* c, const RtUniforms* u, const void* lights_dev, uint32_t count) {
    // the slot's prepass no longer describes its planes: a still camera must not carry the light into the next frame
    for (int b : {RT_BUF_LIGHTING_F32, RT_BUF_LIGHTING_RGBA16}) plane_written(c, c->planes[b]);
    RT_HIP(c, c->ev_query.wait_elsewhere(c->stream));
    rtd::LightsArgs a;
    a.lights = reinterpret_cast<const uint4*>(lights_dev);
    a.count = count;
    LaunchTimer t(c, 1);
    RT_HIP(c, rtd::launch_add_lights(scene_of(c), frame_of(c, u), planes_of(c), a, c->stream));
    return RT_OK;
}
}  // namespace

extern "C" {

int rt_add_lights(RtContext* ctx, const RtUniforms* u, const RtPointLight* lights, uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = add_lights_check(ctx, "rt_add_lights", u, lights, count);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    const uint32_t bad = first_invalid_point_light(lights, count);
    if (bad != count) return fail(ctx, RT_ERR_INVALID_ARG, "rt_add_lights: light " + std::to_string(bad) + " is not a valid light");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    // the records through pinned and device staging, then the launch (the previous synchronous call has finished with the staging:
    // it waited for its launch)
    const size_t need = (size_t)count * sizeof(RtPointLight);
    StagingBlock& q = ctx->query_block;
    RT_HIP(ctx, q.grow(ctx, need, need < ((size_t)64 << 10) ? ((size_t)64 << 10) : need + need / 2u));
    memcpy(q.host, lights, need);
    RT_HIP(ctx, hipMemcpyAsync(q.dev, q.host, need, hipMemcpyHostToDevice, ctx->stream));
    rc = add_lights_launch(ctx, u, q.dev, count);
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_add_lights_async(RtContext* ctx, const RtUniforms* u, const RtPointLight* lights_dev, uint32_t count) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const int rc = add_lights_check(ctx, "rt_add_lights_async", u, lights_dev, count);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!query_device_ptr(ctx, lights_dev))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_add_lights_async: lights must be 16-byte aligned memory of the context's device");
    return add_lights_launch(ctx, u, lights_dev, count);
}

}  // extern "C"
