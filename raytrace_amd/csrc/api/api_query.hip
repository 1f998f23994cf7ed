// api_query.hip — ray queries against the resident world: rt_trace_rays, rt_trace_rays_async, rt_pick_pixels.
#include "rt_context.hpp"

using namespace rta;

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
    // (the previous synchronous call has finished with the staging: it waited for its hits)
    StagingBlock& q = c->query_block;
    RT_HIP(c, q.grow(c, need, need < ((size_t)64 << 10) ? ((size_t)64 << 10) : align16(need + need / 2u)));
    memcpy(q.host, in, in_bytes);
    RT_HIP(c, hipMemcpyAsync(q.dev, q.host, in_bytes, hipMemcpyHostToDevice, st));
    rc = query_launch(c, st, f, picks ? nullptr : q.dev, picks ? q.dev : nullptr, q.dev + off, count);
    if (rc != RT_OK) return rc;
    RT_HIP(c, hipMemcpyAsync(q.host + off, q.dev + off, (size_t)count * sizeof(RtRayHit), hipMemcpyDeviceToHost, st));
    RT_HIP(c, hipStreamSynchronize(st));
    memcpy(hits, q.host + off, (size_t)count * sizeof(RtRayHit));
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
    for (uint32_t i = 0; i < count; i++)
        if (xy[2 * i] < 0 || xy[2 * i] >= ctx->cfg.width || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= ctx->cfg.height)
            return fail(ctx, RT_ERR_INVALID_ARG, "rt_pick_pixels: pixel " + std::to_string(i) + " is outside the frame");
    return query_sync(ctx, frame_of(ctx, u), xy, (size_t)count * 8u, true, hits, count);
}

}  // extern "C"
