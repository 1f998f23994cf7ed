// api_post.hip — what follows a frame on its stream: un-tiling gathered planes, the denoise passes, finalize, and the library's own
// assembled frame (rt_frame_ptr, rt_frame_readback).
#include "rt_context.hpp"

using namespace rta;

extern "C" {

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

}  // extern "C"
