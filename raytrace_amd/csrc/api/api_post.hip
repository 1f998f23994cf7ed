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

namespace {

// RtDenoiseParams as the header states it; nothing is enqueued for a block that fails
int check_denoise_params(RtContext* ctx, const char* who, const RtDenoiseParams* p) {
    const std::string w(who);
    if (!p) return fail(ctx, RT_ERR_INVALID_ARG, w + ": null params");
    if (p->struct_size != sizeof(RtDenoiseParams)) return fail(ctx, RT_ERR_INVALID_ARG, w + ": RtDenoiseParams.struct_size mismatch");
    if (p->weight_by_count != 0 && p->weight_by_count != 1) return fail(ctx, RT_ERR_INVALID_ARG, w + ": weight_by_count must be 0 or 1");
    for (int i = 0; i < 6; i++)
        if (p->settle[i] > 127u) return fail(ctx, RT_ERR_INVALID_ARG, w + ": settle[i] must be 0 (nobody settles) or 1..127");
    for (int i = 0; i < 3; i++)
        if (p->reserved[i] != 0u) return fail(ctx, RT_ERR_INVALID_ARG, w + ": reserved words must be 0");
    return RT_OK;
}

// rt_denoise_planes' seven launches with the counts packed into the working pixel (`counts`: a u32 plane, or the history records)
int denoise_counted(RtContext* ctx, void* lighting, const void* depth, const void* normal, const void* counts, bool counts_are_records,
                    const RtDenoiseParams& p) {
    plane_written(ctx, lighting);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const int sizes[6] = {1, 2, 4, 8, 8, 16};                         // pipeline.rs:103
    const int W = ctx->cfg.width, H = ctx->cfg.height;
    void** work = ctx->slots[ctx->cur_slot].denoise_work;
    for (int i = 0; i < 2; i++)
        if (!work[i]) { uint4* q = nullptr; RT_HIP(ctx, dev_alloc(ctx, &q, (size_t)W * H)); work[i] = q; }
    {
        LaunchTimer t(ctx, 1);
        RT_HIP(ctx, rtd::launch_denoise_prepare_counted(lighting, depth, normal, counts, counts_are_records, W, H, work[0], ctx->stream));
    }
    for (int pass = 0; pass < 6; pass++) {
        const bool odd = pass % 2 == 1;
        LaunchTimer t(ctx, 1);
        RT_HIP(ctx, rtd::launch_denoise_counted(work[pass & 1], W, H, sizes[pass], odd && p.faithful != 0, pass == 5, p.weight_by_count == 1,
                                                p.settle[pass], work[(pass & 1) ^ 1], lighting, ctx->stream));
    }
    return RT_OK;
}

}  // namespace

int rt_denoise_planes_counted(RtContext* ctx, void* lighting, const void* depth, const void* normal, const uint32_t* counts_dev,
                              const RtDenoiseParams* params) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!lighting || !depth || !normal || !counts_dev) return fail(ctx, RT_ERR_INVALID_ARG, "rt_denoise_planes_counted: null plane");
    const int rc = check_denoise_params(ctx, "rt_denoise_planes_counted", params);
    if (rc != RT_OK) return rc;
    return denoise_counted(ctx, lighting, depth, normal, counts_dev, false, *params);
}

int rt_denoise_history(RtContext* ctx, const RtDenoiseParams* params) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (ctx->cfg.tile_world != 1) return fail(ctx, RT_ERR_UNIMPLEMENTED, "rt_denoise_history: whole-frame contexts only (gather the tiles, then rt_denoise_planes_counted)");
    if (!ctx->reproject) return fail(ctx, RT_ERR_INVALID_ARG, "rt_denoise_history: the context was created without RT_FLAG_REPROJECT");
    const int rc = check_denoise_params(ctx, "rt_denoise_history", params);
    if (rc != RT_OK) return rc;
    if (!ctx->frame_recorded) return fail(ctx, RT_ERR_NOT_READY, "rt_denoise_history: no frame drawn yet");
    // The records of the frame drawn last, read on the stream that frame ended on.  The set is next written by the pass of the
    // second frame from now, which is ordered behind this read: it uses this frame's slot (two slots) or follows the next frame,
    // which uses it (one slot), and a frame starts by waiting for everything put behind the previous user of its slot (ev_tail).
    return denoise_counted(ctx, ctx->planes[RT_BUF_LIGHTING_RGBA16], ctx->planes[RT_BUF_DEPTH_R16UI], ctx->planes[RT_BUF_NORMAL_R8UI],
                           ctx->d_hist_rec[ctx->hist_cur], true, *params);
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
