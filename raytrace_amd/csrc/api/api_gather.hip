// api_gather.hip — multi-GPU: RCCL gather of the tile-split G-buffer: the library loader, the rt_comm_* calls,
// rt_gather_gbuffer and its timing.
#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: the library is dlopen'ed on first use (rt_comm_* / rt_gather_gbuffer)

#include <mutex>

#include "rt_context.hpp"

using namespace rta;

namespace {
// the functions taken from librccl: g_rccl.Send is ncclSend
#define RT_RCCL_FUNCS(X) X(GetUniqueId) X(CommInitRank) X(CommInitAll) X(CommDestroy) X(GroupStart) X(GroupEnd) X(Send) X(Recv) X(GetErrorString)
struct Rccl {
    void* handle = nullptr;
#define RT_RCCL_MEMBER(name) decltype(&nccl##name) name = nullptr;
    RT_RCCL_FUNCS(RT_RCCL_MEMBER)
#undef RT_RCCL_MEMBER
    std::string error;
};
Rccl g_rccl;
std::once_flag g_rccl_once;

// librccl is 0.5 GB: loaded on first use only.  A copy the process already holds (e.g. the one PyTorch ships) is reused,
// so a communicator created by the host's own RCCL stays valid here.
bool rccl_load() {
    std::call_once(g_rccl_once, [] {
        const char* names[] = {"librccl.so.1", "librccl.so"};
        for (const char* n : names) { if (!g_rccl.handle) g_rccl.handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD); }
        for (const char* n : names) { if (!g_rccl.handle) g_rccl.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL); }
        if (!g_rccl.handle) { g_rccl.error = std::string("cannot load librccl: ") + dlerror(); return; }
#define RT_RCCL_SYM(name) g_rccl.name = (decltype(g_rccl.name))dlsym(g_rccl.handle, "nccl" #name); if (!g_rccl.name) g_rccl.error = "librccl lacks nccl" #name;
        RT_RCCL_FUNCS(RT_RCCL_SYM)
#undef RT_RCCL_SYM
    });
    return g_rccl.error.empty();
}
#define RT_NCCL(ctx, call)                                                                                   \
    do { ncclResult_t r_ = (call); if (r_ != ncclSuccess)                                                    \
        return fail(ctx, RT_ERR_HIP, std::string(#call) + ": " + g_rccl.GetErrorString(r_)); } while (0)
}  // namespace

extern "C" {

int rt_comm_unique_id(void* id_out, size_t bytes) {
    if (!id_out || bytes != NCCL_UNIQUE_ID_BYTES) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_comm_unique_id: need a 128-byte buffer");
    if (!rccl_load()) return fail(nullptr, RT_ERR_UNIMPLEMENTED, g_rccl.error);
    ncclUniqueId id;
    RT_NCCL(nullptr, g_rccl.GetUniqueId(&id));
    memcpy(id_out, &id, sizeof(id));
    return RT_OK;
}

int rt_comm_init_rank(RtContext* ctx, const void* id, size_t bytes, void** comm_out) {
    if (comm_out) *comm_out = nullptr;
    if (!ctx || !id || bytes != NCCL_UNIQUE_ID_BYTES || !comm_out) return fail(ctx, RT_ERR_INVALID_ARG, "rt_comm_init_rank: bad argument");
    if (!rccl_load()) return fail(ctx, RT_ERR_UNIMPLEMENTED, g_rccl.error);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    ncclComm_t comm = nullptr;
    RT_NCCL(ctx, g_rccl.CommInitRank(&comm, ctx->cfg.tile_world, uid, ctx->cfg.tile_rank));
    *comm_out = comm;
    return RT_OK;
}

int rt_comm_init_all(int ndev, const int* devices, void** comms_out) {
    if (ndev < 1 || !comms_out) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_comm_init_all: bad argument");
    if (!rccl_load()) return fail(nullptr, RT_ERR_UNIMPLEMENTED, g_rccl.error);
    std::vector<ncclComm_t> comms((size_t)ndev, nullptr);
    RT_NCCL(nullptr, g_rccl.CommInitAll(comms.data(), ndev, devices));
    for (int i = 0; i < ndev; i++) comms_out[i] = comms[(size_t)i];
    return RT_OK;
}

int rt_comm_destroy(void* comm) {
    if (!comm) return RT_OK;
    if (!rccl_load()) return fail(nullptr, RT_ERR_UNIMPLEMENTED, g_rccl.error);
    RT_NCCL(nullptr, g_rccl.CommDestroy((ncclComm_t)comm));
    return RT_OK;
}

int rt_gather_gbuffer(RtContext* ctx, void* comm_, int root, void* const* frames_dev, int overlapped) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const int world = ctx->cfg.tile_world, rank = ctx->cfg.tile_rank;
    if (root < 0 || root >= world) return fail(ctx, RT_ERR_INVALID_ARG, "rt_gather_gbuffer: root out of range");
    if (!ctx->frame_recorded) return fail(ctx, RT_ERR_NOT_READY, "rt_gather_gbuffer: no frame drawn yet");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (rank == root && !frames_dev) {
        // no caller-owned planes: assemble into the library's own (allocated once; rt_frame_ptr / rt_frame_readback)
        for (int b = 0; b <= RT_BUF_FOG_RGBA8; b++)
            if (!ctx->frame_planes[b]) {
                uint8_t* p = nullptr;
                RT_HIP(ctx, dev_alloc(ctx, &p, (size_t)ctx->cfg.width * ctx->cfg.height * kBytesPerPixel[b]));
                ctx->frame_planes[b] = p;
            }
        frames_dev = ctx->frame_planes;
    }
    if (world == 1 && !comm_) {
        // one context holds the whole frame, row-major already: plain copies on the stream the frame ended on, after the previous
        // frame's copies (which sit on the other lane's stream when two frames are in flight)
        RT_HIP(ctx, ctx->ev_gather.wait(ctx->stream));
        for (int b = 0; b <= RT_BUF_FOG_RGBA8; b++)
            if (frames_dev[b]) RT_HIP(ctx, hipMemcpyAsync(frames_dev[b], ctx->planes[b], ctx->plane_pixels * kBytesPerPixel[b], hipMemcpyDeviceToDevice, ctx->stream));
        RT_HIP(ctx, ctx->ev_gather.record(ctx->stream));
        return RT_OK;
    }
    if (!comm_) return fail(ctx, RT_ERR_INVALID_ARG, "rt_gather_gbuffer: null communicator");
    if (!rccl_load()) return fail(ctx, RT_ERR_UNIMPLEMENTED, g_rccl.error);
    ncclComm_t comm = (ncclComm_t)comm_;
    const size_t gb = ctx->gbuffer_bytes;
    const int s = overlapped ? (int)(ctx->gathers & 1u) : 0;
    if (rank == root && !ctx->gathered[s]) RT_HIP(ctx, dev_alloc(ctx, &ctx->gathered[s], gb * (size_t)world));
    hipStream_t gs = ctx->stream;
    const uint8_t* src = (const uint8_t*)ctx->gbuffer;
    // gathers share the root's staging and the communicator: with two frames in flight the previous frame's gather sits on the
    // other lane's stream — this one follows it (the frames' rendering still overlaps)
    if (!overlapped) RT_HIP(ctx, ctx->ev_gather.wait(ctx->stream));
    if (overlapped) {
        // The frame's block is copied to one of two staging buffers on the render stream (so the next frame may overwrite the
        // planes), everything else runs on a second stream: frame k's send/recv + un-tile overlap frame k+1's kernels.
        if (!ctx->gather_stream) RT_HIP(ctx, new_stream(ctx, &ctx->gather_stream));
        for (int i = 0; i < 2; i++) {
            if (!ctx->ev_ready[i]) RT_HIP(ctx, new_event(ctx, &ctx->ev_ready[i]));
            if (!ctx->ev_free[i].ev) RT_HIP(ctx, new_event(ctx, &ctx->ev_free[i].ev));
        }
        if (!ctx->stage[s]) RT_HIP(ctx, dev_alloc(ctx, &ctx->stage[s], gb));
        RT_HIP(ctx, ctx->ev_free[s].wait(ctx->stream));   // gather k-2 has left stage[s]
        RT_HIP(ctx, hipMemcpyAsync(ctx->stage[s], ctx->gbuffer, gb, hipMemcpyDeviceToDevice, ctx->stream));
        RT_HIP(ctx, hipEventRecord(ctx->ev_ready[s], ctx->stream));
        RT_HIP(ctx, hipStreamWaitEvent(ctx->gather_stream, ctx->ev_ready[s], 0));
        gs = ctx->gather_stream;
        src = ctx->stage[s];
    }
    // RT_FLAG_TIMING: events round the transfer + un-tile on the stream they run on (rt_get_gather_timing)
    size_t gev = TimingPool::npos;
    if ((ctx->cfg.flags & RT_FLAG_TIMING) != 0) {
        hipError_t e;
        gev = ctx->gather_times.acquire(gs, &e);
        RT_HIP(ctx, e);
    }
    // every rank sends its block to the root; the root posts one receive per rank (its own block included).  Each peer uses
    // its own xGMI link into the root, so the transfers run in parallel.
    RT_NCCL(ctx, g_rccl.GroupStart());
    {   // a failing call must not leave the group open: the group is always closed, the first error is reported
        ncclResult_t first = ncclSuccess;
        const char* what = "";
        if (rank == root)
            for (int r = 0; r < world && first == ncclSuccess; r++) {
                first = g_rccl.Recv(ctx->gathered[s] + (size_t)r * gb, gb, ncclUint8, r, comm, gs);
                what = "ncclRecv";
            }
        if (first == ncclSuccess) { first = g_rccl.Send(src, gb, ncclUint8, root, comm, gs); what = "ncclSend"; }
        const ncclResult_t end = g_rccl.GroupEnd();
        if (first == ncclSuccess && end != ncclSuccess) { first = end; what = "ncclGroupEnd"; }
        if (first != ncclSuccess) return fail(ctx, RT_ERR_HIP, std::string("rt_gather_gbuffer: ") + what + ": " + g_rccl.GetErrorString(first));
    }
    if (rank == root) {
        const int capacity = (ctx->ntiles_total + world - 1) / world;
        for (int b = 0; b <= RT_BUF_FOG_RGBA8; b++) {
            if (!frames_dev[b]) continue;
            if (world == 1) {   // a one-rank communicator (the transfer went to itself): the block holds row-major planes
                RT_HIP(ctx, hipMemcpyAsync(frames_dev[b], ctx->gathered[s] + ctx->gbuffer_offset[b], ctx->plane_pixels * kBytesPerPixel[b],
                                           hipMemcpyDeviceToDevice, gs));
                continue;
            }
            RT_HIP(ctx, rtd::launch_untile_strided(ctx->gathered[s] + ctx->gbuffer_offset[b], gb, frames_dev[b], world, capacity, ctx->tiles_x,
                                                   ctx->tiles_y, ctx->cfg.width, ctx->cfg.height, (int)kBytesPerPixel[b], gs));
        }
    }
    if (gev != TimingPool::npos) RT_HIP(ctx, ctx->gather_times.release(gev, gs));
    RT_HIP(ctx, (overlapped ? ctx->ev_free[s] : ctx->ev_gather).record(gs));
    ctx->gathers++;
    return RT_OK;
}

int rt_get_gather_timing(RtContext* ctx, float* ms_sum, uint32_t* calls) {
    if (!ctx || !ms_sum || !calls) return RT_ERR_INVALID_ARG;
    *ms_sum = 0.0f; *calls = 0;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, sync_lanes(ctx));
    if (ctx->gather_stream) RT_HIP(ctx, hipStreamSynchronize(ctx->gather_stream));
    RT_HIP(ctx, ctx->gather_times.drain([&](size_t, float ms) { *ms_sum += ms; (*calls)++; }));
    return RT_OK;
}

}  // extern "C"
