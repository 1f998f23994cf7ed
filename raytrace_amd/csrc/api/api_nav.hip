// api_nav.hip — navigation fields (rt_nav_*): the store's device side (create, info, read, destroy), the builds and the samples.
// A build is a query ordered like rt_stamp_capture: its launches go to the stream the edits use, behind every earlier world change,
// read the region only and write the field's own block; the lanes are fenced behind them, because the next build or sample may find
// the other lane's stream as the context's.  A sample runs on the same stream and is ordered the same way, so it follows the builds
// enqueued before it; it does not read the world.  The verdicts and the plan are nav_check.hpp's.
#include "nav_check.hpp"
#include "rt_context.hpp"

using namespace rta;

namespace {

static_assert(sizeof(RtNavBuild) == 32 && sizeof(RtNavGoal) == 16 && sizeof(RtNavResult) == 32 && sizeof(RtNavAgent) == 16 && sizeof(RtNavStep) == 32,
              "the layout the header states");
static_assert(kNavHeadWords == rtd::kNavHeadWords && kNavTruncWord == rtd::kNavTruncWord && kNavSpareResult == rtd::kNavSpareResult &&
                  kMaxNavDist == rtd::kNavMaxDist && kMaxNavGoals == rtd::kNavMaxGoals && kMaxNavAgents == rtd::kNavMaxAgents,
              "the host's limits and layout are the kernels'");

uint32_t* nav_scratch(const NavEntry* e) { return reinterpret_cast<uint32_t*>(e->block); }
uint16_t* nav_dist(const NavEntry* e) { return reinterpret_cast<uint16_t*>(e->block + nav_plan(e->ext, 0u, kNavLevels).scratch_words * 4u); }
uint8_t* nav_move(const NavEntry* e) { return reinterpret_cast<uint8_t*>(nav_dist(e) + e->cells()); }

void nav_free(RtContext* c, NavEntry* e) {
    c->device_bytes -= nav_plan(e->ext, 0u, kNavLevels).block_bytes;
    (void)hipFree(reinterpret_cast<void*>(e->block));
    c->navs.remove(e);
}

// checks shared by the two builds: the arguments, the id, the box, the world
int nav_build_check(RtContext* c, const char* fn, uint32_t id, const RtNavBuild* p, const RtNavGoal* goals, uint32_t count, NavEntry** e) {
    const char* err = nav_build_error(p, goals, count);
    if (err) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": " + err + "; nothing was enqueued");
    *e = c->navs.find(id);
    if (!*e) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": unknown field id");
    if (!nav_box_inside(p->lo, (*e)->ext, c->logr)) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": box outside the region");
    if (!c->world_resident) return fail(c, RT_ERR_NOT_READY, std::string(fn) + ": upload the full region first");
    return RT_OK;
}

// The launches of one build on the render stream; goals_dev and result_dev are device addresses the stream may use (or null).
int nav_build_enqueue(RtContext* c, NavEntry* e, const RtNavBuild& p, const void* goals_dev, uint32_t count, void* result_dev) {
    rtd::NavArgs a;
    a.scratch = nav_scratch(e);
    a.dist = nav_dist(e);
    a.move = nav_move(e);
    a.result = result_dev ? reinterpret_cast<uint32_t*>(result_dev) : a.scratch + rtd::kNavSpareResult;
    a.goals = reinterpret_cast<const int4*>(goals_dev);
    for (int k = 0; k < 3; k++) { a.lo[k] = p.lo[k]; a.ext[k] = e->ext[k]; }
    a.max_dist = p.max_dist; a.goal_count = count;
    a.height = p.height; a.max_climb = p.max_climb; a.max_drop = p.max_drop; a.goal_snap = p.goal_snap;
    {
        LaunchTimer lt(c, 1);
        RT_HIP(c, rtd::launch_nav_build(c->d_mine_sw, c->logr, a, c->navs.levels, c->stream));
    }
    for (int k = 0; k < 3; k++) e->lo[k] = p.lo[k];
    e->built = true;
    e->used = true;
    RT_HIP(c, fence_lanes_after(c, c->stream));   // (the next build or sample may start on the other lane's stream)
    return RT_OK;
}

// checks shared by the two samples; RT_OK when there is work to enqueue, 1 for count == 0
int nav_sample_check(RtContext* c, const char* fn, uint32_t id, const void* agents, uint32_t count, const void* steps, NavEntry** e) {
    *e = c->navs.find(id);
    if (!*e) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": unknown field id");
    const char* err = nav_sample_error(agents, count, steps);
    if (err) return fail(c, RT_ERR_INVALID_ARG, std::string(fn) + ": " + err);
    if (!(*e)->built) return fail(c, RT_ERR_NOT_READY, std::string(fn) + ": the field was never built");
    return count == 0u ? 1 : RT_OK;
}

int nav_sample_enqueue(RtContext* c, NavEntry* e, const void* agents_dev, uint32_t count, void* steps_dev) {
    rtd::NavSampleArgs a;
    a.dist = nav_dist(e);
    a.move = nav_move(e);
    a.agents = reinterpret_cast<const uint4*>(agents_dev);
    a.steps = reinterpret_cast<uint4*>(steps_dev);
    a.count = count;
    for (int k = 0; k < 3; k++) { a.lo[k] = e->lo[k]; a.ext[k] = e->ext[k]; }
    {
        LaunchTimer lt(c, 1);
        RT_HIP(c, rtd::launch_nav_sample(a, c->stream));
    }
    e->used = true;
    RT_HIP(c, fence_lanes_after(c, c->stream));   // (a later build of the field may start on the other lane's stream)
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_nav_create(RtContext* ctx, const int32_t extent[3], uint32_t* id_out) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    if (!extent || !id_out) return fail(ctx, RT_ERR_INVALID_ARG, "rt_nav_create: null pointer");
    if (!nav_extent_valid(extent)) return fail(ctx, RT_ERR_INVALID_ARG, "rt_nav_create: an extent outside 1..256");
    if (ctx->navs.live == kMaxNavFields) return fail(ctx, RT_ERR_INVALID_ARG, "rt_nav_create: 64 fields are live");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->navs.live == 0u) env_int("RT_NAV_LEVELS", 1, 8, &ctx->navs.levels);   // A/B timing: 1, 4 or 8 levels per launch
    if (ctx->navs.levels != 1u && ctx->navs.levels != 4u) ctx->navs.levels = kNavLevels;
    const NavPlan plan = nav_plan(extent, 0u, kNavLevels);
    void* block = nullptr;
    const hipError_t err = hipMalloc(&block, plan.block_bytes);
    if (err != hipSuccess)
        return fail(ctx, err == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP, std::string("rt_nav_create: ") + hipGetErrorString(err));
    NavEntry* e = ctx->navs.add(extent);
    e->block = reinterpret_cast<uint64_t>(block);
    ctx->device_bytes += plan.block_bytes;
    *id_out = e->id;
    return RT_OK;
}

int rt_nav_info(RtContext* ctx, uint32_t id, int32_t extent_out[3], int32_t lo_out[3], uint32_t* built_out) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const NavEntry* e = ctx->navs.find(id);
    if (!e) return fail(ctx, RT_ERR_INVALID_ARG, "rt_nav_info: unknown field id");
    for (int k = 0; k < 3; k++) {
        if (extent_out) extent_out[k] = e->ext[k];
        if (lo_out) lo_out[k] = e->lo[k];
    }
    if (built_out) *built_out = e->built ? 1u : 0u;
    return RT_OK;
}

int rt_nav_read(RtContext* ctx, uint32_t id, uint16_t* dist, uint8_t* move) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    NavEntry* e = ctx->navs.find(id);
    if (!e) return fail(ctx, RT_ERR_INVALID_ARG, "rt_nav_read: unknown field id");
    if (!e->built) return fail(ctx, RT_ERR_NOT_READY, "rt_nav_read: the field was never built");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, sync_lanes(ctx));   // (a build may still be writing it)
    e->used = false;
    if (dist) RT_HIP(ctx, hipMemcpy(dist, nav_dist(e), e->cells() * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (move) RT_HIP(ctx, hipMemcpy(move, nav_move(e), e->cells(), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_nav_destroy(RtContext* ctx, uint32_t id) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    NavEntry* e = ctx->navs.find(id);
    if (!e) return fail(ctx, RT_ERR_INVALID_ARG, "rt_nav_destroy: unknown field id");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (e->used) RT_HIP(ctx, sync_lanes(ctx));   // the builds that wrote it and the samples that read it have finished
    nav_free(ctx, e);
    return RT_OK;
}

int rt_nav_build(RtContext* ctx, uint32_t id, const RtNavBuild* params, const RtNavGoal* goals, uint32_t goal_count, RtNavResult* result) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    NavEntry* e = nullptr;
    int rc = nav_build_check(ctx, "rt_nav_build", id, params, goals, goal_count, &e);
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    // the goals and the result through the synchronous calls' pinned and device block on the render stream, the launches there, and
    // the result back (a call without goals or without a result stages a spare record in their place)
    const RtNavGoal no_goal{};
    RtNavResult spare{};
    RtNavResult* res = result ? result : &spare;
    uint8_t* dev[2];
    rc = stage_sync(ctx, ctx->stream, {{goal_count ? goals : &no_goal, (size_t)(goal_count ? goal_count : 1u) * sizeof(RtNavGoal)}, {res, sizeof *res}}, dev);
    if (rc != RT_OK) return rc;
    rc = nav_build_enqueue(ctx, e, *params, dev[0], goal_count, dev[1]);
    if (rc != RT_OK) return rc;
    uint8_t* host = ctx->query_block.host + (dev[1] - ctx->query_block.dev);
    RT_HIP(ctx, hipMemcpyAsync(host, dev[1], sizeof *res, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(res, host, sizeof *res);
    return RT_OK;
}

int rt_nav_build_async(RtContext* ctx, uint32_t id, const RtNavBuild* params, const RtNavGoal* goals_dev, uint32_t goal_count,
                       RtNavResult* result_dev) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    NavEntry* e = nullptr;
    const int rc = nav_build_check(ctx, "rt_nav_build_async", id, params, goals_dev, goal_count, &e);
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if ((goal_count > 0u && !query_device_ptr(ctx, goals_dev)) || (result_dev && !query_device_ptr(ctx, result_dev)))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_nav_build_async: goals and result must be 16-byte aligned memory of the context's device");
    return nav_build_enqueue(ctx, e, *params, goals_dev, goal_count, result_dev);
}

int rt_nav_sample(RtContext* ctx, uint32_t id, const RtNavAgent* agents, uint32_t count, RtNavStep* steps) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    NavEntry* e = nullptr;
    int rc = nav_sample_check(ctx, "rt_nav_sample", id, agents, count, steps, &e);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    // the agents through pinned and device staging, the launch, the steps back
    const size_t out_bytes = (size_t)count * sizeof(RtNavStep);
    uint8_t* dev[2];
    rc = stage_sync(ctx, ctx->stream, {{agents, (size_t)count * sizeof(RtNavAgent)}, {nullptr, out_bytes}}, dev);
    if (rc != RT_OK) return rc;
    rc = nav_sample_enqueue(ctx, e, dev[0], count, dev[1]);
    if (rc != RT_OK) return rc;
    uint8_t* host = ctx->query_block.host + (dev[1] - ctx->query_block.dev);
    RT_HIP(ctx, hipMemcpyAsync(host, dev[1], out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(steps, host, out_bytes);
    return RT_OK;
}

int rt_nav_sample_async(RtContext* ctx, uint32_t id, const RtNavAgent* agents_dev, uint32_t count, RtNavStep* steps_dev) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    NavEntry* e = nullptr;
    const int rc = nav_sample_check(ctx, "rt_nav_sample_async", id, agents_dev, count, steps_dev, &e);
    if (rc != RT_OK) return rc == 1 ? RT_OK : rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!query_device_ptr(ctx, agents_dev) || !query_device_ptr(ctx, steps_dev))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_nav_sample_async: agents and steps must be 16-byte aligned memory of the context's device");
    return nav_sample_enqueue(ctx, e, agents_dev, count, steps_dev);
}

}  // extern "C"
