// bench_run.hpp — what rt_bench's modes run on: the options, one session (a pipeline with one drawn frame), the timed pass and the
// event-bracketed repeat of an asynchronous call.
#pragma once

#include <dlfcn.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bench_scene.hpp"
#include "render.hpp"

namespace bench {

// the command line (rt_bench.cpp parses and validates it); -1: the flag was not given
struct Options {
    int width = 1024, height = 1024;   // WINDOW_WIDTH / WINDOW_HEIGHT, src/render/constants.rs:9-10
    int spp = 1, depth = 2, frames = 240, device = 0, gpus = 1;
    bool gather = false, overlap = false, post = false, accumulate = false, edit_spread = false;
    int edits = 0, edit_radius = 0;
    const char* edit_shape = nullptr;
    int edit_stamp = -1;
    long long entity_rays = 0, entity_sweeps = 0;
    bool coherent = false;
    long long rays = 0, boxes = -1, lights = -1, models = -1, shadows = -1, particles = -1;
    float particle_half = 0.0625f, particle_near = 10.0f;
    int simulate = 0, step_sweeps = 3;
    int debris = 0, debris_density = 256;   // --debris RADIUS [--density D]
    int settle = 0;                         // --debris RADIUS --settle T
    long long fall = 0;                     // --debris RADIUS --settle T --fall K (0xFFFFFFFF: until at rest)
    int collapse = 0;                       // --collapse RADIUS
    int navigate = 0;                       // --navigate EXTENT
    long long agents = 0;                   // --navigate EXTENT --agents N
    int flood = 0, flood_ticks = 0;         // --flood EXTENT [--ticks K] (0: eight ticks a call)
    bool shadow_models = false, light_shadows = false, occluders_far = false;
    float model_scale = 0.125f, occluder_spread = 3.0f;
    bool rays_coherent = false;
    bool reproject = false, stream = false, stream_history = false, history_denoise = false;
    float camera_step = 0.0f;
    int frames_in_flight = 1;      // 2: RT_FLAG_FRAMES_IN_FLIGHT_2 and no fence between frames (bench.py's default), one device
    std::string noise_path = "tests/golden/blue_noise_512.rgba";
};

// what every mode is handed besides the options: the generated world and the blue-noise table
struct World {
    rt::game::Game& game;
    const std::vector<uint8_t>& noise;
};

// the modes that run instead of the frame loop (bench_modes.cpp); each prints one JSON line and returns the exit code
int run_rays(const Options& o, const World& w);
int run_entity_rays(const Options& o, const World& w);
int run_entity_sweeps(const Options& o, const World& w);
int run_boxes(const Options& o, const World& w);
int run_particles(const Options& o, const World& w);
int run_simulate(const Options& o, const World& w);
int run_debris(const Options& o, const World& w);
int run_settle(const Options& o, const World& w);
int run_fall(const Options& o, const World& w);
int run_collapse(const Options& o, const World& w);
int run_navigate(const Options& o, const World& w);
int run_flood(const Options& o, const World& w);
int run_models(const Options& o, const World& w);
int run_lights(const Options& o, const World& w);
int run_shadows(const Options& o, const World& w);
int run_light_shadows(const Options& o, const World& w);

inline double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

inline RtConfig make_config(const Options& o, int rank, int world, uint32_t flags) {
    RtConfig cfg{};
    cfg.struct_size = sizeof(cfg);
    cfg.width = o.width; cfg.height = o.height; cfg.region = RT_ROOT_BLOCK_SIZE; cfg.spp = o.spp; cfg.depth = o.depth;
    cfg.device = o.device + rank; cfg.tile_rank = rank; cfg.tile_world = world; cfg.kernel = RT_KERNEL_DEFAULT;
    cfg.flags = flags;
    return cfg;
}

// One mode's pipeline with one frame drawn: its context, that frame's view and the scene's generator.
struct Session {
    rt::render::Pipeline* p = nullptr;
    RtContext* ctx = nullptr;
    View view;
    Rng rnd;
    Session() = default;
    Session(const Session&) = delete;
    Session& operator=(const Session&) = delete;
    ~Session() { delete p; }
    const RtUniforms& u() const { return view.u; }
    // the library's call failed: the mode's message, exit code 1
    int fail(const char* what, int rc) const { std::fprintf(stderr, "%s failed (%d): %s\n", what, rc, rt_last_error(ctx)); return 1; }
    bool create_stamp(SparseStamp* s) const {
        if (p->stamp_create(s->ext, s->mats.data(), s->state.data(), &s->id) == RT_OK) return true;
        std::fprintf(stderr, "stamp_create failed: %s\n", p->last_error());
        return false;
    }
    int read_plane(uint32_t buffer, std::vector<float>* plane) const { return rt_readback(ctx, buffer, plane->data(), plane->size() * sizeof(float)); }
};
// `flags` besides RT_FLAG_CACHE_PRIMARY; false (after the message) when the pipeline or its first frame failed
inline bool open_session(Session* s, const Options& o, const World& w, uint32_t flags) {
    std::string err;
    s->p = rt::render::create_instance(make_config(o, 0, 1, RT_FLAG_CACHE_PRIMARY | flags), w.noise.data(), w.game, &err);
    if (!s->p) { std::fprintf(stderr, "create_instance failed: %s\n", err.c_str()); return false; }
    s->ctx = s->p->context();
    // the camera's uniforms, from one drawn frame
    if (s->p->draw_frame(w.game) != RT_OK || s->p->wait() != RT_OK) { std::fprintf(stderr, "frame failed: %s\n", s->p->last_error()); return false; }
    s->view.u = s->p->uniforms();
    s->view.width = o.width; s->view.height = o.height;
    return true;
}

// The timed pass: PASS_REPS + 1 times (the first warms the staging up and is discarded) a frame, a sync and a read of the timing that
// drains the frame's own launches; then `call` between two clock reads and the timing read that holds its launches alone.  `before_last`
// runs in the last repetition between the drain and the call (a readback of the planes the call is about to change).  Nothing runs
// when rc is not RT_OK on entry; returns the first failure.
constexpr int PASS_REPS = 20;
struct PassTime {
    double device_ms = 0.0, call_ms = 0.0;   // per call: the launches bracketed by events (RT_FLAG_TIMING_ALL), call to return
    uint32_t launches = 0;                   // of all PASS_REPS calls
};
template <class Call, class Hook>
int timed_pass(const Session& s, int rc, PassTime* out, Call call, Hook before_last) {
    for (int i = 0; i < PASS_REPS + 1 && rc == RT_OK; i++) {
        RtTiming tm{};
        rc = rt_draw_frame(s.ctx, &s.u());
        if (rc == RT_OK) rc = rt_sync(s.ctx);
        if (rc == RT_OK) rc = rt_get_timing(s.ctx, &tm);
        if (rc == RT_OK && i == PASS_REPS) rc = before_last();
        const auto t = std::chrono::steady_clock::now();
        if (rc == RT_OK) rc = call();
        const double ms = ms_since(t);
        if (rc == RT_OK) rc = rt_get_timing(s.ctx, &tm);
        if (i > 0) { out->device_ms += tm.shade_ms / PASS_REPS; out->call_ms += ms / PASS_REPS; out->launches += tm.other_launches; }
    }
    return rc;
}
template <class Call>
int timed_pass(const Session& s, int rc, PassTime* out, Call call) { return timed_pass(s, rc, out, call, [] { return (int)RT_OK; }); }

// pixels whose `floats` floats (1: a depth, 4: a lighting value) differ in any bit between two planes
inline uint64_t changed_pixels(const std::vector<float>& a, const std::vector<float>& b, size_t floats) {
    uint64_t n = 0;
    for (size_t i = 0; i + floats <= a.size(); i += floats) n += std::memcmp(&a[i], &b[i], floats * sizeof(float)) != 0;
    return n;
}

// The few HIP runtime calls --entity-rays, --entity-sweeps and --simulate need to time asynchronous calls with an event pair, taken from the runtime the
// library itself runs on (this program is plain C++ and includes no HIP header).  ok == false: no device times.
struct HipEvents {
    typedef int (*malloc_t)(void**, size_t);
    typedef int (*free_t)(void*);
    typedef int (*memcpy_t)(void*, const void*, size_t, int);
    typedef int (*make_t)(void**);
    typedef int (*one_t)(void*);
    typedef int (*record_t)(void*, void*);
    typedef int (*elapsed_t)(float*, void*, void*);
    malloc_t dev_malloc = nullptr; free_t dev_free = nullptr; memcpy_t copy = nullptr;
    make_t stream_create = nullptr, event_create = nullptr;
    one_t stream_destroy = nullptr, event_destroy = nullptr, event_sync = nullptr;
    record_t event_record = nullptr;
    elapsed_t elapsed = nullptr;
    bool ok = false;
    HipEvents() {
        void* h = dlopen("libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return;
        dev_malloc = (malloc_t)dlsym(h, "hipMalloc"); dev_free = (free_t)dlsym(h, "hipFree"); copy = (memcpy_t)dlsym(h, "hipMemcpy");
        stream_create = (make_t)dlsym(h, "hipStreamCreate"); stream_destroy = (one_t)dlsym(h, "hipStreamDestroy");
        event_create = (make_t)dlsym(h, "hipEventCreate"); event_destroy = (one_t)dlsym(h, "hipEventDestroy");
        event_sync = (one_t)dlsym(h, "hipEventSynchronize"); event_record = (record_t)dlsym(h, "hipEventRecord");
        elapsed = (elapsed_t)dlsym(h, "hipEventElapsedTime");
        ok = dev_malloc && dev_free && copy && stream_create && stream_destroy && event_create && event_destroy && event_sync && event_record && elapsed;
    }
};

// One run on the device: buffers, then a stream of this program's that the context works on, and two events.  `fine` turns false at
// the first failure and every later step is skipped; close() (the destructor at the latest) hands the context its own stream back
// and frees everything.
struct DeviceRun {
    const HipEvents& hip;
    RtContext* ctx;
    void *st = nullptr, *e0 = nullptr, *e1 = nullptr;
    std::vector<void*> buffers;
    bool fine = true, open = true;
    DeviceRun(const HipEvents& hip_, RtContext* ctx_) : hip(hip_), ctx(ctx_) {}
    DeviceRun(const DeviceRun&) = delete;
    DeviceRun& operator=(const DeviceRun&) = delete;
    ~DeviceRun() { close(); }
    // `bytes` of device memory holding a copy of `host` (nullptr: uninitialised)
    void* on_device(const void* host, size_t bytes) {
        void* d = nullptr;
        if (hip.dev_malloc(&d, bytes ? bytes : 16) != 0) { fine = false; return nullptr; }
        buffers.push_back(d);
        if (host && bytes && hip.copy(d, host, bytes, 1 /* hipMemcpyHostToDevice */) != 0) fine = false;
        return d;
    }
    void start() { fine = fine && hip.stream_create(&st) == 0 && hip.event_create(&e0) == 0 && hip.event_create(&e1) == 0 && rt_set_stream(ctx, st) == RT_OK; }
    bool mark() { return hip.event_record(e0, st) == 0; }
    // ms since mark(), once the stream has got there
    bool lap(float* ms) { return hip.event_record(e1, st) == 0 && hip.event_sync(e1) == 0 && hip.elapsed(ms, e0, e1) == 0; }
    // `call` reps + 1 times (the first warms up; the events bracket the others): device ms per call, -1 when something failed
    template <class Call>
    double repeat(int reps, Call call) {
        for (int i = 0; i < reps + 1 && fine; i++) {
            if (i == 1) fine = mark();
            if (fine) fine = call() == RT_OK;
        }
        float ms = 0.0f;
        fine = fine && lap(&ms);
        return fine ? (double)ms / reps : -1.0;
    }
    bool close() {
        if (!open) return fine;
        open = false;
        if (rt_sync(ctx) != RT_OK || rt_set_stream(ctx, nullptr) != RT_OK) fine = false;
        if (e0) (void)hip.event_destroy(e0);
        if (e1) (void)hip.event_destroy(e1);
        if (st) (void)hip.stream_destroy(st);
        for (void* d : buffers) (void)hip.dev_free(d);
        return fine;
    }
};

}  // namespace bench
