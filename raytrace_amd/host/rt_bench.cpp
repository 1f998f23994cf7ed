// rt_bench — headless counterpart of the reference's interactive binary (src/bin/main.rs:8-57): builds the Game
// (six optional positional floats `x y z heading pitch sun_angle`, src/game/mod.rs:45-52), creates the renderer, then
// loops draw_frame and prints the rolling average / maximum frame time of the last 120 frames
// (RingBufferAverage, src/util.rs:175-221; printout main.rs:42-47) — followed by ONE JSON line with the metrics SURVEY.md 5
// asks of the bench binary (config, rays, ms, Mrays/s).
//
//   rt_bench [x y z heading pitch sun] [--width W] [--height H] [--spp N] [--depth D] [--frames F]
//            [--noise tests/golden/blue_noise_512.rgba] [--device I] [--gpus N] [--gather] [--overlap] [--post] [--accumulate]
//            [--reproject [--history-denoise]] [--camera-step DX] [--frames-in-flight N] [--edits N [--edit-spread]] [--edit-radius N]
//            [--edit-shape sphere:R|box:E]
//            [--stream [--stream-history]]
//            [--rays N [--rays-coherent]]
//            [--boxes N]
//            [--particles N [--particle-half H] [--particle-near D] [--simulate T [--sweeps S]]]
//            [--entity-rays N [--coherent] [--boxes B] [--models M] [--model-scale S]]
//            [--lights N] [--shadows N [--shadow-models]]
//            [--light-shadows [--lights N] [--boxes B] [--models M] [--occluder-spread S] [--occluders-far]]
//
// --post: the reference's whole frame — ray trace, six denoise dispatches, finalize (pipeline.rs:86-123) — per draw_frame
// (Pipeline::enable_post_passes; one device only: the passes need the whole frame).
//
// --gpus N (one host thread per device, ncclCommInitAll through rt_comm_init_all): device i renders the tiles t % N == i and
// every frame ends with rt_gather_gbuffer to device 0, which assembles the full frame in the library's own planes.
// --gather runs that frame-end step with N = 1 too (a one-rank communicator).
//
// --accumulate: the contexts are created with RT_FLAG_ACCUMULATE.  The camera stays where it is and the mirror's draw_frame
// advances the seed by spp per frame, so every frame continues the accumulation; the JSON line adds the samples the last frame's
// lighting holds (rt_get_accumulation).
//
// --reproject (implies --accumulate): RT_FLAG_REPROJECT as well — the lighting history is carried across camera changes (one-sample
// frames on one device).  --camera-step DX: before every frame after the first, DX is added to the camera's origin.x and DX / 100 rad
// to its heading, so that every frame is a moved one; with --accumulate alone the accumulation then restarts every frame, which is
// the baseline --reproject is measured against.
// --history-denoise (with --post --reproject): the denoise is rt_denoise_history with the measured preset (settle 0, 16, 8, 4, 4, 2; no
// count weighting) in place of rt_denoise (Pipeline::enable_history_denoise); the JSON line then carries "history_denoise": true.
//
// --frames-in-flight 2 (one device): the context gets RT_FLAG_FRAMES_IN_FLIGHT_2 and the mirror's draw_frame does not wait for the
// previous frame (Pipeline::set_frames_in_flight), so frame k + 1 is enqueued while frame k runs, as bench.py does by default; with
// --camera-step every frame then runs its own prepass (a still camera's frames reuse their slot's).
//
// --edits N: before every frame, rt_edit_voxels places or breaks (alternating from frame to frame) N voxels of a deterministic brush
// near the camera — a cube of voxels centred 16 texels ahead of it — or, with --edit-spread, N voxels dealt round every 64^3 chunk
// of the region.  After the timed loop the same batches run alone on a second pipeline created with RT_FLAG_TIMING_ALL: the JSON
// line adds the device time of the edit launches per call (rt_get_timing's shade_ms: the rebuild and nibble-map launches, each
// bracketed by events), the launches per call, the host time spent inside rt_edit_voxels and the wall time per call.
//
// --edit-shape sphere:R | box:E: before every frame, rt_edit_shapes carves or fills (alternating from frame to frame) ONE shape where
// --edits puts its brush, centred 16 texels ahead of the camera: a sphere of radius R round that voxel's centre, or a cube of E voxels
// per edge — whose low corner is moved down to a multiple of 64 when E is one (box:64 is exactly one chunk, box:256 the region) —
// clipped to the region.  Timed like --edits; the JSON line carries the same four edit timing fields and "edit_shape".
//
// --edit-stamp N (1..4096): before every frame, rt_edit_stamps pastes N copies of a small built-in stamp (a 5 x 5 x 7 hut: walls, a
// hollow of AIR, ABSENT corners) where --edit-shape puts its shape, side by side in rows of eight and each turned by its index — on odd
// frames an all-AIR stamp of the same extent, which takes the huts away again.  Timed like --edits; the JSON line carries the same
// four edit timing fields and "edit_stamp".
//
// --edit-radius N (with --reproject --edits N): RtConfig.edit_radius — the edits no longer restart the lighting history; every frame
// runs the moved pass with the edited boxes and restarts only the pixels near one or in its sun shadow.  The JSON line's acc_frames /
// samples (rt_get_accumulation) show that the history went on.
//
// --stream (one device): the terrain streams as --camera-step moves the camera — Pipeline::enable_terrain_streaming(seed, "", true),
// one rt_generate_slice per frame while the window lags the camera, lr following.  With --reproject every slab restarts the
// lighting history unless --stream-history (with --edit-radius N) sets RtConfig.stream_history: then a frame after a slab restarts
// only the pixels near the occupied voxels that left or arrived or in their sun shadow.  The JSON line's acc_frames / samples
// (rt_get_accumulation) show whether the history went on.
//
// --rays N: instead of the frame loop, ray queries against the generated world.  rt_trace_rays on N rays — seeded origins in the
// region with random directions, or with --rays-coherent the primary rays of a --width x --height camera at the default pose handed
// over as arbitrary rays — timed call to return (the transfers both ways included; the kernel alone: rocprofv3 --kernel-trace
// --stats, or tools/ray_query_bench.py's device events), then the call-to-return latency of one-pixel rt_pick_pixels, idle and
// right behind a --width x --height --spp --depth frame still in flight.  One JSON line.
// --entity-rays N [--coherent] [--boxes B] [--models M] [--model-scale S]: instead of the frame loop, entity queries.  rt_trace_entities on
// N rays — --rays' seeded rays, or with --coherent its camera rays — against B boxes and M models scattered as --boxes and --models
// scatter them, and rt_trace_rays on the same rays as the yardstick, both timed call to return; then their asynchronous twins on device
// copies of the same records, on a stream of this program's, between two HIP events: the device time of each.  The JSON line also
// counts the rays that report an entity and those whose entity the world occludes.  (The kernels alone, k_entity_query and k_query:
// rocprofv3 --kernel-trace --stats, which tools/entity_query_bench.py runs.)
// --boxes N: instead of the frame loop, entity boxes.  N entity-sized boxes are scattered deterministically in front of the camera
// (20 to 400 units away, over the whole view), their six face probes lit with rt_probe_light (4 samples, depth 2), and rt_draw_boxes
// composites them into a freshly drawn --width x --height frame, 20 times.  One JSON line: the device time of the pass (the launch
// bracketed by events, RT_FLAG_TIMING_ALL), the call-to-return time of rt_draw_boxes and of the probes, and the pixels drawn.
// --particles N [--particle-half H] [--particle-near D]: instead of the frame loop, particles.  A seeded cloud of N cubes of half edge H
// (default 1/16) is scattered in front of the camera, D to 20 D units away (default 10 to 200, log-uniform) over the whole view, lit
// by 64 whole-sphere probes that the particles share, and drawn by rt_draw_particles into a freshly drawn --width x --height frame, 20
// times; with N <= 4096, as a yardstick in the same process, rt_draw_boxes draws the derived boxes, 20 times.  One JSON line: the
// device time per call (the memset and the four launches bracketed by events, RT_FLAG_TIMING_ALL), the call-to-return time and the
// pixels drawn, of both.  (--particle-half 300 --particle-near 400 makes every particle wide: the worst path.)
// --particles N --simulate T [--sweeps S]: instead of drawing the cloud as it stands, simulate it.  The cloud's cubes become debris
// (RtParticleState: the cube as the swept box, a seeded velocity up to 12 units per second per axis, RT_PARTICLE_BOUNCE, gravity 32,
// dt 1/60, restitution 1/2, friction 3/4, S sub-sweeps per tick, default 3) in device buffers.  T ticks follow each other there
// without a host read: a frame, then rt_step_particles_async -> rt_draw_particles_async, the tick's two calls bracketed by events.
// In the same process, between events of their own: the first tick alone, repeated, and rt_sweep_boxes_async — the yardstick — on the
// same boxes with that tick's motions; and the synchronous rt_sweep_boxes on those records, call to return: the host round trip a
// tick on the device replaces (without the upload of the draw records it would also need).  One JSON line.
// --models N [--model-scale S]: instead of the frame loop, voxel-model entities.  One built-in 9 x 9 x 12 sparse stamp (about a third of
// its voxels solid) is drawn N times at scale S (default 1/8) — scattered like --boxes' boxes, in seeded orientations, lit by their
// bounding boxes' face probes — by rt_draw_stamps into a freshly drawn --width x --height frame, 20 times; and, as a yardstick in the
// same process, rt_draw_boxes draws the bounding boxes of the same records, 20 times.  One JSON line: the device time of both passes
// (the launch bracketed by events, RT_FLAG_TIMING_ALL), their ratio, the call-to-return time of rt_draw_stamps and the pixels drawn.
// --shadows N [--shadow-models [--model-scale S]]: instead of the frame loop, entity shadows.  N occluders stand 0.5 to 6 units above what
// N random pixels show — player-sized boxes, or with --shadow-models the 9 x 9 x 12 stamp of --models at scale S in the 48
// orientations in turn — and rt_shadow_entities shades a freshly drawn --width x --height frame with them, 20 times.  As yardsticks in
// the same process rt_draw_boxes draws the same boxes (the models' bounding boxes) and rt_add_lights adds as many lights (at most 1024)
// at the occluders' centres.  One JSON line: the device time of each launch (bracketed by events, RT_FLAG_TIMING_ALL), the
// call-to-return time of rt_shadow_entities and the pixels it changed.
// --lights N: instead of the frame loop, point lights.  N lights of radius 8 are scattered deterministically just off visible
// surfaces — rt_pick_pixels on N pixels spread over the view, each light 1 to 4 units off its hit point along the face's normal (30
// units along the ray where the pixel shows sky) — and rt_add_lights adds them to a freshly drawn --width x --height frame, 20 times.
// One JSON line: the device time of the pass (the launch bracketed by events, RT_FLAG_TIMING_ALL), the call-to-return time of
// rt_add_lights and the pixels lit.
// --light-shadows [--lights N] [--boxes B] [--models M]: instead of the frame loop, point-light shadows of entities.  --lights' N
// lights (64 without --lights); B player-sized boxes and M models (a 5 x 4 x 6 stamp at --model-scale, the 48 orientations in turn),
// each within --occluder-spread units (3) of a light, in turn — or, with --occluders-far, 400 units above it, where no segment of the
// frame passes.  rt_add_lights_occluded lights a freshly drawn frame with them 20 times, then rt_add_lights does as the yardstick.
// One JSON line: device time (the launch bracketed by events) and call-to-return time of both, and the pixels the entities changed.
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "render.hpp"

namespace {

// RingBufferAverage — src/util.rs:175-221
class RingBufferAverage {
 public:
    explicit RingBufferAverage(size_t n) : buf_(n, 0.0), filled_(0), next_(0) {}
    void push_sample(double v) {
        buf_[next_] = v;
        next_ = (next_ + 1) % buf_.size();
        filled_ = std::min(filled_ + 1, buf_.size());
    }
    double average() const {
        double s = 0;
        for (size_t i = 0; i < filled_; i++) s += buf_[i];
        return filled_ ? s / (double)filled_ : 0.0;
    }
    double max() const {
        double m = 0;
        for (size_t i = 0; i < filled_; i++) m = std::max(m, buf_[i]);
        return m;
    }

 private:
    std::vector<double> buf_;
    size_t filled_, next_;
};

RtConfig make_config(int width, int height, int spp, int depth, int device, int rank, int world, uint32_t flags) {
    RtConfig cfg{};
    cfg.struct_size = sizeof(cfg);
    cfg.width = width; cfg.height = height; cfg.region = RT_ROOT_BLOCK_SIZE; cfg.spp = spp; cfg.depth = depth;
    cfg.device = device; cfg.tile_rank = rank; cfg.tile_world = world; cfg.kernel = RT_KERNEL_DEFAULT;
    cfg.flags = flags;
    return cfg;
}

// the host threads of --gpus N meet here once per frame (C++17 has no std::barrier)
class ThreadBarrier {
 public:
    explicit ThreadBarrier(int n) : n_(n) {}
    void arrive_and_wait() {
        std::unique_lock<std::mutex> lk(m_);
        const unsigned long gen = gen_;
        if (++count_ == n_) { count_ = 0; gen_++; cv_.notify_all(); return; }
        cv_.wait(lk, [&] { return gen_ != gen; });
    }
 private:
    std::mutex m_;
    std::condition_variable cv_;
    int n_, count_ = 0;
    unsigned long gen_ = 0;
};

// --edits: the brush of frame-independent voxel positions (texel coordinates of the 256 region)
std::vector<RtVoxelEdit> edit_brush(int n, bool spread, const float origin[3]) {
    const int R = RT_ROOT_BLOCK_SIZE;
    std::vector<RtVoxelEdit> v((size_t)n);
    const int c[3] = {(int)origin[0] + R / 2, (int)origin[1] + R / 2 + 16, (int)origin[2] + R / 2};
    for (int i = 0; i < n; i++) {
        int p[3];
        if (spread) {   // chunk i % 64, then a position inside it that moves with i / 64
            const int ch = i % 64, k = i / 64;
            p[0] = (ch & 3) * 64 + (k * 7) % 64; p[1] = ((ch >> 2) & 3) * 64 + (k * 13) % 64; p[2] = (ch >> 4) * 64 + (k * 29) % 64;
        } else {        // a cube of edge 16 around the centre, further cubes stacked above it for N > 4096
            p[0] = c[0] - 8 + i % 16; p[1] = c[1] - 8 + (i / 16) % 16; p[2] = c[2] - 8 + (i / 256) % 16 + 16 * (i / 4096);
        }
        for (int a = 0; a < 3; a++) p[a] = std::min(std::max(p[a], 0), R - 1);
        RtVoxelEdit& e = v[(size_t)i];
        e.x = (uint16_t)p[0]; e.y = (uint16_t)p[1]; e.z = (uint16_t)p[2];
        e.solid = 1; e.material = (1u << 15) | (90u << 14) | (60u << 7) | 30u; e.reserved = 0;
    }
    return v;
}
void set_solid(std::vector<RtVoxelEdit>& v, int frame) { for (RtVoxelEdit& e : v) e.solid = (uint16_t)((frame & 1) == 0); }

// --edit-shape: "sphere:R" or "box:E" at the brush's centre; false when the text is neither
bool shape_brush(const char* text, const float origin[3], RtShapeEdit* out) {
    const int R = RT_ROOT_BLOCK_SIZE;
    const int c[3] = {(int)origin[0] + R / 2, (int)origin[1] + R / 2 + 16, (int)origin[2] + R / 2};
    RtShapeEdit s{};
    s.material = (1u << 15) | (90u << 14) | (60u << 7) | 30u;
    s.where = RT_WHERE_ALL;
    int n = 0;
    if (std::sscanf(text, "sphere:%d", &n) == 1 && n >= 0 && n <= 2 * R) {
        s.kind = RT_SHAPE_SPHERE;
        for (int a = 0; a < 3; a++) s.a[a] = 2 * c[a] + 1;
        s.b[0] = (2 * n) * (2 * n);
    } else if (std::sscanf(text, "box:%d", &n) == 1 && n >= 1 && n <= R) {
        s.kind = RT_SHAPE_BOX;
        for (int a = 0; a < 3; a++) {
            int lo = std::min(std::max(c[a] - n / 2, 0), R - n);
            if (n % 64 == 0) lo -= lo % 64;
            s.a[a] = lo; s.b[a] = lo + n - 1;
        }
    } else {
        return false;
    }
    *out = s;
    return true;
}

// --edit-stamp: the built-in stamps of one pipeline (ids[0] the hut, ids[1] the all-AIR one) and the placements of N copies
bool stamp_brush_create(rt::render::Pipeline* p, uint32_t ids[2]) {
    const int32_t ext[3] = {5, 5, 7};
    std::vector<uint32_t> mats(5 * 5 * 7, (1u << 15) | (90u << 14) | (60u << 7) | 30u);
    std::vector<uint8_t> hut(5 * 5 * 7), air(5 * 5 * 7, RT_STAMP_AIR);
    for (int z = 0; z < 7; z++)
        for (int y = 0; y < 5; y++)
            for (int x = 0; x < 5; x++) {
                const bool edge_x = x == 0 || x == 4, edge_y = y == 0 || y == 4;
                hut[(size_t)(z * 5 + y) * 5 + x] = (edge_x && edge_y && z > 4) ? RT_STAMP_ABSENT : (edge_x || edge_y || z == 0 || z >= 5) ? RT_STAMP_SOLID : RT_STAMP_AIR;
            }
    return p->stamp_create(ext, mats.data(), hut.data(), &ids[0]) == RT_OK && p->stamp_create(ext, mats.data(), air.data(), &ids[1]) == RT_OK;
}
std::vector<RtStampPlace> stamp_brush(int n, const float origin[3]) {
    const int R = RT_ROOT_BLOCK_SIZE;
    const int c[3] = {(int)origin[0] + R / 2, (int)origin[1] + R / 2 + 16, (int)origin[2] + R / 2};
    std::vector<RtStampPlace> v((size_t)n);
    for (int i = 0; i < n; i++) {
        RtStampPlace& s = v[(size_t)i];
        s = RtStampPlace{};
        const int at[3] = {c[0] - 32 + 8 * (i % 8), c[1] - 32 + 8 * ((i / 8) % 8), c[2] - 8 + 8 * (i / 64)};
        for (int a = 0; a < 3; a++) s.at[a] = std::min(std::max(at[a], 0), R - 8);   // (inside the region, as --edit-shape's box)
        s.orient = (uint8_t)(i % 48);
        s.where = RT_WHERE_ALL;
    }
    return v;
}
void set_stamp(std::vector<RtStampPlace>& v, const uint32_t ids[2], int frame) { for (RtStampPlace& s : v) s.stamp = ids[frame & 1]; }

// --rays: see the head of the file
int run_rays(rt::game::Game& game, const std::vector<uint8_t>& noise, int width, int height, int spp, int depth, int device,
             uint32_t n, bool coherent) {
    std::string err;
    RtConfig cfg = make_config(width, height, spp, depth, device, 0, 1, RT_FLAG_CACHE_PRIMARY);
    rt::render::Pipeline* p = rt::render::create_instance(cfg, noise.data(), game, &err);
    if (!p) { std::fprintf(stderr, "create_instance failed: %s\n", err.c_str()); return 1; }
    RtContext* ctx = p->context();
    // the camera's uniforms, from one drawn frame
    if (p->draw_frame(game) != RT_OK || p->wait() != RT_OK) { std::fprintf(stderr, "frame failed: %s\n", p->last_error()); delete p; return 1; }
    const RtUniforms u = p->uniforms();
    std::vector<RtRay> rays(n);
    std::vector<RtRayHit> hits(n);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (float)((x >> 40) * (1.0 / 16777216.0)); };   // [0, 1)
    for (uint32_t i = 0; i < n; i++) {
        RtRay& r = rays[i];
        r = RtRay{};
        if (coherent) {
            const uint32_t px = i % (uint32_t)width, py = (i / (uint32_t)width) % (uint32_t)height;
            const float sx = ((float)px / (float)width) * 2.0f - 1.0f, sy = ((float)py / (float)height) * 2.0f - 1.0f;
            for (int a = 0; a < 3; a++) { r.origin[a] = u.origin[a]; r.direction[a] = u.forward[a] + u.right[a] * sx + u.up[a] * sy; }
        } else {
            for (int a = 0; a < 3; a++) { r.origin[a] = (rnd() - 0.5f) * 254.0f; r.direction[a] = rnd() * 2.0f - 1.0f; }
        }
    }
    const int32_t lr[3] = {u.lr[0], u.lr[1], u.lr[2]};
    auto ms_since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    int rc = rt_trace_rays(ctx, rays.data(), n, lr, hits.data());   // warm-up (staging grows once)
    const int reps = n >= (1u << 20) ? 5 : 50;
    auto t = std::chrono::steady_clock::now();
    for (int i = 0; i < reps && rc == RT_OK; i++) rc = rt_trace_rays(ctx, rays.data(), n, lr, hits.data());
    const double ms = ms_since(t) / reps;
    uint64_t solid = 0;
    for (const RtRayHit& h : hits) solid += h.kind == RT_HIT_SOLID;
    const int32_t xy[2] = {width / 2, height / 2};
    RtRayHit one{};
    std::vector<double> idle, busy;
    for (int i = 0; i < 220 && rc == RT_OK; i++) {
        t = std::chrono::steady_clock::now();
        rc = rt_pick_pixels(ctx, &u, xy, 1, &one);
        if (i >= 20) idle.push_back(ms_since(t));
    }
    double frame_ms = 0;
    for (int i = 0; i < 21 && rc == RT_OK; i++) {
        const auto tf = std::chrono::steady_clock::now();
        rc = rt_draw_frame(ctx, &u);
        t = std::chrono::steady_clock::now();
        if (rc == RT_OK) rc = rt_pick_pixels(ctx, &u, xy, 1, &one);
        if (i > 0) busy.push_back(ms_since(t));
        if (rc == RT_OK) rc = rt_sync(ctx);
        if (i > 0) frame_ms += ms_since(tf) / 20.0;
    }
    if (rc != RT_OK) { std::fprintf(stderr, "ray queries failed (%d): %s\n", rc, rt_last_error(ctx)); delete p; return 1; }
    std::sort(idle.begin(), idle.end());
    std::sort(busy.begin(), busy.end());
    std::printf("{\"rays\": %u, \"coherent\": %s, \"trace_rays_ms\": %.4f, \"grays_call_to_return\": %.3f, \"solid_hits\": %llu, "
                "\"pick_ms_idle_median\": %.4f, \"pick_ms_in_flight_median\": %.4f, \"pick_ms_in_flight_max\": %.4f, "
                "\"frame\": \"%dx%d spp %d depth %d\", \"frame_ms\": %.3f}\n",
                n, coherent ? "true" : "false", ms, (double)n / (ms * 1e-3) / 1e9, (unsigned long long)solid, idle[idle.size() / 2],
                busy[busy.size() / 2], busy.back(), width, height, spp, depth, frame_ms);
    delete p;
    return 0;
}

// The few HIP runtime calls --entity-rays needs to time the asynchronous calls with an event pair, taken from the runtime the library
// itself runs on (this program is plain C++ and includes no HIP header).  ok == false: no device times.
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
    // `bytes` of device memory holding a copy of `host` (nullptr: uninitialised); nullptr on failure
    void* on_device(const void* host, size_t bytes) const {
        void* p = nullptr;
        if (dev_malloc(&p, bytes ? bytes : 16) != 0) return nullptr;
        if (host && bytes && copy(p, host, bytes, 1 /* hipMemcpyHostToDevice */) != 0) { (void)dev_free(p); return nullptr; }
        return p;
    }
};

// --entity-rays: see the head of the file
int run_entity_rays(rt::game::Game& game, const std::vector<uint8_t>& noise, int width, int height, int spp, int depth, int device, uint32_t n,
                    uint32_t nboxes, uint32_t nmodels, float scale, bool coherent) {
    std::string err;
    RtConfig cfg = make_config(width, height, spp, depth, device, 0, 1, RT_FLAG_CACHE_PRIMARY);
    rt::render::Pipeline* p = rt::render::create_instance(cfg, noise.data(), game, &err);
    if (!p) { std::fprintf(stderr, "create_instance failed: %s\n", err.c_str()); return 1; }
    RtContext* ctx = p->context();
    if (p->draw_frame(game) != RT_OK || p->wait() != RT_OK) { std::fprintf(stderr, "frame failed: %s\n", p->last_error()); delete p; return 1; }
    const RtUniforms u = p->uniforms();
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (float)((x >> 40) * (1.0 / 16777216.0)); };   // [0, 1)
    // the rays of --rays: the camera's primary rays handed over as arbitrary rays, or seeded origins in the region and random directions
    std::vector<RtRay> rays(n);
    for (uint32_t i = 0; i < n; i++) {
        RtRay& r = rays[i];
        r = RtRay{};
        if (coherent) {
            const uint32_t px = i % (uint32_t)width, py = (i / (uint32_t)width) % (uint32_t)height;
            const float sx = ((float)px / (float)width) * 2.0f - 1.0f, sy = ((float)py / (float)height) * 2.0f - 1.0f;
            for (int a = 0; a < 3; a++) { r.origin[a] = u.origin[a]; r.direction[a] = u.forward[a] + u.right[a] * sx + u.up[a] * sy; }
        } else {
            for (int a = 0; a < 3; a++) { r.origin[a] = (rnd() - 0.5f) * 254.0f; r.direction[a] = rnd() * 2.0f - 1.0f; }
        }
    }
    // the entities of --boxes and --models: scattered over the view 20 to 400 units away
    const int32_t E[3] = {9, 9, 12};
    std::vector<uint32_t> mats((size_t)E[0] * E[1] * E[2]);
    std::vector<uint8_t> state(mats.size());
    for (size_t i = 0; i < mats.size(); i++) {
        state[i] = rnd() < 0.3333f ? RT_STAMP_SOLID : (i & 1u ? RT_STAMP_AIR : RT_STAMP_ABSENT);
        mats[i] = (1u << 15) | ((40u + (uint32_t)i % 80u) << 14) | ((30u + (uint32_t)i % 90u) << 7) | (20u + (uint32_t)i % 100u);
    }
    uint32_t id = 0;
    if (p->stamp_create(E, mats.data(), state.data(), &id) != RT_OK) { std::fprintf(stderr, "stamp_create failed: %s\n", p->last_error()); delete p; return 1; }
    static const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    std::vector<RtDrawBox> boxes(nboxes);
    std::vector<RtDrawStamp> models(nmodels);
    for (uint32_t i = 0; i < nboxes + nmodels; i++) {
        const float sx = rnd() * 2.0f - 1.0f, sy = rnd() * 2.0f - 1.0f, dist = 20.0f * std::pow(20.0f, rnd());   // 20 .. 400, log-uniform
        float v[3], len = 0.0f;
        for (int a = 0; a < 3; a++) { v[a] = u.forward[a] + u.right[a] * sx + u.up[a] * sy; len += v[a] * v[a]; }
        len = std::sqrt(len);
        if (i < nboxes) {
            RtDrawBox& b = boxes[i];
            for (int a = 0; a < 3; a++) {
                const float c = u.origin[a] + v[a] / len * dist, half = a == 2 ? 0.9f : 0.3f;   // a player's box: 0.6 x 0.6 x 1.8
                b.lo[a] = c - half; b.hi[a] = c + half;
            }
            b.material = 0x12345u; b.emission = 0xFF000000u;
        } else {
            RtDrawStamp& m = models[i - nboxes];
            m = RtDrawStamp{};
            m.stamp = id; m.scale = scale; m.orient = (uint8_t)(i % 48u); m.emission = 0xFF000000u;
            for (int a = 0; a < 3; a++) m.origin[a] = u.origin[a] + v[a] / len * dist - 0.5f * (float)E[perms[m.orient >> 3][a]] * scale;
        }
    }
    const int32_t lr[3] = {u.lr[0], u.lr[1], u.lr[2]};
    auto ms_since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    std::vector<RtRayHit> world(n), plain(n);
    std::vector<RtEntityHit> hits(n);
    const int reps = n >= (1u << 20) ? 5 : 20;
    double ms[2] = {0.0, 0.0};
    int rc = RT_OK;
    for (int which = 0; which < 2 && rc == RT_OK; which++) {      // 0: rt_trace_entities, 1: rt_trace_rays on the same rays, the yardstick
        for (int i = 0; i < reps + 1 && rc == RT_OK; i++) {       // (the first repetition warms the staging up)
            const auto t = std::chrono::steady_clock::now();
            rc = which == 0 ? rt_trace_entities(ctx, rays.data(), n, lr, boxes.data(), nboxes, models.data(), nmodels, world.data(), hits.data())
                            : rt_trace_rays(ctx, rays.data(), n, lr, plain.data());
            if (i > 0) ms[which] += ms_since(t) / reps;
        }
    }
    if (rc != RT_OK) { std::fprintf(stderr, "entity queries failed (%d): %s\n", rc, rt_last_error(ctx)); delete p; return 1; }
    if (std::memcmp(world.data(), plain.data(), (size_t)n * sizeof(RtRayHit)) != 0) { std::fprintf(stderr, "the world hits differ from rt_trace_rays'\n"); delete p; return 1; }
    // reported: the call's own answer; occluded: rays that report an entity only once the world is out of the way — the same call with
    // the window moved 2^20 voxels off, where every ray leaves the region at once (D = 65535)
    uint64_t reported = 0, under_sky = 0, met = 0;
    for (uint32_t i = 0; i < n; i++) { reported += hits[i].kind != RT_ENTITY_NONE; under_sky += hits[i].kind != RT_ENTITY_NONE && world[i].kind == RT_HIT_AIR; }
    const int32_t away[3] = {lr[0] + (1 << 20), lr[1], lr[2]};
    rc = rt_trace_entities(ctx, rays.data(), n, away, boxes.data(), nboxes, models.data(), nmodels, nullptr, hits.data());
    if (rc != RT_OK) { std::fprintf(stderr, "entity queries failed (%d): %s\n", rc, rt_last_error(ctx)); delete p; return 1; }
    for (uint32_t i = 0; i < n; i++) met += hits[i].kind != RT_ENTITY_NONE;
    // device time of each call: the asynchronous twins on device copies of the same records, on a stream of this program's, between
    // two events (-1: the HIP runtime could not be reached from here)
    double device_ms[2] = {-1.0, -1.0};
    const HipEvents hip;
    if (hip.ok) {
        void *st = nullptr, *e0 = nullptr, *e1 = nullptr;
        void* d_rays = hip.on_device(rays.data(), (size_t)n * sizeof(RtRay));
        void* d_boxes = hip.on_device(boxes.data(), (size_t)nboxes * sizeof(RtDrawBox));
        void* d_world = hip.on_device(nullptr, (size_t)n * sizeof(RtRayHit));
        void* d_hits = hip.on_device(nullptr, (size_t)n * sizeof(RtEntityHit));
        bool fine = d_rays && d_boxes && d_world && d_hits && hip.stream_create(&st) == 0 && hip.event_create(&e0) == 0 && hip.event_create(&e1) == 0 &&
                    rt_set_stream(ctx, st) == RT_OK;
        for (int which = 0; which < 2 && fine; which++) {
            for (int i = 0; i < reps + 1 && fine; i++) {          // (the first repetition warms up; the events bracket the others)
                if (i == 1) fine = hip.event_record(e0, st) == 0;
                if (fine)
                    fine = (which == 0 ? rt_trace_entities_async(ctx, (const RtRay*)d_rays, n, lr, nboxes ? (const RtDrawBox*)d_boxes : nullptr, nboxes,
                                                                 models.data(), nmodels, (RtRayHit*)d_world, (RtEntityHit*)d_hits)
                                       : rt_trace_rays_async(ctx, (const RtRay*)d_rays, n, lr, (RtRayHit*)d_world)) == RT_OK;
            }
            float ms_f = 0.0f;
            fine = fine && hip.event_record(e1, st) == 0 && hip.event_sync(e1) == 0 && hip.elapsed(&ms_f, e0, e1) == 0;
            if (fine) device_ms[which] = (double)ms_f / reps;
        }
        if (rt_sync(ctx) != RT_OK || rt_set_stream(ctx, nullptr) != RT_OK) fine = false;
        if (e0) (void)hip.event_destroy(e0);
        if (e1) (void)hip.event_destroy(e1);
        if (st) (void)hip.stream_destroy(st);
        for (void* d : {d_rays, d_boxes, d_world, d_hits})
            if (d) (void)hip.dev_free(d);
        if (!fine) { std::fprintf(stderr, "timing the asynchronous calls failed: %s\n", rt_last_error(ctx)); delete p; return 1; }
    }
    std::printf("{\"entity_rays\": %u, \"coherent\": %s, \"boxes\": %u, \"models\": %u, \"model_scale\": %g, \"trace_entities_call_ms\": %.4f, "
                "\"trace_rays_call_ms\": %.4f, \"ratio\": %.2f, \"entities_reported\": %llu, \"entities_occluded\": %llu, \"reported_under_sky\": %llu, "
                "\"trace_entities_device_ms\": %.4f, \"trace_rays_device_ms\": %.4f}\n",
                n, coherent ? "true" : "false", nboxes, nmodels, (double)scale, ms[0], ms[1], ms[1] > 0.0 ? ms[0] / ms[1] : 0.0,
                (unsigned long long)reported, (unsigned long long)(met > reported ? met - reported : 0), (unsigned long long)under_sky, device_ms[0], device_ms[1]);
    delete p;
    return 0;
}

// --boxes: see the head of the file
int run_boxes(rt::game::Game& game, const std::vector<uint8_t>& noise, int width, int height, int spp, int depth, int device, uint32_t n) {
    std::string err;
    RtConfig cfg = make_config(width, height, spp, depth, device, 0, 1, RT_FLAG_CACHE_PRIMARY | RT_FLAG_TIMING_ALL);
    rt::render::Pipeline* p = rt::render::create_instance(cfg, noise.data(), game, &err);
    if (!p) { std::fprintf(stderr, "create_instance failed: %s\n", err.c_str()); return 1; }
    RtContext* ctx = p->context();
    if (p->draw_frame(game) != RT_OK || p->wait() != RT_OK) { std::fprintf(stderr, "frame failed: %s\n", p->last_error()); delete p; return 1; }
    const RtUniforms u = p->uniforms();
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (float)((x >> 40) * (1.0 / 16777216.0)); };   // [0, 1)
    std::vector<RtDrawBox> boxes(n);
    std::vector<RtLightProbe> probes(6u * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        const float sx = rnd() * 2.0f - 1.0f, sy = rnd() * 2.0f - 1.0f, dist = 20.0f * std::pow(20.0f, rnd());   // 20 .. 400, log-uniform
        float v[3], len = 0.0f;
        for (int a = 0; a < 3; a++) { v[a] = u.forward[a] + u.right[a] * sx + u.up[a] * sy; len += v[a] * v[a]; }
        len = std::sqrt(len);
        RtDrawBox& b = boxes[i];
        for (int a = 0; a < 3; a++) {
            const float c = u.origin[a] + v[a] / len * dist, half = a == 2 ? 0.9f : 0.3f;   // a player's box: 0.6 x 0.6 x 1.8
            b.lo[a] = c - half; b.hi[a] = c + half;
        }
        b.material = (1u << 15) | ((40u + i % 80u) << 14) | ((30u + i % 90u) << 7) | (20u + i % 100u);
        b.emission = 0xFF000000u;
        for (uint32_t code = 0; code < 6u; code++) {   // the face centre, 0.001 off the face along its normal
            RtLightProbe& q = probes[6u * (size_t)i + code];
            q = RtLightProbe{};
            for (int a = 0; a < 3; a++) q.position[a] = (b.lo[a] + b.hi[a]) * 0.5f;
            const int a = (int)(code / 2u);
            q.position[a] = code % 2u == 0u ? b.hi[a] + 0.001f : b.lo[a] - 0.001f;
            q.normal = code;
            q.cell[0] = (uint16_t)(i % 16u); q.cell[1] = (uint16_t)((i / 16u) % 16u);
        }
    }
    auto ms_since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    std::vector<RtProbeLight> lights(probes.size());
    auto t = std::chrono::steady_clock::now();
    int rc = n ? rt_probe_light(ctx, &u, probes.data(), (uint32_t)probes.size(), 4, 2, lights.data()) : RT_OK;
    const double probe_ms = ms_since(t);
    const size_t npix = (size_t)width * (size_t)height;
    std::vector<float> before(npix), after(npix);
    if (rc == RT_OK) rc = rt_readback(ctx, RT_BUF_DEPTH_F32, before.data(), npix * sizeof(float));
    const int reps = 20;
    double device_ms = 0.0, call_ms = 0.0;
    uint32_t launches = 0;
    for (int i = 0; i < reps + 1 && rc == RT_OK; i++) {   // (the first repetition warms the staging up)
        RtTiming tm{};
        rc = rt_draw_frame(ctx, &u);
        if (rc == RT_OK) rc = rt_sync(ctx);
        if (rc == RT_OK) rc = rt_get_timing(ctx, &tm);   // (drains the frame's own launches)
        t = std::chrono::steady_clock::now();
        if (rc == RT_OK) rc = rt_draw_boxes(ctx, &u, boxes.data(), lights.data(), n);
        const double call = ms_since(t);
        if (rc == RT_OK) rc = rt_get_timing(ctx, &tm);
        if (i > 0) { device_ms += tm.shade_ms / reps; call_ms += call / reps; launches += tm.other_launches; }
    }
    if (rc == RT_OK) rc = rt_readback(ctx, RT_BUF_DEPTH_F32, after.data(), npix * sizeof(float));
    if (rc != RT_OK) { std::fprintf(stderr, "entity boxes failed (%d): %s\n", rc, rt_last_error(ctx)); delete p; return 1; }
    uint64_t drawn = 0;
    for (size_t i = 0; i < npix; i++) drawn += std::memcmp(&before[i], &after[i], 4) != 0;
    std::printf("{\"boxes\": %u, \"frame\": \"%dx%d spp %d depth %d\", \"draw_boxes_device_ms\": %.4f, \"draw_boxes_call_ms\": %.4f, "
                "\"launches_per_call\": %.2f, \"probe_light_call_ms\": %.3f, \"pixels_drawn\": %llu}\n",
                n, width, height, spp, depth, device_ms, call_ms, (double)launches / reps, probe_ms, (unsigned long long)drawn);
    delete p;
    return 0;
}

// --particles: see the head of the file
int run_particles(rt::game::Game& game, const std::vector<uint8_t>& noise, int width, int height, int spp, int depth, int device, uint32_t n, float half,
                  float near_dist) {
    std::string err;
    RtConfig cfg = make_config(width, height, spp, depth, device, 0, 1, RT_FLAG_CACHE_PRIMARY | RT_FLAG_TIMING_ALL);
    rt::render::Pipeline* p = rt::render::create_instance(cfg, noise.data(), game, &err);
    if (!p) { std::fprintf(stderr, "create_instance failed: %s\n", err.c_str()); return 1; }
    RtContext* ctx = p->context();
    if (p->draw_frame(game) != RT_OK || p->wait() != RT_OK) { std::fprintf(stderr, "frame failed: %s\n", p->last_error()); delete p; return 1; }
    const RtUniforms u = p->uniforms();
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (float)((x >> 40) * (1.0 / 16777216.0)); };   // [0, 1)
    const uint32_t nlights = 64;
    std::vector<RtParticle> particles(n);
    std::vector<RtDrawBox> boxes(n <= 4096u ? n : 0u);            // the yardstick: rt_draw_boxes on the derived boxes
    std::vector<RtLightProbe> probes(nlights);
    for (uint32_t i = 0; i < n; i++) {
        const float sx = rnd() * 2.0f - 1.0f, sy = rnd() * 2.0f - 1.0f, dist = near_dist * std::pow(20.0f, rnd());   // near .. 20 near, log-uniform
        float v[3], len = 0.0f;
        for (int a = 0; a < 3; a++) { v[a] = u.forward[a] + u.right[a] * sx + u.up[a] * sy; len += v[a] * v[a]; }
        len = std::sqrt(len);
        RtParticle& q = particles[i];
        q = RtParticle{};
        for (int a = 0; a < 3; a++) q.center[a] = u.origin[a] + v[a] / len * dist;
        q.half = half;
        q.material = (1u << 15) | ((40u + i % 80u) << 14) | ((30u + i % 90u) << 7) | (20u + i % 100u);
        q.emission = 0xFF000000u;
        q.light = i % nlights;
        if (i < boxes.size()) {
            RtDrawBox& b = boxes[i];
            for (int a = 0; a < 3; a++) { b.lo[a] = q.center[a] - q.half; b.hi[a] = q.center[a] + q.half; }
            b.material = q.material; b.emission = q.emission;
        }
        if (i < nlights) {                                        // one whole-sphere probe per cluster, where its first particle is
            RtLightProbe& l = probes[i];
            l = RtLightProbe{};
            for (int a = 0; a < 3; a++) l.position[a] = q.center[a];
            l.normal = RT_PROBE_SPHERE;
            l.cell[0] = (uint16_t)(i % 16u); l.cell[1] = (uint16_t)(i / 16u);
        }
    }
    auto ms_since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    std::vector<RtProbeLight> lights(nlights);
    int rc = n ? rt_probe_light(ctx, &u, probes.data(), n < nlights ? n : nlights, 4, 2, lights.data()) : RT_OK;
    std::vector<RtProbeLight> face(6u * boxes.size());
    for (size_t i = 0; i < face.size(); i++) face[i] = lights[particles[i / 6u].light];
    const size_t npix = (size_t)width * (size_t)height;
    std::vector<float> before(npix), after(npix);
    if (rc == RT_OK) rc = rt_readback(ctx, RT_BUF_DEPTH_F32, before.data(), npix * sizeof(float));
    const int reps = 20;
    double device_ms[2] = {0.0, 0.0}, call_ms[2] = {0.0, 0.0};
    uint64_t drawn[2] = {0, 0};
    for (int pass = 0; pass < (boxes.empty() ? 1 : 2) && rc == RT_OK; pass++) {     // 0: the particles, 1: their boxes
        for (int i = 0; i < reps + 1 && rc == RT_OK; i++) {   // (the first repetition warms the staging and the scratch up)
            RtTiming tm{};
            rc = rt_draw_frame(ctx, &u);
            if (rc == RT_OK) rc = rt_sync(ctx);
            if (rc == RT_OK) rc = rt_get_timing(ctx, &tm);   // (drains the frame's own launches)
            auto t = std::chrono::steady_clock::now();
            if (rc == RT_OK) rc = pass == 0 ? rt_draw_particles(ctx, &u, particles.data(), n, lights.data(), nlights)
                                            : rt_draw_boxes(ctx, &u, boxes.data(), face.data(), n);
            const double call = ms_since(t);
            if (rc == RT_OK) rc = rt_get_timing(ctx, &tm);
            if (i > 0) { device_ms[pass] += tm.shade_ms / reps; call_ms[pass] += call / reps; }
        }
        if (rc == RT_OK) rc = rt_readback(ctx, RT_BUF_DEPTH_F32, after.data(), npix * sizeof(float));
        for (size_t i = 0; i < npix; i++) drawn[pass] += std::memcmp(&before[i], &after[i], 4) != 0;
    }
    if (rc != RT_OK) { std::fprintf(stderr, "particles failed (%d): %s\n", rc, rt_last_error(ctx)); delete p; return 1; }
    std::printf("{\"particles\": %u, \"half\": %g, \"near\": %g, \"frame\": \"%dx%d spp %d depth %d\", \"draw_particles_device_ms\": %.4f, "
                "\"draw_particles_call_ms\": %.4f, \"pixels_drawn\": %llu",
                n, (double)half, (double)near_dist, width, height, spp, depth, device_ms[0], call_ms[0], (unsigned long long)drawn[0]);
    if (!boxes.empty())
        std::printf(", \"draw_boxes_device_ms\": %.4f, \"draw_boxes_call_ms\": %.4f, \"boxes_pixels_drawn\": %llu", device_ms[1], call_ms[1],
                    (unsigned long long)drawn[1]);
    std::printf("}\n");
    delete p;
    return 0;
}

// --particles N --simulate T: see the head of the file
int run_simulate(rt::game::Game& game, const std::vector<uint8_t>& noise, int width, int height, int spp, int depth, int device, uint32_t n, float half,
                 float near_dist, int ticks, uint32_t sweeps) {
    std::string err;
    RtConfig cfg = make_config(width, height, spp, depth, device, 0, 1, RT_FLAG_CACHE_PRIMARY);
    rt::render::Pipeline* p = rt::render::create_instance(cfg, noise.data(), game, &err);
    if (!p) { std::fprintf(stderr, "create_instance failed: %s\n", err.c_str()); return 1; }
    RtContext* ctx = p->context();
    if (p->draw_frame(game) != RT_OK || p->wait() != RT_OK) { std::fprintf(stderr, "frame failed: %s\n", p->last_error()); delete p; return 1; }
    const RtUniforms u = p->uniforms();
    const HipEvents hip;
    if (!hip.ok) { std::fprintf(stderr, "--simulate needs the HIP runtime for its device buffers\n"); delete p; return 1; }
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (float)((x >> 40) * (1.0 / 16777216.0)); };   // [0, 1)
    RtParticleStep step{};
    step.dt = 1.0f / 60.0f; step.accel[2] = -32.0f; step.damping = 1.0f; step.restitution = 0.5f; step.friction = 0.75f; step.rest_speed = 0.5f;
    for (int a = 0; a < 3; a++) step.lr[a] = u.lr[a];
    step.sweeps = sweeps;
    // debris: --particles' cloud, every cube with a seeded velocity; and the same boxes with the first tick's motions as plain sweeps
    const uint32_t nlights = 64;
    std::vector<RtParticleState> states(n);
    std::vector<RtBoxSweep> as_sweeps(n);
    std::vector<RtLightProbe> probes(nlights);
    for (uint32_t i = 0; i < n; i++) {
        const float sx = rnd() * 2.0f - 1.0f, sy = rnd() * 2.0f - 1.0f, dist = near_dist * std::pow(20.0f, rnd());
        float v[3], len = 0.0f;
        for (int a = 0; a < 3; a++) { v[a] = u.forward[a] + u.right[a] * sx + u.up[a] * sy; len += v[a] * v[a]; }
        len = std::sqrt(len);
        RtParticleState& s = states[i];
        s = RtParticleState{};
        RtBoxSweep& w = as_sweeps[i];
        w = RtBoxSweep{};
        for (int a = 0; a < 3; a++) {
            const float c = u.origin[a] + v[a] / len * dist;
            s.lo[a] = w.lo[a] = c - half; s.hi[a] = w.hi[a] = c + half;
            s.velocity[a] = (rnd() * 2.0f - 1.0f) * 12.0f;
            const float m = (s.velocity[a] + step.accel[a] * step.dt) * step.damping * step.dt;
            w.motion[a] = m < -64.0f ? -64.0f : (m > 64.0f ? 64.0f : m);
        }
        s.life = INFINITY; s.flags = RT_PARTICLE_BOUNCE; s.half = half; s.light = i % nlights;
        s.material = (1u << 15) | ((40u + i % 80u) << 14) | ((30u + i % 90u) << 7) | (20u + i % 100u);
        s.emission = 0xFF000000u;
        if (i < nlights) {
            RtLightProbe& l = probes[i];
            l = RtLightProbe{};
            for (int a = 0; a < 3; a++) l.position[a] = 0.5f * (s.lo[a] + s.hi[a]);
            l.normal = RT_PROBE_SPHERE;
            l.cell[0] = (uint16_t)(i % 16u); l.cell[1] = (uint16_t)(i / 16u);
        }
    }
    auto ms_since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    const int32_t lr[3] = {u.lr[0], u.lr[1], u.lr[2]};
    std::vector<RtProbeLight> lights(nlights);
    int rc = n ? rt_probe_light(ctx, &u, probes.data(), n < nlights ? n : nlights, 4, 2, lights.data()) : RT_OK;
    // the host round trip a tick on the device replaces, in part: the synchronous sweep of the same records
    std::vector<RtSweepHit> hits(n);
    const int reps = n >= (1u << 19) ? 5 : 20;
    double sync_ms = 0.0;
    for (int i = 0; i < 4 && rc == RT_OK; i++) {                  // (the first call warms the staging up)
        const auto t = std::chrono::steady_clock::now();
        rc = rt_sweep_boxes(ctx, as_sweeps.data(), n, lr, hits.data());
        if (i > 0) sync_ms += ms_since(t) / 3.0;
    }
    uint64_t blocked = 0;
    for (uint32_t i = 0; i < n; i++) blocked += hits[i].kind == RT_SWEEP_BLOCKED;
    if (rc != RT_OK) { std::fprintf(stderr, "simulate failed (%d): %s\n", rc, rt_last_error(ctx)); delete p; return 1; }
    void *st = nullptr, *e0 = nullptr, *e1 = nullptr;
    void* d_a = hip.on_device(states.data(), (size_t)n * sizeof(RtParticleState));
    void* d_b = hip.on_device(nullptr, (size_t)n * sizeof(RtParticleState));
    void* d_first = hip.on_device(states.data(), (size_t)n * sizeof(RtParticleState));
    void* d_draw = hip.on_device(nullptr, (size_t)n * sizeof(RtParticle));
    void* d_sweeps = hip.on_device(as_sweeps.data(), (size_t)n * sizeof(RtBoxSweep));
    void* d_hits = hip.on_device(nullptr, (size_t)n * sizeof(RtSweepHit));
    void* d_lights = hip.on_device(lights.data(), (size_t)nlights * sizeof(RtProbeLight));
    bool fine = d_a && d_b && d_first && d_draw && d_sweeps && d_hits && d_lights && hip.stream_create(&st) == 0 && hip.event_create(&e0) == 0 &&
                hip.event_create(&e1) == 0 && rt_set_stream(ctx, st) == RT_OK;
    // the first tick from the initial states and the plain sweep of the same boxes and motions: the same launch repeated between two events
    double first_ms[2] = {-1.0, -1.0};
    for (int which = 0; which < 2 && fine; which++) {
        for (int i = 0; i < reps + 1 && fine; i++) {
            if (i == 1) fine = hip.event_record(e0, st) == 0;
            if (fine)
                fine = (which == 0 ? rt_step_particles_async(ctx, &step, (const RtParticleState*)d_first, (RtParticleState*)d_b, (RtParticle*)d_draw, n)
                                   : rt_sweep_boxes_async(ctx, (const RtBoxSweep*)d_sweeps, n, lr, (RtSweepHit*)d_hits)) == RT_OK;
        }
        float ms_f = 0.0f;
        fine = fine && hip.event_record(e1, st) == 0 && hip.event_sync(e1) == 0 && hip.elapsed(&ms_f, e0, e1) == 0;
        if (fine) first_ms[which] = (double)ms_f / reps;
    }
    // T ticks chained on the device: the frame (not timed), then step -> draw between two events
    double tick_ms = 0.0;
    for (int t = 0; t < ticks && fine; t++) {
        fine = rt_draw_frame(ctx, &u) == RT_OK && hip.event_record(e0, st) == 0 &&
               rt_step_particles_async(ctx, &step, (const RtParticleState*)d_a, (RtParticleState*)d_b, (RtParticle*)d_draw, n) == RT_OK &&
               rt_draw_particles_async(ctx, &u, (const RtParticle*)d_draw, n, (const RtProbeLight*)d_lights, nlights) == RT_OK;
        float ms_f = 0.0f;
        fine = fine && hip.event_record(e1, st) == 0 && hip.event_sync(e1) == 0 && hip.elapsed(&ms_f, e0, e1) == 0;
        tick_ms += (double)ms_f / ticks;
        std::swap(d_a, d_b);
    }
    uint64_t alive = 0, contact = 0;
    if (fine && n) {
        fine = rt_sync(ctx) == RT_OK && hip.copy(states.data(), d_a, (size_t)n * sizeof(RtParticleState), 2 /* hipMemcpyDeviceToHost */) == 0;
        for (uint32_t i = 0; i < n; i++) { alive += !(states[i].flags & (RT_PSTATE_DEAD | RT_PSTATE_INVALID)); contact += (states[i].flags & RT_PSTATE_CONTACT) != 0; }
    }
    if (rt_sync(ctx) != RT_OK || rt_set_stream(ctx, nullptr) != RT_OK) fine = false;
    if (e0) (void)hip.event_destroy(e0);
    if (e1) (void)hip.event_destroy(e1);
    if (st) (void)hip.stream_destroy(st);
    for (void* d : {d_a, d_b, d_first, d_draw, d_sweeps, d_hits, d_lights})
        if (d) (void)hip.dev_free(d);
    if (!fine) { std::fprintf(stderr, "simulate failed: %s\n", rt_last_error(ctx)); delete p; return 1; }
    std::printf("{\"particles\": %u, \"half\": %g, \"simulate\": %d, \"sweeps\": %u, \"frame\": \"%dx%d spp %d depth %d\", \"step_device_ms\": %.4f, "
                "\"sweep_boxes_device_ms\": %.4f, \"step_over_sweep\": %.2f, \"tick_device_ms\": %.4f, \"sweep_boxes_sync_call_ms\": %.3f, "
                "\"first_tick_blocked\": %llu, \"alive\": %llu, \"in_contact_last_tick\": %llu}\n",
                n, (double)half, ticks, sweeps, width, height, spp, depth, first_ms[0], first_ms[1], first_ms[1] > 0.0 ? first_ms[0] / first_ms[1] : 0.0,
                tick_ms, sync_ms, (unsigned long long)blocked, (unsigned long long)alive, (unsigned long long)contact);
    delete p;
    return 0;
}

// --models: see the head of the file
int run_models(rt::game::Game& game, const std::vector<uint8_t>& noise, int width, int height, int spp, int depth, int device, uint32_t n, float scale) {
    std::string err;
    RtConfig cfg = make_config(width, height, spp, depth, device, 0, 1, RT_FLAG_CACHE_PRIMARY | RT_FLAG_TIMING_ALL);
    rt::render::Pipeline* p = rt::render::create_instance(cfg, noise.data(), game, &err);
    if (!p) { std::fprintf(stderr, "create_instance failed: %s\n", err.c_str()); return 1; }
    RtContext* ctx = p->context();
    if (p->draw_frame(game) != RT_OK || p->wait() != RT_OK) { std::fprintf(stderr, "frame failed: %s\n", p->last_error()); delete p; return 1; }
    const RtUniforms u = p->uniforms();
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (float)((x >> 40) * (1.0 / 16777216.0)); };   // [0, 1)
    // the stamp: a third solid, the rest air and absent in turn, a material per voxel
    const int32_t E[3] = {9, 9, 12};
    std::vector<uint32_t> mats((size_t)E[0] * E[1] * E[2]);
    std::vector<uint8_t> state(mats.size());
    for (size_t i = 0; i < mats.size(); i++) {
        const float r = rnd();
        state[i] = r < 0.3333f ? RT_STAMP_SOLID : (i & 1u ? RT_STAMP_AIR : RT_STAMP_ABSENT);
        mats[i] = (1u << 15) | ((40u + (uint32_t)i % 80u) << 14) | ((30u + (uint32_t)i % 90u) << 7) | (20u + (uint32_t)i % 100u);
    }
    uint32_t id = 0;
    if (p->stamp_create(E, mats.data(), state.data(), &id) != RT_OK) { std::fprintf(stderr, "stamp_create failed: %s\n", p->last_error()); delete p; return 1; }
    static const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    std::vector<RtDrawStamp> models(n);
    std::vector<RtDrawBox> boxes(n);
    std::vector<RtLightProbe> probes(6u * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        const float sx = rnd() * 2.0f - 1.0f, sy = rnd() * 2.0f - 1.0f, dist = 20.0f * std::pow(20.0f, rnd());   // 20 .. 400, log-uniform
        float v[3], len = 0.0f;
        for (int a = 0; a < 3; a++) { v[a] = u.forward[a] + u.right[a] * sx + u.up[a] * sy; len += v[a] * v[a]; }
        len = std::sqrt(len);
        RtDrawStamp& m = models[i];
        m = RtDrawStamp{};
        m.stamp = id; m.scale = scale; m.orient = (uint8_t)(i % 48u); m.emission = 0xFF000000u;
        RtDrawBox& b = boxes[i];
        for (int a = 0; a < 3; a++) {
            const float ext = (float)E[perms[m.orient >> 3][a]];
            m.origin[a] = u.origin[a] + v[a] / len * dist - 0.5f * ext * scale;
            b.lo[a] = m.origin[a]; b.hi[a] = std::fma(ext, scale, m.origin[a]);
        }
        b.material = mats[0]; b.emission = m.emission;
        for (uint32_t code = 0; code < 6u; code++) {   // the bounding box's face centre, 0.001 off the face along its normal
            RtLightProbe& q = probes[6u * (size_t)i + code];
            q = RtLightProbe{};
            for (int a = 0; a < 3; a++) q.position[a] = (b.lo[a] + b.hi[a]) * 0.5f;
            const int a = (int)(code / 2u);
            q.position[a] = code % 2u == 0u ? b.hi[a] + 0.001f : b.lo[a] - 0.001f;
            q.normal = code;
            q.cell[0] = (uint16_t)(i % 16u); q.cell[1] = (uint16_t)((i / 16u) % 16u);
        }
    }
    auto ms_since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    std::vector<RtProbeLight> lights(probes.size());
    int rc = n ? rt_probe_light(ctx, &u, probes.data(), (uint32_t)probes.size(), 4, 2, lights.data()) : RT_OK;
    const size_t npix = (size_t)width * (size_t)height;
    std::vector<float> before(npix), after(npix);
    if (rc == RT_OK) rc = rt_readback(ctx, RT_BUF_DEPTH_F32, before.data(), npix * sizeof(float));
    const int reps = 20;
    double device_ms[2] = {0.0, 0.0}, call_ms[2] = {0.0, 0.0};
    uint64_t drawn[2] = {0, 0};
    for (int pass = 0; pass < 2 && rc == RT_OK; pass++) {       // 0: the models, 1: their bounding boxes
        for (int i = 0; i < reps + 1 && rc == RT_OK; i++) {      // (the first repetition warms the staging up)
            RtTiming tm{};
            rc = rt_draw_frame(ctx, &u);
            if (rc == RT_OK) rc = rt_sync(ctx);
            if (rc == RT_OK) rc = rt_get_timing(ctx, &tm);       // (drains the frame's own launches)
            auto t = std::chrono::steady_clock::now();
            if (rc == RT_OK) rc = pass == 0 ? rt_draw_stamps(ctx, &u, models.data(), lights.data(), n) : rt_draw_boxes(ctx, &u, boxes.data(), lights.data(), n);
            const double call = ms_since(t);
            if (rc == RT_OK) rc = rt_get_timing(ctx, &tm);
            if (i > 0) { device_ms[pass] += tm.shade_ms / reps; call_ms[pass] += call / reps; }
        }
        if (rc == RT_OK) rc = rt_readback(ctx, RT_BUF_DEPTH_F32, after.data(), npix * sizeof(float));
        for (size_t i = 0; i < npix; i++) drawn[pass] += std::memcmp(&before[i], &after[i], 4) != 0;
    }
    if (rc != RT_OK) { std::fprintf(stderr, "voxel-model entities failed (%d): %s\n", rc, rt_last_error(ctx)); delete p; return 1; }
    std::printf("{\"models\": %u, \"model_scale\": %g, \"frame\": \"%dx%d spp %d depth %d\", \"draw_stamps_device_ms\": %.4f, "
                "\"bounding_boxes_device_ms\": %.4f, \"ratio\": %.2f, \"draw_stamps_call_ms\": %.4f, \"draw_boxes_call_ms\": %.4f, "
                "\"pixels_drawn\": %llu, \"bounding_box_pixels\": %llu}\n",
                n, (double)scale, width, height, spp, depth, device_ms[0], device_ms[1], device_ms[1] > 0.0 ? device_ms[0] / device_ms[1] : 0.0,
                call_ms[0], call_ms[1], (unsigned long long)drawn[0], (unsigned long long)drawn[1]);
    delete p;
    return 0;
}

// --lights: see the head of the file
int run_lights(rt::game::Game& game, const std::vector<uint8_t>& noise, int width, int height, int spp, int depth, int device, uint32_t n) {
    std::string err;
    RtConfig cfg = make_config(width, height, spp, depth, device, 0, 1, RT_FLAG_CACHE_PRIMARY | RT_FLAG_TIMING_ALL);
    rt::render::Pipeline* p = rt::render::create_instance(cfg, noise.data(), game, &err);
    if (!p) { std::fprintf(stderr, "create_instance failed: %s\n", err.c_str()); return 1; }
    RtContext* ctx = p->context();
    if (p->draw_frame(game) != RT_OK || p->wait() != RT_OK) { std::fprintf(stderr, "frame failed: %s\n", p->last_error()); delete p; return 1; }
    const RtUniforms u = p->uniforms();
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (float)((x >> 40) * (1.0 / 16777216.0)); };   // [0, 1)
    std::vector<int32_t> xy(2u * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        xy[2u * i] = std::min(width - 1, (int)(rnd() * (float)width));
        xy[2u * i + 1] = std::min(height - 1, (int)(rnd() * (float)height));
    }
    std::vector<RtRayHit> hits(n);
    int rc = n ? rt_pick_pixels(ctx, &u, xy.data(), n, hits.data()) : RT_OK;
    std::vector<RtPointLight> lights(n);
    for (uint32_t i = 0; i < n && rc == RT_OK; i++) {
        RtPointLight& l = lights[i];
        l = RtPointLight{};
        const float off = 1.0f + 3.0f * rnd();
        if (hits[i].kind == RT_HIT_SOLID) {
            for (int a = 0; a < 3; a++) l.position[a] = hits[i].position[a];
            l.position[hits[i].normal / 2u] += hits[i].normal % 2u == 0u ? off : -off;
        } else {
            const float sx = ((float)xy[2u * i] / (float)width) * 2.0f - 1.0f, sy = ((float)xy[2u * i + 1] / (float)height) * 2.0f - 1.0f;
            float v[3], len = 0.0f;
            for (int a = 0; a < 3; a++) { v[a] = u.forward[a] + u.right[a] * sx + u.up[a] * sy; len += v[a] * v[a]; }
            len = std::sqrt(len);
            for (int a = 0; a < 3; a++) l.position[a] = u.origin[a] + v[a] / len * 30.0f;
        }
        l.radius = 8.0f;
        l.color[0] = 20.0f + 20.0f * rnd(); l.color[1] = 15.0f + 15.0f * rnd(); l.color[2] = 5.0f + 10.0f * rnd();
    }
    auto ms_since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    const size_t npix = (size_t)width * (size_t)height;
    std::vector<float> before(4u * npix), after(4u * npix);
    const int reps = 20;
    double device_ms = 0.0, call_ms = 0.0;
    uint32_t launches = 0;
    for (int i = 0; i < reps + 1 && rc == RT_OK; i++) {   // (the first repetition warms the staging up)
        RtTiming tm{};
        rc = rt_draw_frame(ctx, &u);
        if (rc == RT_OK) rc = rt_sync(ctx);
        if (rc == RT_OK) rc = rt_get_timing(ctx, &tm);   // (drains the frame's own launches)
        if (rc == RT_OK && i == reps) rc = rt_readback(ctx, RT_BUF_LIGHTING_F32, before.data(), npix * 16u);
        auto t = std::chrono::steady_clock::now();
        if (rc == RT_OK) rc = rt_add_lights(ctx, &u, lights.data(), n);
        const double call = ms_since(t);
        if (rc == RT_OK) rc = rt_get_timing(ctx, &tm);
        if (i > 0) { device_ms += tm.shade_ms / reps; call_ms += call / reps; launches += tm.other_launches; }
    }
    if (rc == RT_OK) rc = rt_readback(ctx, RT_BUF_LIGHTING_F32, after.data(), npix * 16u);
    if (rc != RT_OK) { std::fprintf(stderr, "point lights failed (%d): %s\n", rc, rt_last_error(ctx)); delete p; return 1; }
    uint64_t lit = 0;
    for (size_t i = 0; i < npix; i++) lit += std::memcmp(&before[4u * i], &after[4u * i], 16) != 0;
    std::printf("{\"lights\": %u, \"frame\": \"%dx%d spp %d depth %d\", \"add_lights_device_ms\": %.4f, \"add_lights_call_ms\": %.4f, "
                "\"launches_per_call\": %.2f, \"pixels_lit\": %llu}\n",
                n, width, height, spp, depth, device_ms, call_ms, (double)launches / reps, (unsigned long long)lit);
    delete p;
    return 0;
}

// --shadows: see the head of the file
int run_shadows(rt::game::Game& game, const std::vector<uint8_t>& noise, int width, int height, int spp, int depth, int device, uint32_t n,
                bool as_models, float scale) {
    std::string err;
    RtConfig cfg = make_config(width, height, spp, depth, device, 0, 1, RT_FLAG_CACHE_PRIMARY | RT_FLAG_TIMING_ALL);
    rt::render::Pipeline* p = rt::render::create_instance(cfg, noise.data(), game, &err);
    if (!p) { std::fprintf(stderr, "create_instance failed: %s\n", err.c_str()); return 1; }
    RtContext* ctx = p->context();
    if (p->draw_frame(game) != RT_OK || p->wait() != RT_OK) { std::fprintf(stderr, "frame failed: %s\n", p->last_error()); delete p; return 1; }
    const RtUniforms u = p->uniforms();
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (float)((x >> 40) * (1.0 / 16777216.0)); };   // [0, 1)
    // the stamp of --models: a third solid, the rest air and absent in turn
    const int32_t E[3] = {9, 9, 12};
    std::vector<uint32_t> mats((size_t)E[0] * E[1] * E[2]);
    std::vector<uint8_t> state(mats.size());
    for (size_t i = 0; i < mats.size(); i++) {
        state[i] = rnd() < 0.3333f ? RT_STAMP_SOLID : (i & 1u ? RT_STAMP_AIR : RT_STAMP_ABSENT);
        mats[i] = (1u << 15) | ((40u + (uint32_t)i % 80u) << 14) | ((30u + (uint32_t)i % 90u) << 7) | (20u + (uint32_t)i % 100u);
    }
    uint32_t id = 0;
    if (as_models && p->stamp_create(E, mats.data(), state.data(), &id) != RT_OK) { std::fprintf(stderr, "stamp_create failed: %s\n", p->last_error()); delete p; return 1; }
    static const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    // where the occluders stand: what random pixels show, 0.5 to 6 units above it (30 units along the ray where the pixel shows sky)
    std::vector<int32_t> xy(2u * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        xy[2u * i] = std::min(width - 1, (int)(rnd() * (float)width));
        xy[2u * i + 1] = std::min(height - 1, (int)(rnd() * (float)height));
    }
    std::vector<RtRayHit> hits(n);
    int rc = n ? rt_pick_pixels(ctx, &u, xy.data(), n, hits.data()) : RT_OK;
    std::vector<RtDrawBox> boxes(n);
    std::vector<RtDrawStamp> models(as_models ? n : 0u);
    const uint32_t nlights = std::min(n, 1024u);
    std::vector<RtPointLight> lights(nlights);
    for (uint32_t i = 0; i < n && rc == RT_OK; i++) {
        float c[3];
        if (hits[i].kind == RT_HIT_SOLID) {
            for (int a = 0; a < 3; a++) c[a] = hits[i].position[a];
            c[2] += 0.5f + 5.5f * rnd();
        } else {
            const float sx = ((float)xy[2u * i] / (float)width) * 2.0f - 1.0f, sy = ((float)xy[2u * i + 1] / (float)height) * 2.0f - 1.0f;
            float v[3], len = 0.0f;
            for (int a = 0; a < 3; a++) { v[a] = u.forward[a] + u.right[a] * sx + u.up[a] * sy; len += v[a] * v[a]; }
            len = std::sqrt(len);
            for (int a = 0; a < 3; a++) c[a] = u.origin[a] + v[a] / len * 30.0f;
        }
        RtDrawBox& b = boxes[i];
        b = RtDrawBox{};
        if (as_models) {
            RtDrawStamp& m = models[i];
            m = RtDrawStamp{};
            m.stamp = id; m.scale = scale; m.orient = (uint8_t)(i % 48u); m.emission = 0xFF000000u;
            for (int a = 0; a < 3; a++) {
                const float ext = (float)E[perms[m.orient >> 3][a]];
                m.origin[a] = c[a] - 0.5f * ext * scale;
                b.lo[a] = m.origin[a]; b.hi[a] = std::fma(ext, scale, m.origin[a]);
            }
        } else {
            for (int a = 0; a < 3; a++) { const float half = a == 2 ? 0.9f : 0.3f; b.lo[a] = c[a] - half; b.hi[a] = c[a] + half; }   // a player's box
        }
        b.material = (1u << 15) | ((40u + i % 80u) << 14) | ((30u + i % 90u) << 7) | (20u + i % 100u);
        b.emission = 0xFF000000u;
        if (i < nlights) {
            RtPointLight& l = lights[i];
            l = RtPointLight{};
            for (int a = 0; a < 3; a++) { l.position[a] = c[a]; l.color[a] = 20.0f; }
            l.radius = 8.0f;
        }
    }
    auto ms_since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    const size_t npix = (size_t)width * (size_t)height;
    std::vector<float> before(4u * npix), after(4u * npix);
    std::vector<RtProbeLight> face(6u * (size_t)n);
    for (RtProbeLight& f : face) { f = RtProbeLight{}; f.light[0] = f.light[1] = f.light[2] = 8.0f; }
    const int reps = 20;
    double device_ms[3] = {0.0, 0.0, 0.0}, call_ms = 0.0;   // 0: the shadows; the yardsticks: 1 rt_draw_boxes of the same boxes, 2 rt_add_lights of as many lights
    uint32_t launches = 0;
    for (int pass = 0; pass < 3 && rc == RT_OK; pass++) {
        for (int i = 0; i < reps + 1 && rc == RT_OK; i++) {   // (the first repetition warms the staging up)
            RtTiming tm{};
            rc = rt_draw_frame(ctx, &u);
            if (rc == RT_OK) rc = rt_sync(ctx);
            if (rc == RT_OK) rc = rt_get_timing(ctx, &tm);   // (drains the frame's own launches)
            if (rc == RT_OK && pass == 0 && i == reps) rc = rt_readback(ctx, RT_BUF_LIGHTING_F32, before.data(), npix * 16u);
            auto t = std::chrono::steady_clock::now();
            if (rc == RT_OK) {
                if (pass == 0) rc = rt_shadow_entities(ctx, &u, as_models ? nullptr : boxes.data(), as_models ? 0u : n, models.data(), as_models ? n : 0u, 1.0f);
                else if (pass == 1) rc = rt_draw_boxes(ctx, &u, boxes.data(), face.data(), n);
                else rc = rt_add_lights(ctx, &u, lights.data(), nlights);
            }
            const double call = ms_since(t);
            if (rc == RT_OK) rc = rt_get_timing(ctx, &tm);
            if (i > 0) { device_ms[pass] += tm.shade_ms / reps; if (pass == 0) { call_ms += call / reps; launches += tm.other_launches; } }
        }
        if (rc == RT_OK && pass == 0) rc = rt_readback(ctx, RT_BUF_LIGHTING_F32, after.data(), npix * 16u);
    }
    if (rc != RT_OK) { std::fprintf(stderr, "entity shadows failed (%d): %s\n", rc, rt_last_error(ctx)); delete p; return 1; }
    uint64_t changed = 0;
    for (size_t i = 0; i < npix; i++) changed += std::memcmp(&before[4u * i], &after[4u * i], 16) != 0;
    std::printf("{\"shadows\": %u, \"shadow_models\": %d, \"model_scale\": %g, \"frame\": \"%dx%d spp %d depth %d\", \"shadow_entities_device_ms\": %.4f, "
                "\"shadow_entities_call_ms\": %.4f, \"launches_per_call\": %.2f, \"draw_boxes_device_ms\": %.4f, \"add_lights_device_ms\": %.4f, "
                "\"add_lights_count\": %u, \"pixels_changed\": %llu}\n",
                n, as_models ? 1 : 0, (double)scale, width, height, spp, depth, device_ms[0], call_ms, (double)launches / reps, device_ms[1],
                device_ms[2], nlights, (unsigned long long)changed);
    delete p;
    return 0;
}

// --light-shadows: see the head of the file
int run_light_shadows(rt::game::Game& game, const std::vector<uint8_t>& noise, int width, int height, int spp, int depth, int device, uint32_t nlights,
                      uint32_t nboxes, uint32_t nmodels, float scale, float spread, bool far_away) {
    std::string err;
    RtConfig cfg = make_config(width, height, spp, depth, device, 0, 1, RT_FLAG_CACHE_PRIMARY | RT_FLAG_TIMING_ALL);
    rt::render::Pipeline* p = rt::render::create_instance(cfg, noise.data(), game, &err);
    if (!p) { std::fprintf(stderr, "create_instance failed: %s\n", err.c_str()); return 1; }
    RtContext* ctx = p->context();
    if (p->draw_frame(game) != RT_OK || p->wait() != RT_OK) { std::fprintf(stderr, "frame failed: %s\n", p->last_error()); delete p; return 1; }
    const RtUniforms u = p->uniforms();
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (float)((x >> 40) * (1.0 / 16777216.0)); };   // [0, 1)
    // the lights: --lights' own, so that the two runs light the same frame
    std::vector<int32_t> xy(2u * (size_t)nlights);
    for (uint32_t i = 0; i < nlights; i++) {
        xy[2u * i] = std::min(width - 1, (int)(rnd() * (float)width));
        xy[2u * i + 1] = std::min(height - 1, (int)(rnd() * (float)height));
    }
    std::vector<RtRayHit> hits(nlights);
    int rc = nlights ? rt_pick_pixels(ctx, &u, xy.data(), nlights, hits.data()) : RT_OK;
    std::vector<RtPointLight> lights(nlights);
    for (uint32_t i = 0; i < nlights && rc == RT_OK; i++) {
        RtPointLight& l = lights[i];
        l = RtPointLight{};
        const float off = 1.0f + 3.0f * rnd();
        if (hits[i].kind == RT_HIT_SOLID) {
            for (int a = 0; a < 3; a++) l.position[a] = hits[i].position[a];
            l.position[hits[i].normal / 2u] += hits[i].normal % 2u == 0u ? off : -off;
        } else {
            const float sx = ((float)xy[2u * i] / (float)width) * 2.0f - 1.0f, sy = ((float)xy[2u * i + 1] / (float)height) * 2.0f - 1.0f;
            float v[3], len = 0.0f;
            for (int a = 0; a < 3; a++) { v[a] = u.forward[a] + u.right[a] * sx + u.up[a] * sy; len += v[a] * v[a]; }
            len = std::sqrt(len);
            for (int a = 0; a < 3; a++) l.position[a] = u.origin[a] + v[a] / len * 30.0f;
        }
        l.radius = 8.0f;
        l.color[0] = 20.0f + 20.0f * rnd(); l.color[1] = 15.0f + 15.0f * rnd(); l.color[2] = 5.0f + 10.0f * rnd();
    }
    // the stamp of the models: a third solid, the rest air and absent in turn
    const int32_t E[3] = {5, 4, 6};
    std::vector<uint32_t> mats((size_t)E[0] * E[1] * E[2]);
    std::vector<uint8_t> state(mats.size());
    for (size_t i = 0; i < mats.size(); i++) {
        state[i] = rnd() < 0.3333f ? RT_STAMP_SOLID : (i & 1u ? RT_STAMP_AIR : RT_STAMP_ABSENT);
        mats[i] = (1u << 15) | ((40u + (uint32_t)i % 80u) << 14) | ((30u + (uint32_t)i % 90u) << 7) | (20u + (uint32_t)i % 100u);
    }
    uint32_t id = 0;
    if (nmodels && p->stamp_create(E, mats.data(), state.data(), &id) != RT_OK) { std::fprintf(stderr, "stamp_create failed: %s\n", p->last_error()); delete p; return 1; }
    static const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    // the occluders: each within `spread` units of a light, in turn — or 400 units above it, where no segment of the frame passes
    auto centre = [&](uint32_t i, float c[3]) {
        const RtPointLight& l = lights[i % std::max(nlights, 1u)];
        for (int a = 0; a < 3; a++) c[a] = (nlights ? l.position[a] : u.origin[a]) + spread * (2.0f * rnd() - 1.0f);
        if (far_away) c[2] += 400.0f;
    };
    std::vector<RtDrawBox> boxes(nboxes);
    for (uint32_t i = 0; i < nboxes; i++) {
        float c[3];
        centre(i, c);
        RtDrawBox& b = boxes[i];
        b = RtDrawBox{};
        for (int a = 0; a < 3; a++) { const float half = a == 2 ? 0.9f : 0.3f; b.lo[a] = c[a] - half; b.hi[a] = c[a] + half; }   // a player's box
        b.emission = 0xFF000000u;
    }
    std::vector<RtDrawStamp> models(nmodels);
    for (uint32_t i = 0; i < nmodels; i++) {
        float c[3];
        centre(i + nboxes, c);
        RtDrawStamp& m = models[i];
        m = RtDrawStamp{};
        m.stamp = id; m.scale = scale; m.orient = (uint8_t)(i % 48u); m.emission = 0xFF000000u;
        for (int a = 0; a < 3; a++) m.origin[a] = c[a] - 0.5f * (float)E[perms[m.orient >> 3][a]] * scale;
    }
    auto ms_since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    const size_t npix = (size_t)width * (size_t)height;
    std::vector<float> plain(4u * npix), shaded(4u * npix);
    const int reps = 20;
    double device_ms[2] = {0.0, 0.0}, call_ms[2] = {0.0, 0.0};   // 0: rt_add_lights_occluded; the yardstick: 1 rt_add_lights of the same lights
    uint32_t launches = 0;
    for (int pass = 0; pass < 2 && rc == RT_OK; pass++) {
        for (int i = 0; i < reps + 1 && rc == RT_OK; i++) {   // (the first repetition warms the staging up)
            RtTiming tm{};
            rc = rt_draw_frame(ctx, &u);
            if (rc == RT_OK) rc = rt_sync(ctx);
            if (rc == RT_OK) rc = rt_get_timing(ctx, &tm);   // (drains the frame's own launches)
            auto t = std::chrono::steady_clock::now();
            if (rc == RT_OK)
                rc = pass == 0 ? rt_add_lights_occluded(ctx, &u, lights.data(), nlights, boxes.data(), nboxes, models.data(), nmodels)
                               : rt_add_lights(ctx, &u, lights.data(), nlights);
            const double call = ms_since(t);
            if (rc == RT_OK) rc = rt_get_timing(ctx, &tm);
            if (i > 0) { device_ms[pass] += tm.shade_ms / reps; call_ms[pass] += call / reps; if (pass == 0) launches += tm.other_launches; }
        }
        if (rc == RT_OK) rc = rt_readback(ctx, RT_BUF_LIGHTING_F32, (pass == 0 ? shaded : plain).data(), npix * 16u);
    }
    if (rc != RT_OK) { std::fprintf(stderr, "point-light shadows failed (%d): %s\n", rc, rt_last_error(ctx)); delete p; return 1; }
    uint64_t darker = 0;
    for (size_t i = 0; i < npix; i++) darker += std::memcmp(&plain[4u * i], &shaded[4u * i], 16) != 0;
    std::printf("{\"light_shadows\": %u, \"boxes\": %u, \"models\": %u, \"model_scale\": %g, \"spread\": %g, \"far\": %d, \"frame\": \"%dx%d spp %d depth %d\", "
                "\"add_lights_occluded_device_ms\": %.4f, \"add_lights_occluded_call_ms\": %.4f, \"launches_per_call\": %.2f, "
                "\"add_lights_device_ms\": %.4f, \"add_lights_call_ms\": %.4f, \"pixels_shadowed\": %llu}\n",
                nlights, nboxes, nmodels, (double)scale, (double)spread, far_away ? 1 : 0, width, height, spp, depth, device_ms[0], call_ms[0],
                (double)launches / reps, device_ms[1], call_ms[1], (unsigned long long)darker);
    delete p;
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    int width = 1024, height = 1024;   // WINDOW_WIDTH / WINDOW_HEIGHT, src/render/constants.rs:9-10
    int spp = 1, depth = 2, frames = 240, device = 0, gpus = 1;
    bool gather = false, overlap = false, post = false, accumulate = false, edit_spread = false;
    int edits = 0, edit_radius = 0;
    const char* edit_shape = nullptr;
    int edit_stamp = -1;
    long long entity_rays = 0;
    bool coherent = false;
    long long rays = 0, boxes = -1, lights = -1, models = -1, shadows = -1, particles = -1;
    float particle_half = 0.0625f, particle_near = 10.0f;
    int simulate = 0, step_sweeps = 3;
    bool shadow_models = false, light_shadows = false, occluders_far = false;
    float model_scale = 0.125f, occluder_spread = 3.0f;
    bool rays_coherent = false;
    bool reproject = false, stream = false, stream_history = false, history_denoise = false;
    float camera_step = 0.0f;
    int frames_in_flight = 1;      // 2: RT_FLAG_FRAMES_IN_FLIGHT_2 and no fence between frames (bench.py's default), one device
    std::string noise_path = "tests/golden/blue_noise_512.rgba";
    std::vector<const char*> positional = {argv[0]};
    for (int i = 1; i < argc; i++) {
        auto want = [&](const char* flag) { return std::strcmp(argv[i], flag) == 0 && i + 1 < argc; };
        if (want("--width")) width = std::atoi(argv[++i]);
        else if (want("--height")) height = std::atoi(argv[++i]);
        else if (want("--spp")) spp = std::atoi(argv[++i]);
        else if (want("--depth")) depth = std::atoi(argv[++i]);
        else if (want("--frames")) frames = std::atoi(argv[++i]);
        else if (want("--device")) device = std::atoi(argv[++i]);
        else if (want("--gpus")) gpus = std::atoi(argv[++i]);
        else if (want("--noise")) noise_path = argv[++i];
        else if (std::strcmp(argv[i], "--gather") == 0) gather = true;
        else if (std::strcmp(argv[i], "--overlap") == 0) overlap = true;
        else if (std::strcmp(argv[i], "--post") == 0) post = true;
        else if (std::strcmp(argv[i], "--accumulate") == 0) accumulate = true;
        else if (std::strcmp(argv[i], "--reproject") == 0) reproject = accumulate = true;
        else if (std::strcmp(argv[i], "--history-denoise") == 0) history_denoise = true;
        else if (want("--camera-step")) camera_step = std::strtof(argv[++i], nullptr);
        else if (want("--frames-in-flight")) frames_in_flight = std::atoi(argv[++i]);
        else if (want("--edits")) edits = std::atoi(argv[++i]);
        else if (std::strcmp(argv[i], "--edit-spread") == 0) edit_spread = true;
        else if (want("--edit-radius")) edit_radius = std::atoi(argv[++i]);
        else if (want("--edit-shape")) edit_shape = argv[++i];
        else if (want("--edit-stamp")) edit_stamp = std::atoi(argv[++i]);
        else if (std::strcmp(argv[i], "--stream") == 0) stream = true;
        else if (std::strcmp(argv[i], "--stream-history") == 0) stream_history = true;
        else if (want("--rays")) rays = std::atoll(argv[++i]);
        else if (want("--entity-rays")) entity_rays = std::atoll(argv[++i]);
        else if (std::strcmp(argv[i], "--coherent") == 0) coherent = true;
        else if (std::strcmp(argv[i], "--rays-coherent") == 0) rays_coherent = true;
        else if (want("--boxes")) boxes = std::atoll(argv[++i]);
        else if (want("--lights")) lights = std::atoll(argv[++i]);
        else if (want("--particles")) particles = std::atoll(argv[++i]);
        else if (want("--particle-half")) particle_half = std::strtof(argv[++i], nullptr);
        else if (want("--particle-near")) particle_near = std::strtof(argv[++i], nullptr);
        else if (want("--simulate")) simulate = std::atoi(argv[++i]);
        else if (want("--sweeps")) step_sweeps = std::atoi(argv[++i]);
        else if (std::strcmp(argv[i], "--light-shadows") == 0) light_shadows = true;
        else if (want("--occluder-spread")) occluder_spread = std::strtof(argv[++i], nullptr);
        else if (std::strcmp(argv[i], "--occluders-far") == 0) occluders_far = true;
        else if (want("--models")) models = std::atoll(argv[++i]);
        else if (want("--shadows")) shadows = std::atoll(argv[++i]);
        else if (std::strcmp(argv[i], "--shadow-models") == 0) shadow_models = true;
        else if (want("--model-scale")) model_scale = std::strtof(argv[++i], nullptr);
        else positional.push_back(argv[i]);
    }
    if (gpus < 1 || frames < 1) { std::fprintf(stderr, "--gpus and --frames must be >= 1\n"); return 2; }
    if (edits < 0 || edits > (1 << 24)) { std::fprintf(stderr, "--edits must be in 0..2^24\n"); return 2; }
    if (edit_radius != 0 && (!reproject || (edits == 0 && !edit_shape && edit_stamp < 0 && !stream_history))) { std::fprintf(stderr, "--edit-radius goes with --reproject and --edits N or --stream-history\n"); return 2; }
    if (stream && gpus > 1) { std::fprintf(stderr, "--stream needs one device\n"); return 2; }
    if (stream_history && (!stream || !reproject || edit_radius == 0)) { std::fprintf(stderr, "--stream-history goes with --stream --reproject --edit-radius N\n"); return 2; }
    if (rays < 0 || rays > (1ll << 26)) { std::fprintf(stderr, "--rays must be in 0..2^26\n"); return 2; }
    if (entity_rays < 0 || entity_rays > (1ll << 24)) { std::fprintf(stderr, "--entity-rays must be in 0..2^24\n"); return 2; }
    if (boxes < -1 || boxes > 4096) { std::fprintf(stderr, "--boxes must be in 0..4096\n"); return 2; }
    if (simulate < 0 || simulate > 100000 || step_sweeps < 1 || step_sweeps > 4 || (simulate > 0 && (particles < 0 || particle_half > 4.0f))) {
        std::fprintf(stderr, "--simulate must be in 0..100000 and goes with --particles (--particle-half at most 4), --sweeps in 1..4\n");
        return 2;
    }
    if (models < -1 || models > 4096 || !(model_scale >= 1.0f / 256.0f && model_scale <= 64.0f)) {
        std::fprintf(stderr, "--models must be in 0..4096, --model-scale in 2^-8..64\n");
        return 2;
    }
    if (particles < -1 || particles > (1ll << 20) || !(particle_half > 0.0f && particle_half <= 4096.0f) || !(particle_near > 0.0f && particle_near <= 65536.0f)) {
        std::fprintf(stderr, "--particles must be in 0..2^20, --particle-half in (0, 4096], --particle-near in (0, 65536]\n");
        return 2;
    }
    if (shadows < -1 || shadows > 4096) { std::fprintf(stderr, "--shadows must be in 0..4096\n"); return 2; }
    if (lights < -1 || lights > 1024) { std::fprintf(stderr, "--lights must be in 0..1024\n"); return 2; }
    if (!(occluder_spread >= 0.0f && occluder_spread <= 1024.0f)) { std::fprintf(stderr, "--occluder-spread must be in 0..1024\n"); return 2; }
    if (frames_in_flight != 1 && (frames_in_flight != 2 || gpus > 1)) { std::fprintf(stderr, "--frames-in-flight is 1, or 2 on one device\n"); return 2; }
    if ((reproject || camera_step != 0.0f) && gpus > 1) { std::fprintf(stderr, "--reproject and --camera-step need one device\n"); return 2; }
    if (gpus > 1) gather = true;
    if (history_denoise && (!post || !reproject)) { std::fprintf(stderr, "--history-denoise goes with --post --reproject\n"); return 2; }
    if (post && gpus > 1) { std::fprintf(stderr, "--post needs the whole frame on one device (gather first on several)\n"); return 2; }
    rt::game::Game game((int)positional.size(), positional.data());
    RtShapeEdit shape{};
    if (edit_shape && (edits > 0 || !shape_brush(edit_shape, game.camera.origin, &shape))) {
        std::fprintf(stderr, "--edit-shape is sphere:R (0..512) or box:E (1..256), without --edits\n");
        return 2;
    }

    if (edit_stamp != -1 && (edit_stamp < 1 || edit_stamp > 4096 || edits > 0 || edit_shape)) {
        std::fprintf(stderr, "--edit-stamp is 1..4096, without --edits and --edit-shape\n");
        return 2;
    }

    std::vector<uint8_t> noise(RT_NOISE_BYTES);
    FILE* fp = std::fopen(noise_path.c_str(), "rb");
    if (!fp || std::fread(noise.data(), 1, noise.size(), fp) != noise.size()) {
        std::fprintf(stderr, "cannot read the blue-noise table (512x512 RGBA8 raw) from %s\n", noise_path.c_str());
        return 2;
    }
    std::fclose(fp);

    std::printf("Creating renderer (and world.)\n");                 // main.rs:10
    auto t0 = std::chrono::steady_clock::now();
    game.generate_world(0x5EED);
    if (light_shadows)
        return run_light_shadows(game, noise, width, height, spp, depth, device, (uint32_t)(lights < 0 ? 64 : lights), (uint32_t)(boxes < 0 ? 0 : boxes),
                                 (uint32_t)(models < 0 ? 0 : models), model_scale, occluder_spread, occluders_far);
    if (entity_rays > 0)
        return run_entity_rays(game, noise, width, height, spp, depth, device, (uint32_t)entity_rays, (uint32_t)(boxes < 0 ? 0 : boxes),
                               (uint32_t)(models < 0 ? 0 : models), model_scale, coherent);
    if (rays > 0) return run_rays(game, noise, width, height, spp, depth, device, (uint32_t)rays, rays_coherent);
    if (particles >= 0 && simulate > 0)
        return run_simulate(game, noise, width, height, spp, depth, device, (uint32_t)particles, particle_half, particle_near, simulate, (uint32_t)step_sweeps);
    if (particles >= 0) return run_particles(game, noise, width, height, spp, depth, device, (uint32_t)particles, particle_half, particle_near);
    if (boxes >= 0) return run_boxes(game, noise, width, height, spp, depth, device, (uint32_t)boxes);
    if (models >= 0) return run_models(game, noise, width, height, spp, depth, device, (uint32_t)models, model_scale);
    if (shadows >= 0) return run_shadows(game, noise, width, height, spp, depth, device, (uint32_t)shadows, shadow_models, model_scale);
    if (lights >= 0) return run_lights(game, noise, width, height, spp, depth, device, (uint32_t)lights);
    std::string err;

    // exact ray count of one frame (a counting context, outside the timed loop): the JSON line's Mrays/s is rays actually traced
    unsigned long long rays_per_frame = 0;
    {
        RtConfig ccfg = make_config(width, height, spp, depth, device, 0, 1, RT_FLAG_CACHE_PRIMARY | RT_FLAG_COUNTERS);
        rt::render::Pipeline* cp = rt::render::create_instance(ccfg, noise.data(), game, &err);
        if (!cp) { std::fprintf(stderr, "create_instance failed: %s\n", err.c_str()); return 1; }
        RtCounters cn{};
        if (cp->draw_frame(game) != RT_OK || cp->wait() != RT_OK || rt_get_counters(cp->context(), &cn) != RT_OK) {
            std::fprintf(stderr, "counting frame failed: %s\n", cp->last_error());
            delete cp;
            return 1;
        }
        rays_per_frame = cn.rays;
        delete cp;
    }

    std::vector<rt::render::Pipeline*> pipes((size_t)gpus, nullptr);
    std::vector<void*> comms((size_t)gpus, nullptr);
    std::vector<int> devices((size_t)gpus);
    for (int g = 0; g < gpus; g++) devices[(size_t)g] = device + g;
    for (int g = 0; g < gpus; g++) {
        RtConfig cfg = make_config(width, height, spp, depth, devices[(size_t)g], g, gpus, RT_FLAG_CACHE_PRIMARY | (accumulate ? RT_FLAG_ACCUMULATE : 0u) |
                                                                                                       (reproject ? RT_FLAG_REPROJECT : 0u) |
                                                                                                       (frames_in_flight == 2 ? RT_FLAG_FRAMES_IN_FLIGHT_2 : 0u));
        cfg.edit_radius = edit_radius;
        cfg.stream_history = stream_history ? 1 : 0;
        pipes[(size_t)g] = rt::render::create_instance(cfg, noise.data(), game, &err);
        if (!pipes[(size_t)g]) {
            std::fprintf(stderr, "create_instance failed on device %d: %s\n", devices[(size_t)g], err.c_str());
            return 1;
        }
        pipes[(size_t)g]->set_frames_in_flight(frames_in_flight);
        if (stream) pipes[(size_t)g]->enable_terrain_streaming(0x5EED, "", true);   // (the seed of game.generate_world above)
    }
    if (post && pipes[0]->enable_post_passes(true) != RT_OK) { std::fprintf(stderr, "enable_post_passes failed\n"); return 1; }
    if (history_denoise) {   // the measured preset (raytrace_amd.render.HISTORY_DENOISE_PRESET), the reference's bindings
        RtDenoiseParams dp{};
        dp.struct_size = sizeof(dp);
        dp.faithful = 1;
        const uint32_t settle[6] = {0, 16, 8, 4, 4, 2};
        for (int i = 0; i < 6; i++) dp.settle[i] = settle[i];
        if (pipes[0]->enable_history_denoise(dp) != RT_OK) { std::fprintf(stderr, "enable_history_denoise failed\n"); return 1; }
    }
    if (gather) {
        int rc = rt_comm_init_all(gpus, devices.data(), comms.data());
        if (rc != RT_OK) { std::fprintf(stderr, "rt_comm_init_all failed (%d): %s\n", rc, rt_last_error(nullptr)); return 1; }
    }
    std::printf("Created in %fs.\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());   // main.rs:13

    std::vector<std::vector<RtVoxelEdit>> brushes((size_t)gpus, edit_brush(edits, edit_spread, game.camera.origin));
    std::vector<std::vector<RtStampPlace>> stamp_places((size_t)gpus, stamp_brush(edit_stamp > 0 ? edit_stamp : 0, game.camera.origin));
    std::vector<uint32_t> stamp_ids(2 * (size_t)gpus, 0u);
    for (int g = 0; g < gpus && edit_stamp > 0; g++)
        if (!stamp_brush_create(pipes[(size_t)g], &stamp_ids[2 * (size_t)g])) {
            std::fprintf(stderr, "rt_stamp_create failed on device %d: %s\n", devices[(size_t)g], pipes[(size_t)g]->last_error());
            return 1;
        }
    RingBufferAverage perf(120);                                      // main.rs:16
    ThreadBarrier frame_barrier(gpus);
    std::atomic<int> failed{0};
    double total_ms = 0.0;
    // one host thread per device; thread 0 keeps the reference's frame-time statistics (main.rs:42-47)
    auto worker = [&](int g) {
        rt::render::Pipeline* p = pipes[(size_t)g];
        auto frame_timer = std::chrono::steady_clock::now();
        const auto loop_start = frame_timer;
        for (int f = 0; f < frames; f++) {
            if (g == 0) {
                auto now = std::chrono::steady_clock::now();
                double millis = std::chrono::duration<double, std::milli>(now - frame_timer).count();
                frame_timer = now;
                if (f > 0) perf.push_sample(millis);
            }
            int rc = RT_OK;
            if (camera_step != 0.0f && f > 0) {   // (one device: this thread is the only one that reads the camera)
                game.camera.origin[0] += camera_step;
                game.camera.heading += camera_step / 100.0f;
            }
            if (edits > 0) {
                set_solid(brushes[(size_t)g], f);
                rc = rt_edit_voxels(p->context(), brushes[(size_t)g].data(), (uint32_t)edits);
                if (rc != RT_OK) std::fprintf(stderr, "rt_edit_voxels failed on device %d (%d): %s\n", devices[(size_t)g], rc, rt_last_error(p->context()));
            }
            if (edit_shape) {
                RtShapeEdit sh = shape;
                sh.solid = (uint8_t)((f & 1) == 0);
                rc = p->edit_shapes(&sh, 1);
                if (rc != RT_OK) std::fprintf(stderr, "rt_edit_shapes failed on device %d (%d): %s\n", devices[(size_t)g], rc, rt_last_error(p->context()));
            }
            if (edit_stamp > 0) {
                set_stamp(stamp_places[(size_t)g], &stamp_ids[2 * (size_t)g], f);
                rc = p->edit_stamps(stamp_places[(size_t)g].data(), (uint32_t)edit_stamp);
                if (rc != RT_OK) std::fprintf(stderr, "rt_edit_stamps failed on device %d (%d): %s\n", devices[(size_t)g], rc, rt_last_error(p->context()));
            }
            if (rc == RT_OK) rc = p->draw_frame(game);                // main.rs:52
            if (rc != RT_OK) {
                std::fprintf(stderr, "frame %d failed on device %d (%d): %s\n", f, devices[(size_t)g], rc, p->last_error());
                failed.store(1);
            }
            if (gpus > 1) {
                // either every rank posts the frame's send/recv or none does: a rank that posted alone would wait for its peers for ever
                frame_barrier.arrive_and_wait();
                if (failed.load()) break;
            } else if (rc != RT_OK) break;
            if (gather) {
                rc = rt_gather_gbuffer(p->context(), comms[(size_t)g], 0, nullptr, overlap ? 1 : 0);
                if (rc != RT_OK) {
                    // the peers have posted theirs already and cannot be recalled: leave without waiting for them
                    std::fprintf(stderr, "gather of frame %d failed on device %d (%d): %s\n", f, devices[(size_t)g], rc, p->last_error());
                    std::fflush(nullptr);
                    if (gpus > 1) std::_Exit(1);
                    failed.store(1);
                    break;
                }
            }
        }
        if (failed.load()) return;     // nothing is waited for on the failure path: queued collectives may have no peer
        if (rt_sync(p->context()) != RT_OK) failed.store(1);
        if (g == 0) total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - loop_start).count();
    };
    std::vector<std::thread> threads;
    for (int g = 1; g < gpus; g++) threads.emplace_back(worker, g);
    worker(0);
    for (auto& t : threads) t.join();

    int exit_code = failed.load() ? 1 : 0;
    // --edits: the edit batches alone, on a pipeline whose launches are timed
    double edit_dev_ms = 0.0, edit_host_ms = 0.0, edit_wall_ms = 0.0, edit_launches = 0.0;
    if (!exit_code && (edits > 0 || edit_shape || edit_stamp > 0)) {
        RtConfig tcfg = make_config(width, height, spp, depth, device, 0, 1, RT_FLAG_CACHE_PRIMARY | RT_FLAG_TIMING_ALL);
        rt::render::Pipeline* tp = rt::render::create_instance(tcfg, noise.data(), game, &err);
        RtTiming tm{};
        if (!tp || tp->draw_frame(game) != RT_OK || tp->wait() != RT_OK || rt_get_timing(tp->context(), &tm) != RT_OK) {
            std::fprintf(stderr, "edit timing pipeline failed: %s\n", tp ? tp->last_error() : err.c_str());
            exit_code = 1;
        } else {
            std::vector<RtVoxelEdit> brush = edit_brush(edits, edit_spread, game.camera.origin);
            std::vector<RtStampPlace> places = stamp_brush(edit_stamp > 0 ? edit_stamp : 0, game.camera.origin);
            uint32_t ids[2] = {0, 0};
            if (edit_stamp > 0 && !stamp_brush_create(tp, ids)) exit_code = 1;
            const auto w0 = std::chrono::steady_clock::now();
            for (int f = 0; f < frames && !exit_code; f++) {
                set_solid(brush, f);
                RtShapeEdit sh = shape;
                sh.solid = (uint8_t)((f & 1) == 0);
                const auto h0 = std::chrono::steady_clock::now();
                set_stamp(places, ids, f);
                if ((edit_stamp > 0 ? tp->edit_stamps(places.data(), (uint32_t)edit_stamp)
                     : edit_shape ? tp->edit_shapes(&sh, 1) : rt_edit_voxels(tp->context(), brush.data(), (uint32_t)edits)) != RT_OK) exit_code = 1;
                edit_host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
            }
            if (rt_sync(tp->context()) != RT_OK) exit_code = 1;
            edit_wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count() / frames;
            if (rt_get_timing(tp->context(), &tm) != RT_OK) exit_code = 1;
            edit_dev_ms = tm.shade_ms / frames;
            edit_launches = (double)tm.other_launches / frames;
            edit_host_ms /= frames;
            if (exit_code) std::fprintf(stderr, "edit timing failed: %s\n", rt_last_error(tp->context()));
        }
        delete tp;
    }
    if (exit_code && gpus > 1) { std::fflush(nullptr); std::_Exit(1); }   // communicators may hold unmatched operations: no orderly teardown
    if (!exit_code) {
        std::printf("%.3fms / %.3fms\n", perf.average(), perf.max());    // main.rs:45-46: average / max
        // a checksum of the assembled frame's depth plane shows that the gather delivered pixels (0 without --gather)
        unsigned long long checksum = 0;
        if (gather) {
            std::vector<uint16_t> depth_plane((size_t)width * height);
            if (rt_frame_readback(pipes[0]->context(), RT_BUF_DEPTH_R16UI, depth_plane.data(), depth_plane.size() * 2) == RT_OK)
                for (uint16_t v : depth_plane) checksum += v;
            else { std::fprintf(stderr, "rt_frame_readback failed: %s\n", pipes[0]->last_error()); exit_code = 1; }
        }
        unsigned long long final_checksum = 0;   // --post: sum over the swapchain image's bytes (0 without)
        if (post) {
            std::vector<uint8_t> final_plane((size_t)width * height * 4);
            if (rt_readback(pipes[0]->context(), RT_BUF_FINAL_BGRA8, final_plane.data(), final_plane.size()) == RT_OK)
                for (uint8_t v : final_plane) final_checksum += v;
            else { std::fprintf(stderr, "rt_readback(final) failed: %s\n", pipes[0]->last_error()); exit_code = 1; }
        }
        uint32_t acc_frames = 0, acc_samples = 0;   // what the last frame's lighting holds (spp without --accumulate)
        if (rt_get_accumulation(pipes[0]->context(), &acc_frames, &acc_samples) != RT_OK) exit_code = 1;
        const double ms = total_ms / frames;
        std::printf("{\"binary\": \"rt_bench\", \"config\": {\"width\": %d, \"height\": %d, \"spp\": %d, \"depth\": %d, \"gpus\": %d, "
                    "\"gather\": \"%s\", \"post_passes\": %s, \"pose\": [%g, %g, %g, %g, %g], \"sun_angle\": %g}, \"frames\": %d, \"rays_per_frame\": %llu, "
                    "\"ms_per_frame\": %.4f, \"avg_ms_last_120\": %.4f, \"max_ms_last_120\": %.4f, \"mrays_per_s\": %.2f, "
                    "\"depth_plane_checksum\": %llu, \"final_image_checksum\": %llu, \"accumulate\": %s, \"reproject\": %s, \"camera_step\": %g, \"samples\": %u, \"acc_frames\": %u, \"edit_radius\": %d, \"stream\": %s, \"stream_history\": %s, "
                    "\"edits\": %d, \"edit_spread\": %s, \"edit_device_ms_per_call\": %.4f, \"edit_launches_per_call\": %.1f, "
                    "\"edit_host_ms_per_call\": %.4f, \"edit_wall_ms_per_call\": %.4f%s%s%s%s%s}\n",
                    width, height, spp, depth, gpus, gather ? (overlap ? "rccl-overlapped" : "rccl-serial") : "none", post ? "true" : "false",
                    game.camera.origin[0], game.camera.origin[1], game.camera.origin[2], game.camera.heading, game.camera.pitch,
                    game.sun_angle, frames, rays_per_frame, ms, perf.average(), perf.max(), (double)rays_per_frame / (ms * 1e3), checksum, final_checksum,
                    accumulate ? "true" : "false", reproject ? "true" : "false", (double)camera_step, acc_samples, acc_frames, edit_radius, stream ? "true" : "false", stream_history ? "true" : "false", edits, edit_spread ? "true" : "false", edit_dev_ms, edit_launches,
                    edit_host_ms, edit_wall_ms, history_denoise ? ", \"history_denoise\": true" : "", edit_shape ? ", \"edit_shape\": \"" : "",
                    edit_shape ? edit_shape : "", edit_shape ? "\"" : "", edit_stamp > 0 ? (", \"edit_stamp\": " + std::to_string(edit_stamp)).c_str() : "");
    }
    for (int g = 0; g < gpus; g++) {
        if (comms[(size_t)g]) rt_comm_destroy(comms[(size_t)g]);
        delete pipes[(size_t)g];
    }
    return exit_code;
}
