// rt_bench — headless counterpart of the reference's interactive binary (src/bin/main.rs:8-57): builds the Game
// (six optional positional floats `x y z heading pitch sun_angle`, src/game/mod.rs:45-52), creates the renderer, then
// loops draw_frame and prints the rolling average / maximum frame time of the last 120 frames
// (RingBufferAverage, src/util.rs:175-221; printout main.rs:42-47) — followed by ONE JSON line with the metrics SURVEY.md 5
// asks of the bench binary (config, rays, ms, Mrays/s).  This file: the options, the dispatch and the frame loop; the modes that run
// instead of the frame loop are in bench_modes.cpp (each described at its function), their records in bench_scene.hpp, the session
// and the timing helpers in bench_run.hpp.
//
//   rt_bench [x y z heading pitch sun] [--width W] [--height H] [--spp N] [--depth D] [--frames F]
//            [--noise tests/golden/blue_noise_512.rgba] [--device I] [--gpus N] [--gather] [--overlap] [--post] [--accumulate]
//            [--reproject [--history-denoise]] [--camera-step DX] [--frames-in-flight N] [--edits N [--edit-spread]] [--edit-radius N]
//            [--edit-shape sphere:R|box:E]
//            [--stream [--stream-history]]
//            [--rays N [--rays-coherent]]
//            [--boxes N]
//            [--particles N [--particle-half H] [--particle-near D] [--simulate T [--sweeps S]]]
//            [--debris RADIUS [--density D] [--settle T [--fall K]]] [--collapse RADIUS]
//            [--navigate EXTENT [--agents N]] [--flood EXTENT [--ticks K]]
//            [--entity-rays N [--coherent] [--boxes B] [--models M] [--model-scale S]]
//            [--entity-sweeps N [--coherent] [--boxes B] [--models M] [--model-scale S]]
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
// Instead of the frame loop, in this order of precedence: --light-shadows, --entity-rays N, --entity-sweeps N, --rays N, --particles N --simulate T,
// --debris RADIUS [--settle T [--fall K]], --collapse RADIUS, --navigate EXTENT [--agents N], --flood EXTENT [--ticks K], --particles N, --boxes N, --models N, --shadows N, --lights N (bench_modes.cpp).
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <thread>

#include "bench_run.hpp"

namespace {

using namespace bench;

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
std::vector<RtVoxelEdit> edit_brush(int n, bool spread, const int c[3]) {
    const int R = RT_ROOT_BLOCK_SIZE;
    std::vector<RtVoxelEdit> v((size_t)n);
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
        e.solid = 1; e.material = BRUSH_MATERIAL; e.reserved = 0;
    }
    return v;
}

// --edit-shape: "sphere:R" or "box:E" at the brush's centre; false when the text is neither
bool shape_brush(const char* text, const int c[3], RtShapeEdit* out) {
    const int R = RT_ROOT_BLOCK_SIZE;
    RtShapeEdit s{};
    s.material = BRUSH_MATERIAL;
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
    std::vector<uint32_t> mats(5 * 5 * 7, BRUSH_MATERIAL);
    std::vector<uint8_t> hut(5 * 5 * 7), air(5 * 5 * 7, RT_STAMP_AIR);
    for (int z = 0; z < 7; z++)
        for (int y = 0; y < 5; y++)
            for (int x = 0; x < 5; x++) {
                const bool edge_x = x == 0 || x == 4, edge_y = y == 0 || y == 4;
                hut[(size_t)(z * 5 + y) * 5 + x] = (edge_x && edge_y && z > 4) ? RT_STAMP_ABSENT : (edge_x || edge_y || z == 0 || z >= 5) ? RT_STAMP_SOLID : RT_STAMP_AIR;
            }
    return p->stamp_create(ext, mats.data(), hut.data(), &ids[0]) == RT_OK && p->stamp_create(ext, mats.data(), air.data(), &ids[1]) == RT_OK;
}
std::vector<RtStampPlace> stamp_brush(int n, const int c[3]) {
    const int R = RT_ROOT_BLOCK_SIZE;
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

// What --edits, --edit-shape or --edit-stamp does before every frame, for one pipeline (the options allow one of the three at a time).
struct FrameEdit {
    const char* call = nullptr;          // the C-ABI call behind it, for messages; nullptr: no edit
    std::vector<RtVoxelEdit> voxels;
    RtShapeEdit shape{};
    std::vector<RtStampPlace> places;
    uint32_t stamp_ids[2] = {0, 0};      // stamp_brush_create's, of the pipeline the edit goes to
};
FrameEdit frame_edit(const Options& o, const RtShapeEdit& shape, const float origin[3]) {
    int c[3];
    brush_centre(origin, c);
    FrameEdit e;
    e.call = o.edits > 0 ? "rt_edit_voxels" : o.edit_shape ? "rt_edit_shapes" : o.edit_stamp > 0 ? "rt_edit_stamps" : nullptr;
    e.voxels = edit_brush(o.edits, o.edit_spread, c);
    e.shape = shape;
    e.places = stamp_brush(o.edit_stamp > 0 ? o.edit_stamp : 0, c);
    return e;
}
// frame f's edit: placed or filled on even frames, taken away on odd ones; *host_ms gains the time spent in the call (with the
// choice of the stamp)
int apply_edit(rt::render::Pipeline* p, FrameEdit& e, int f, double* host_ms) {
    for (RtVoxelEdit& v : e.voxels) v.solid = (uint16_t)((f & 1) == 0);
    RtShapeEdit sh = e.shape;
    sh.solid = (uint8_t)((f & 1) == 0);
    const auto h0 = std::chrono::steady_clock::now();
    for (RtStampPlace& s : e.places) s.stamp = e.stamp_ids[f & 1];
    const int rc = !e.places.empty() ? p->edit_stamps(e.places.data(), (uint32_t)e.places.size())
                   : !e.voxels.empty() ? rt_edit_voxels(p->context(), e.voxels.data(), (uint32_t)e.voxels.size()) : p->edit_shapes(&sh, 1);
    *host_ms += ms_since(h0);
    return rc;
}

// fills `o` and the positional arguments; 2 (after the message) when an option is out of its range
int parse_options(int argc, char** argv, Options& o, std::vector<const char*>& positional) {
    for (int i = 1; i < argc; i++) {
        auto want = [&](const char* flag) { return std::strcmp(argv[i], flag) == 0 && i + 1 < argc; };
        auto is = [&](const char* flag) { return std::strcmp(argv[i], flag) == 0; };
        if (want("--width")) o.width = std::atoi(argv[++i]);
        else if (want("--height")) o.height = std::atoi(argv[++i]);
        else if (want("--spp")) o.spp = std::atoi(argv[++i]);
        else if (want("--depth")) o.depth = std::atoi(argv[++i]);
        else if (want("--frames")) o.frames = std::atoi(argv[++i]);
        else if (want("--device")) o.device = std::atoi(argv[++i]);
        else if (want("--gpus")) o.gpus = std::atoi(argv[++i]);
        else if (want("--noise")) o.noise_path = argv[++i];
        else if (is("--gather")) o.gather = true;
        else if (is("--overlap")) o.overlap = true;
        else if (is("--post")) o.post = true;
        else if (is("--accumulate")) o.accumulate = true;
        else if (is("--reproject")) o.reproject = o.accumulate = true;
        else if (is("--history-denoise")) o.history_denoise = true;
        else if (want("--camera-step")) o.camera_step = std::strtof(argv[++i], nullptr);
        else if (want("--frames-in-flight")) o.frames_in_flight = std::atoi(argv[++i]);
        else if (want("--edits")) o.edits = std::atoi(argv[++i]);
        else if (is("--edit-spread")) o.edit_spread = true;
        else if (want("--edit-radius")) o.edit_radius = std::atoi(argv[++i]);
        else if (want("--edit-shape")) o.edit_shape = argv[++i];
        else if (want("--edit-stamp")) o.edit_stamp = std::atoi(argv[++i]);
        else if (is("--stream")) o.stream = true;
        else if (is("--stream-history")) o.stream_history = true;
        else if (want("--rays")) o.rays = std::atoll(argv[++i]);
        else if (want("--entity-rays")) o.entity_rays = std::atoll(argv[++i]);
        else if (want("--entity-sweeps")) o.entity_sweeps = std::atoll(argv[++i]);
        else if (is("--coherent")) o.coherent = true;
        else if (is("--rays-coherent")) o.rays_coherent = true;
        else if (want("--boxes")) o.boxes = std::atoll(argv[++i]);
        else if (want("--lights")) o.lights = std::atoll(argv[++i]);
        else if (want("--particles")) o.particles = std::atoll(argv[++i]);
        else if (want("--particle-half")) o.particle_half = std::strtof(argv[++i], nullptr);
        else if (want("--particle-near")) o.particle_near = std::strtof(argv[++i], nullptr);
        else if (want("--simulate")) o.simulate = std::atoi(argv[++i]);
        else if (want("--sweeps")) o.step_sweeps = std::atoi(argv[++i]);
        else if (want("--debris")) o.debris = std::atoi(argv[++i]);
        else if (want("--density")) o.debris_density = std::atoi(argv[++i]);
        else if (want("--settle")) o.settle = std::atoi(argv[++i]);
        else if (want("--fall")) o.fall = std::atoll(argv[++i]);
        else if (want("--collapse")) o.collapse = std::atoi(argv[++i]);
        else if (want("--navigate")) o.navigate = std::atoi(argv[++i]);
        else if (want("--agents")) o.agents = std::atoll(argv[++i]);
        else if (want("--flood")) o.flood = std::atoi(argv[++i]);
        else if (want("--ticks")) o.flood_ticks = std::atoi(argv[++i]);
        else if (is("--light-shadows")) o.light_shadows = true;
        else if (want("--occluder-spread")) o.occluder_spread = std::strtof(argv[++i], nullptr);
        else if (is("--occluders-far")) o.occluders_far = true;
        else if (want("--models")) o.models = std::atoll(argv[++i]);
        else if (want("--shadows")) o.shadows = std::atoll(argv[++i]);
        else if (is("--shadow-models")) o.shadow_models = true;
        else if (want("--model-scale")) o.model_scale = std::strtof(argv[++i], nullptr);
        else positional.push_back(argv[i]);
    }
    auto bad = [](const char* message) { std::fprintf(stderr, "%s\n", message); return 2; };
    if (o.gpus < 1 || o.frames < 1) return bad("--gpus and --frames must be >= 1");
    if (o.edits < 0 || o.edits > (1 << 24)) return bad("--edits must be in 0..2^24");
    if (o.edit_radius != 0 && (!o.reproject || (o.edits == 0 && !o.edit_shape && o.edit_stamp < 0 && !o.stream_history)))
        return bad("--edit-radius goes with --reproject and --edits N or --stream-history");
    if (o.stream && o.gpus > 1) return bad("--stream needs one device");
    if (o.stream_history && (!o.stream || !o.reproject || o.edit_radius == 0)) return bad("--stream-history goes with --stream --reproject --edit-radius N");
    if (o.rays < 0 || o.rays > (1ll << 26)) return bad("--rays must be in 0..2^26");
    if (o.entity_rays < 0 || o.entity_rays > (1ll << 24)) return bad("--entity-rays must be in 0..2^24");
    if (o.entity_sweeps < 0 || o.entity_sweeps > (1ll << 24)) return bad("--entity-sweeps must be in 0..2^24");
    if (o.boxes < -1 || o.boxes > 4096) return bad("--boxes must be in 0..4096");
    if (o.simulate < 0 || o.simulate > 100000 || o.step_sweeps < 1 || o.step_sweeps > 4 || (o.simulate > 0 && (o.particles < 0 || o.particle_half > 4.0f)))
        return bad("--simulate must be in 0..100000 and goes with --particles (--particle-half at most 4), --sweeps in 1..4");
    if (o.models < -1 || o.models > 4096 || !(o.model_scale >= 1.0f / 256.0f && o.model_scale <= 64.0f))
        return bad("--models must be in 0..4096, --model-scale in 2^-8..64");
    if (o.debris < 0 || o.debris > 127 || o.debris_density < 1 || o.debris_density > 256) return bad("--debris must be in 0..127, --density in 1..256");
    if (o.settle < 0 || o.settle > 100000 || (o.settle > 0 && o.debris == 0)) return bad("--settle must be in 0..100000 and goes with --debris");
    if (o.fall < 0 || o.fall > 0xFFFFFFFFll || (o.fall > 0 && o.settle == 0)) return bad("--fall must be in 1..4294967295 and goes with --debris RADIUS --settle T");
    if (o.collapse < 0 || o.collapse > 120 || (o.collapse > 0 && (o.collapse < 4 || o.debris > 0))) return bad("--collapse must be in 4..120, without --debris");
    if (o.navigate < 0 || o.navigate > 256 || (o.navigate > 0 && o.navigate < 16) || o.agents < 0 || o.agents > (1ll << 20) || (o.agents > 0 && o.navigate == 0))
        return bad("--navigate must be in 16..256, --agents in 0..2^20 and goes with --navigate");
    if (o.flood < 0 || o.flood > 256 || (o.flood > 0 && o.flood < 16) || o.flood_ticks < 0 || o.flood_ticks > 256 || (o.flood_ticks > 0 && o.flood == 0))
        return bad("--flood must be in 16..256, --ticks in 1..256 and goes with --flood");
    if (o.particles < -1 || o.particles > (1ll << 20) || !(o.particle_half > 0.0f && o.particle_half <= 4096.0f) ||
        !(o.particle_near > 0.0f && o.particle_near <= 65536.0f))
        return bad("--particles must be in 0..2^20, --particle-half in (0, 4096], --particle-near in (0, 65536]");
    if (o.shadows < -1 || o.shadows > 4096) return bad("--shadows must be in 0..4096");
    if (o.lights < -1 || o.lights > 1024) return bad("--lights must be in 0..1024");
    if (!(o.occluder_spread >= 0.0f && o.occluder_spread <= 1024.0f)) return bad("--occluder-spread must be in 0..1024");
    if (o.frames_in_flight != 1 && (o.frames_in_flight != 2 || o.gpus > 1)) return bad("--frames-in-flight is 1, or 2 on one device");
    if ((o.reproject || o.camera_step != 0.0f) && o.gpus > 1) return bad("--reproject and --camera-step need one device");
    if (o.gpus > 1) o.gather = true;
    if (o.history_denoise && (!o.post || !o.reproject)) return bad("--history-denoise goes with --post --reproject");
    if (o.post && o.gpus > 1) return bad("--post needs the whole frame on one device (gather first on several)");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    Options o;
    std::vector<const char*> positional = {argv[0]};
    if (parse_options(argc, argv, o, positional) != 0) return 2;
    rt::game::Game game((int)positional.size(), positional.data());
    int brush_at[3];
    brush_centre(game.camera.origin, brush_at);
    RtShapeEdit shape{};
    if (o.edit_shape && (o.edits > 0 || !shape_brush(o.edit_shape, brush_at, &shape))) {
        std::fprintf(stderr, "--edit-shape is sphere:R (0..512) or box:E (1..256), without --edits\n");
        return 2;
    }
    if (o.edit_stamp != -1 && (o.edit_stamp < 1 || o.edit_stamp > 4096 || o.edits > 0 || o.edit_shape)) {
        std::fprintf(stderr, "--edit-stamp is 1..4096, without --edits and --edit-shape\n");
        return 2;
    }

    std::vector<uint8_t> noise(RT_NOISE_BYTES);
    FILE* fp = std::fopen(o.noise_path.c_str(), "rb");
    if (!fp || std::fread(noise.data(), 1, noise.size(), fp) != noise.size()) {
        std::fprintf(stderr, "cannot read the blue-noise table (512x512 RGBA8 raw) from %s\n", o.noise_path.c_str());
        return 2;
    }
    std::fclose(fp);

    std::printf("Creating renderer (and world.)\n");                 // main.rs:10
    auto t0 = std::chrono::steady_clock::now();
    game.generate_world(0x5EED);
    const World world{game, noise};
    if (o.light_shadows) return run_light_shadows(o, world);
    if (o.entity_rays > 0) return run_entity_rays(o, world);
    if (o.entity_sweeps > 0) return run_entity_sweeps(o, world);
    if (o.rays > 0) return run_rays(o, world);
    if (o.particles >= 0 && o.simulate > 0) return run_simulate(o, world);
    if (o.collapse > 0) return run_collapse(o, world);
    if (o.navigate > 0) return run_navigate(o, world);
    if (o.flood > 0) return run_flood(o, world);
    if (o.debris > 0) return o.fall > 0 ? run_fall(o, world) : o.settle > 0 ? run_settle(o, world) : run_debris(o, world);
    if (o.particles >= 0) return run_particles(o, world);
    if (o.boxes >= 0) return run_boxes(o, world);
    if (o.models >= 0) return run_models(o, world);
    if (o.shadows >= 0) return run_shadows(o, world);
    if (o.lights >= 0) return run_lights(o, world);
    const int width = o.width, height = o.height, frames = o.frames, gpus = o.gpus;
    std::string err;

    // exact ray count of one frame (a counting context, outside the timed loop): the JSON line's Mrays/s is rays actually traced
    unsigned long long rays_per_frame = 0;
    {
        RtConfig ccfg = make_config(o, 0, 1, RT_FLAG_CACHE_PRIMARY | RT_FLAG_COUNTERS);
        const std::unique_ptr<rt::render::Pipeline> cp(rt::render::create_instance(ccfg, noise.data(), game, &err));
        if (!cp) { std::fprintf(stderr, "create_instance failed: %s\n", err.c_str()); return 1; }
        RtCounters cn{};
        if (cp->draw_frame(game) != RT_OK || cp->wait() != RT_OK || rt_get_counters(cp->context(), &cn) != RT_OK) {
            std::fprintf(stderr, "counting frame failed: %s\n", cp->last_error());
            return 1;
        }
        rays_per_frame = cn.rays;
    }

    std::vector<rt::render::Pipeline*> pipes((size_t)gpus, nullptr);
    std::vector<void*> comms((size_t)gpus, nullptr);
    std::vector<int> devices((size_t)gpus);
    for (int g = 0; g < gpus; g++) devices[(size_t)g] = o.device + g;
    for (int g = 0; g < gpus; g++) {
        RtConfig cfg = make_config(o, g, gpus, RT_FLAG_CACHE_PRIMARY | (o.accumulate ? RT_FLAG_ACCUMULATE : 0u) | (o.reproject ? RT_FLAG_REPROJECT : 0u) |
                                                   (o.frames_in_flight == 2 ? RT_FLAG_FRAMES_IN_FLIGHT_2 : 0u));
        cfg.edit_radius = o.edit_radius;
        cfg.stream_history = o.stream_history ? 1 : 0;
        pipes[(size_t)g] = rt::render::create_instance(cfg, noise.data(), game, &err);
        if (!pipes[(size_t)g]) {
            std::fprintf(stderr, "create_instance failed on device %d: %s\n", devices[(size_t)g], err.c_str());
            return 1;
        }
        pipes[(size_t)g]->set_frames_in_flight(o.frames_in_flight);
        if (o.stream) pipes[(size_t)g]->enable_terrain_streaming(0x5EED, "", true);   // (the seed of game.generate_world above)
    }
    if (o.post && pipes[0]->enable_post_passes(true) != RT_OK) { std::fprintf(stderr, "enable_post_passes failed\n"); return 1; }
    if (o.history_denoise) {   // the measured preset (raytrace_amd.render.HISTORY_DENOISE_PRESET), the reference's bindings
        RtDenoiseParams dp{};
        dp.struct_size = sizeof(dp);
        dp.faithful = 1;
        const uint32_t settle[6] = {0, 16, 8, 4, 4, 2};
        for (int i = 0; i < 6; i++) dp.settle[i] = settle[i];
        if (pipes[0]->enable_history_denoise(dp) != RT_OK) { std::fprintf(stderr, "enable_history_denoise failed\n"); return 1; }
    }
    if (o.gather) {
        int rc = rt_comm_init_all(gpus, devices.data(), comms.data());
        if (rc != RT_OK) { std::fprintf(stderr, "rt_comm_init_all failed (%d): %s\n", rc, rt_last_error(nullptr)); return 1; }
    }
    std::printf("Created in %fs.\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());   // main.rs:13

    std::vector<FrameEdit> edit((size_t)gpus, frame_edit(o, shape, game.camera.origin));
    for (int g = 0; g < gpus && o.edit_stamp > 0; g++)
        if (!stamp_brush_create(pipes[(size_t)g], edit[(size_t)g].stamp_ids)) {
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
        FrameEdit& mine = edit[(size_t)g];
        double edit_ms = 0.0;
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
            if (o.camera_step != 0.0f && f > 0) {   // (one device: this thread is the only one that reads the camera)
                game.camera.origin[0] += o.camera_step;
                game.camera.heading += o.camera_step / 100.0f;
            }
            if (mine.call) {
                rc = apply_edit(p, mine, f, &edit_ms);
                if (rc != RT_OK) std::fprintf(stderr, "%s failed on device %d (%d): %s\n", mine.call, devices[(size_t)g], rc, rt_last_error(p->context()));
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
            if (o.gather) {
                rc = rt_gather_gbuffer(p->context(), comms[(size_t)g], 0, nullptr, o.overlap ? 1 : 0);
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
    if (!exit_code && edit[0].call) {
        RtConfig tcfg = make_config(o, 0, 1, RT_FLAG_CACHE_PRIMARY | RT_FLAG_TIMING_ALL);
        const std::unique_ptr<rt::render::Pipeline> tp(rt::render::create_instance(tcfg, noise.data(), game, &err));
        RtTiming tm{};
        if (!tp || tp->draw_frame(game) != RT_OK || tp->wait() != RT_OK || rt_get_timing(tp->context(), &tm) != RT_OK) {
            std::fprintf(stderr, "edit timing pipeline failed: %s\n", tp ? tp->last_error() : err.c_str());
            exit_code = 1;
        } else {
            FrameEdit timed = frame_edit(o, shape, game.camera.origin);
            if (o.edit_stamp > 0 && !stamp_brush_create(tp.get(), timed.stamp_ids)) exit_code = 1;
            const auto w0 = std::chrono::steady_clock::now();
            for (int f = 0; f < frames && !exit_code; f++)
                if (apply_edit(tp.get(), timed, f, &edit_host_ms) != RT_OK) exit_code = 1;
            if (rt_sync(tp->context()) != RT_OK) exit_code = 1;
            edit_wall_ms = ms_since(w0) / frames;
            if (rt_get_timing(tp->context(), &tm) != RT_OK) exit_code = 1;
            edit_dev_ms = tm.shade_ms / frames;
            edit_launches = (double)tm.other_launches / frames;
            edit_host_ms /= frames;
            if (exit_code) std::fprintf(stderr, "edit timing failed: %s\n", rt_last_error(tp->context()));
        }
    }
    if (exit_code && gpus > 1) { std::fflush(nullptr); std::_Exit(1); }   // communicators may hold unmatched operations: no orderly teardown
    if (!exit_code) {
        std::printf("%.3fms / %.3fms\n", perf.average(), perf.max());    // main.rs:45-46: average / max
        // a checksum of the assembled frame's depth plane shows that the gather delivered pixels (0 without --gather)
        unsigned long long checksum = 0;
        if (o.gather) {
            std::vector<uint16_t> depth_plane((size_t)width * height);
            if (rt_frame_readback(pipes[0]->context(), RT_BUF_DEPTH_R16UI, depth_plane.data(), depth_plane.size() * 2) == RT_OK)
                for (uint16_t v : depth_plane) checksum += v;
            else { std::fprintf(stderr, "rt_frame_readback failed: %s\n", pipes[0]->last_error()); exit_code = 1; }
        }
        unsigned long long final_checksum = 0;   // --post: sum over the swapchain image's bytes (0 without)
        if (o.post) {
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
                    width, height, o.spp, o.depth, gpus, o.gather ? (o.overlap ? "rccl-overlapped" : "rccl-serial") : "none", o.post ? "true" : "false",
                    game.camera.origin[0], game.camera.origin[1], game.camera.origin[2], game.camera.heading, game.camera.pitch,
                    game.sun_angle, frames, rays_per_frame, ms, perf.average(), perf.max(), (double)rays_per_frame / (ms * 1e3), checksum, final_checksum,
                    o.accumulate ? "true" : "false", o.reproject ? "true" : "false", (double)o.camera_step, acc_samples, acc_frames, o.edit_radius,
                    o.stream ? "true" : "false", o.stream_history ? "true" : "false", o.edits, o.edit_spread ? "true" : "false", edit_dev_ms, edit_launches,
                    edit_host_ms, edit_wall_ms, o.history_denoise ? ", \"history_denoise\": true" : "", o.edit_shape ? ", \"edit_shape\": \"" : "",
                    o.edit_shape ? o.edit_shape : "", o.edit_shape ? "\"" : "", o.edit_stamp > 0 ? (", \"edit_stamp\": " + std::to_string(o.edit_stamp)).c_str() : "");
    }
    for (int g = 0; g < gpus; g++) {
        if (comms[(size_t)g]) rt_comm_destroy(comms[(size_t)g]);
        delete pipes[(size_t)g];
    }
    return exit_code;
}
