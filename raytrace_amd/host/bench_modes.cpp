// bench_modes.cpp — rt_bench's modes that run instead of the frame loop.  Each opens one session (RT_FLAG_TIMING_ALL where the mode
// reads the device time of a launch from rt_get_timing), builds its records with bench_scene.hpp's builders in the order that
// consumes the generator as the committed figures were measured with, times its calls and prints one JSON line.
#include <algorithm>
#include <cmath>

#include "bench_run.hpp"

namespace bench {

// --rays N: ray queries against the generated world.  rt_trace_rays on N rays — seeded origins in the region with random
// directions, or with --rays-coherent the primary rays of a --width x --height camera at the default pose handed over as arbitrary
// rays — timed call to return (the transfers both ways included; the kernel alone: rocprofv3 --kernel-trace --stats, or
// tools/ray_query_bench.py's device events), then the call-to-return latency of one-pixel rt_pick_pixels, idle and right behind a
// --width x --height --spp --depth frame still in flight.
int run_rays(const Options& o, const World& w) {
    Session s;
    if (!open_session(&s, o, w, 0u)) return 1;
    const uint32_t n = (uint32_t)o.rays;
    const std::vector<RtRay> rays = ray_list(s.view, s.rnd, n, o.rays_coherent);
    std::vector<RtRayHit> hits(n);
    int rc = rt_trace_rays(s.ctx, rays.data(), n, s.u().lr, hits.data());   // warm-up (staging grows once)
    const int reps = n >= (1u << 20) ? 5 : 50;
    auto t = std::chrono::steady_clock::now();
    for (int i = 0; i < reps && rc == RT_OK; i++) rc = rt_trace_rays(s.ctx, rays.data(), n, s.u().lr, hits.data());
    const double ms = ms_since(t) / reps;
    uint64_t solid = 0;
    for (const RtRayHit& h : hits) solid += h.kind == RT_HIT_SOLID;
    const int32_t xy[2] = {o.width / 2, o.height / 2};
    RtRayHit one{};
    std::vector<double> idle, busy;
    for (int i = 0; i < 220 && rc == RT_OK; i++) {
        t = std::chrono::steady_clock::now();
        rc = rt_pick_pixels(s.ctx, &s.u(), xy, 1, &one);
        if (i >= 20) idle.push_back(ms_since(t));
    }
    double frame_ms = 0;
    for (int i = 0; i < 21 && rc == RT_OK; i++) {
        const auto tf = std::chrono::steady_clock::now();
        rc = rt_draw_frame(s.ctx, &s.u());
        t = std::chrono::steady_clock::now();
        if (rc == RT_OK) rc = rt_pick_pixels(s.ctx, &s.u(), xy, 1, &one);
        if (i > 0) busy.push_back(ms_since(t));
        if (rc == RT_OK) rc = rt_sync(s.ctx);
        if (i > 0) frame_ms += ms_since(tf) / 20.0;
    }
    if (rc != RT_OK) return s.fail("ray queries", rc);
    std::sort(idle.begin(), idle.end());
    std::sort(busy.begin(), busy.end());
    std::printf("{\"rays\": %u, \"coherent\": %s, \"trace_rays_ms\": %.4f, \"grays_call_to_return\": %.3f, \"solid_hits\": %llu, "
                "\"pick_ms_idle_median\": %.4f, \"pick_ms_in_flight_median\": %.4f, \"pick_ms_in_flight_max\": %.4f, "
                "\"frame\": \"%dx%d spp %d depth %d\", \"frame_ms\": %.3f}\n",
                n, o.rays_coherent ? "true" : "false", ms, (double)n / (ms * 1e-3) / 1e9, (unsigned long long)solid, idle[idle.size() / 2],
                busy[busy.size() / 2], busy.back(), o.width, o.height, o.spp, o.depth, frame_ms);
    return 0;
}

// --entity-rays N [--coherent] [--boxes B] [--models M] [--model-scale S]: entity queries.  rt_trace_entities on N rays — --rays'
// seeded rays, or with --coherent its camera rays — against B boxes and M models scattered as --boxes and --models scatter them (in
// one index run: the orientation follows the joint index), and rt_trace_rays on the same rays as the yardstick, both timed call to
// return; then their asynchronous twins on device copies of the same records, on a stream of this program's, between two HIP events:
// the device time of each.  The JSON line also counts the rays that report an entity and those whose entity the world occludes.  (The
// kernels alone, k_entity_query and k_query: rocprofv3 --kernel-trace --stats, which tools/entity_query_bench.py runs.)
int run_entity_rays(const Options& o, const World& w) {
    Session s;
    if (!open_session(&s, o, w, 0u)) return 1;
    const uint32_t n = (uint32_t)o.entity_rays, nboxes = (uint32_t)std::max(o.boxes, 0ll), nmodels = (uint32_t)std::max(o.models, 0ll);
    const std::vector<RtRay> rays = ray_list(s.view, s.rnd, n, o.coherent);
    SparseStamp stamp = sparse_stamp(s.rnd, 9, 9, 12);
    if (!s.create_stamp(&stamp)) return 1;
    std::vector<RtDrawBox> boxes(nboxes);
    std::vector<RtDrawStamp> models(nmodels);
    for (uint32_t i = 0; i < nboxes + nmodels; i++) {
        float c[3];
        scatter_point(s.u(), s.rnd, 20.0f, c);   // 20 .. 400 units away
        if (i < nboxes) {
            player_box(c, &boxes[i]);
            boxes[i].material = 0x12345u; boxes[i].emission = 0xFF000000u;
        } else {
            models[i - nboxes] = model_at(stamp, o.model_scale, i, c, nullptr);
        }
    }
    const int32_t* lr = s.u().lr;
    std::vector<RtRayHit> world(n), plain(n);
    std::vector<RtEntityHit> hits(n);
    const int reps = n >= (1u << 20) ? 5 : 20;
    double ms[2] = {0.0, 0.0};
    int rc = RT_OK;
    for (int which = 0; which < 2 && rc == RT_OK; which++) {      // 0: rt_trace_entities, 1: rt_trace_rays on the same rays, the yardstick
        for (int i = 0; i < reps + 1 && rc == RT_OK; i++) {       // (the first repetition warms the staging up)
            const auto t = std::chrono::steady_clock::now();
            rc = which == 0 ? rt_trace_entities(s.ctx, rays.data(), n, lr, boxes.data(), nboxes, models.data(), nmodels, world.data(), hits.data())
                            : rt_trace_rays(s.ctx, rays.data(), n, lr, plain.data());
            if (i > 0) ms[which] += ms_since(t) / reps;
        }
    }
    if (rc != RT_OK) return s.fail("entity queries", rc);
    if (std::memcmp(world.data(), plain.data(), (size_t)n * sizeof(RtRayHit)) != 0) { std::fprintf(stderr, "the world hits differ from rt_trace_rays'\n"); return 1; }
    // reported: the call's own answer; occluded: rays that report an entity only once the world is out of the way — the same call with
    // the window moved 2^20 voxels off, where every ray leaves the region at once (D = 65535)
    uint64_t reported = 0, under_sky = 0, met = 0;
    for (uint32_t i = 0; i < n; i++) { reported += hits[i].kind != RT_ENTITY_NONE; under_sky += hits[i].kind != RT_ENTITY_NONE && world[i].kind == RT_HIT_AIR; }
    const int32_t away[3] = {lr[0] + (1 << 20), lr[1], lr[2]};
    rc = rt_trace_entities(s.ctx, rays.data(), n, away, boxes.data(), nboxes, models.data(), nmodels, nullptr, hits.data());
    if (rc != RT_OK) return s.fail("entity queries", rc);
    for (uint32_t i = 0; i < n; i++) met += hits[i].kind != RT_ENTITY_NONE;
    // device time of each call: the asynchronous twins between two events (-1: the HIP runtime could not be reached from here)
    double device_ms[2] = {-1.0, -1.0};
    const HipEvents hip;
    if (hip.ok) {
        DeviceRun run(hip, s.ctx);
        const RtRay* d_rays = (const RtRay*)run.on_device(rays.data(), (size_t)n * sizeof(RtRay));
        const RtDrawBox* d_boxes = (const RtDrawBox*)run.on_device(boxes.data(), (size_t)nboxes * sizeof(RtDrawBox));
        RtRayHit* d_world = (RtRayHit*)run.on_device(nullptr, (size_t)n * sizeof(RtRayHit));
        RtEntityHit* d_hits = (RtEntityHit*)run.on_device(nullptr, (size_t)n * sizeof(RtEntityHit));
        run.start();
        device_ms[0] = run.repeat(reps, [&] { return rt_trace_entities_async(s.ctx, d_rays, n, lr, nboxes ? d_boxes : nullptr, nboxes, models.data(), nmodels, d_world, d_hits); });
        device_ms[1] = run.repeat(reps, [&] { return rt_trace_rays_async(s.ctx, d_rays, n, lr, d_world); });
        if (!run.close()) { std::fprintf(stderr, "timing the asynchronous calls failed: %s\n", rt_last_error(s.ctx)); return 1; }
    }
    std::printf("{\"entity_rays\": %u, \"coherent\": %s, \"boxes\": %u, \"models\": %u, \"model_scale\": %g, \"trace_entities_call_ms\": %.4f, "
                "\"trace_rays_call_ms\": %.4f, \"ratio\": %.2f, \"entities_reported\": %llu, \"entities_occluded\": %llu, \"reported_under_sky\": %llu, "
                "\"trace_entities_device_ms\": %.4f, \"trace_rays_device_ms\": %.4f}\n",
                n, o.coherent ? "true" : "false", nboxes, nmodels, (double)o.model_scale, ms[0], ms[1], ms[1] > 0.0 ? ms[0] / ms[1] : 0.0,
                (unsigned long long)reported, (unsigned long long)(met > reported ? met - reported : 0), (unsigned long long)under_sky, device_ms[0], device_ms[1]);
    return 0;
}

// --entity-sweeps N [--coherent] [--boxes B] [--models M] [--model-scale S]: entity sweeps.  B boxes and M models scattered as
// --entity-rays scatters them; N player-sized sweeps, each beside one of the entities (or, without entities, at a scattered point of
// its own) and moving up to 2 units per axis.  With --coherent sweep i stands beside entity i * (B + M) / N, so a wave's 64 sweeps
// lie together; without it the same sweeps are handed over in a seeded shuffle.  rt_sweep_entities and, as the yardstick,
// rt_sweep_boxes on the same records, both timed call to return; then their asynchronous twins on device copies, between two HIP
// events: the device time of each.  The JSON line also counts what the entities and the world blocked.  (The kernels alone,
// k_sweep_entities and k_sweep: rocprofv3 --kernel-trace --stats, which tools/sweep_entities_profile.py runs.)
int run_entity_sweeps(const Options& o, const World& w) {
    Session s;
    if (!open_session(&s, o, w, 0u)) return 1;
    const uint32_t n = (uint32_t)o.entity_sweeps, nboxes = (uint32_t)std::max(o.boxes, 0ll), nmodels = (uint32_t)std::max(o.models, 0ll);
    const uint32_t nent = nboxes + nmodels;
    SparseStamp stamp = sparse_stamp(s.rnd, 9, 9, 12);
    if (!s.create_stamp(&stamp)) return 1;
    std::vector<RtDrawBox> boxes(nboxes);
    std::vector<RtDrawStamp> models(nmodels);
    std::vector<float> centres(3u * (size_t)nent);
    for (uint32_t i = 0; i < nent; i++) {
        float* c = &centres[3u * (size_t)i];
        scatter_point(s.u(), s.rnd, 20.0f, c);   // 20 .. 400 units away
        if (i < nboxes) {
            player_box(c, &boxes[i]);
            boxes[i].material = 0x12345u; boxes[i].emission = 0xFF000000u;
        } else {
            models[i - nboxes] = model_at(stamp, o.model_scale, i, c, nullptr);
        }
    }
    std::vector<RtBoxSweep> sweeps(n);
    for (uint32_t i = 0; i < n; i++) {
        float c[3];
        if (nent) { const float* e = &centres[3u * (size_t)((uint64_t)i * nent / n)]; for (int a = 0; a < 3; a++) c[a] = e[a] + (s.rnd() * 2.0f - 1.0f) * 3.0f; }
        else scatter_point(s.u(), s.rnd, 20.0f, c);
        RtDrawBox b{};
        player_box(c, &b);
        RtBoxSweep& sw = sweeps[i];
        sw = RtBoxSweep{};
        for (int a = 0; a < 3; a++) { sw.lo[a] = b.lo[a]; sw.hi[a] = b.hi[a]; sw.motion[a] = (s.rnd() * 2.0f - 1.0f) * 2.0f; }
    }
    if (!o.coherent)
        for (uint32_t i = n; i > 1; i--) std::swap(sweeps[i - 1], sweeps[std::min(i - 1, (uint32_t)(s.rnd() * (float)i))]);
    const int32_t* lr = s.u().lr;
    std::vector<RtSweepHit> world(n), plain(n);
    std::vector<RtEntitySweepHit> hits(n);
    const int reps = n >= (1u << 19) ? 5 : 20;
    double ms[2] = {0.0, 0.0};
    int rc = RT_OK;
    for (int which = 0; which < 2 && rc == RT_OK; which++) {      // 0: rt_sweep_entities, 1: rt_sweep_boxes on the same records, the yardstick
        for (int i = 0; i < reps + 1 && rc == RT_OK; i++) {       // (the first repetition warms the staging up)
            const auto t = std::chrono::steady_clock::now();
            rc = which == 0 ? rt_sweep_entities(s.ctx, sweeps.data(), n, lr, boxes.data(), nboxes, models.data(), nmodels, world.data(), hits.data())
                            : rt_sweep_boxes(s.ctx, sweeps.data(), n, lr, plain.data());
            if (i > 0) ms[which] += ms_since(t) / reps;
        }
    }
    if (rc != RT_OK) return s.fail("entity sweeps", rc);
    if (std::memcmp(world.data(), plain.data(), (size_t)n * sizeof(RtSweepHit)) != 0) { std::fprintf(stderr, "the world hits differ from rt_sweep_boxes'\n"); return 1; }
    uint64_t by_entity = 0, embedded = 0, by_world = 0;
    for (uint32_t i = 0; i < n; i++) {
        by_entity += hits[i].kind == RT_SWEEP_BLOCKED; embedded += hits[i].kind == RT_SWEEP_EMBEDDED;
        by_world += hits[i].entity == RT_ENTITY_NONE && world[i].kind == RT_SWEEP_BLOCKED;
    }
    // device time of each call: the asynchronous twins between two events (-1: the HIP runtime could not be reached from here)
    double device_ms[2] = {-1.0, -1.0};
    const HipEvents hip;
    if (hip.ok) {
        DeviceRun run(hip, s.ctx);
        const RtBoxSweep* d_sweeps = (const RtBoxSweep*)run.on_device(sweeps.data(), (size_t)n * sizeof(RtBoxSweep));
        const RtDrawBox* d_boxes = (const RtDrawBox*)run.on_device(boxes.data(), (size_t)nboxes * sizeof(RtDrawBox));
        RtSweepHit* d_world = (RtSweepHit*)run.on_device(nullptr, (size_t)n * sizeof(RtSweepHit));
        RtEntitySweepHit* d_hits = (RtEntitySweepHit*)run.on_device(nullptr, (size_t)n * sizeof(RtEntitySweepHit));
        run.start();
        device_ms[0] = run.repeat(reps, [&] { return rt_sweep_entities_async(s.ctx, d_sweeps, n, lr, nboxes ? d_boxes : nullptr, nboxes, models.data(), nmodels, d_world, d_hits); });
        device_ms[1] = run.repeat(reps, [&] { return rt_sweep_boxes_async(s.ctx, d_sweeps, n, lr, d_world); });
        if (!run.close()) { std::fprintf(stderr, "timing the asynchronous calls failed: %s\n", rt_last_error(s.ctx)); return 1; }
    }
    std::printf("{\"entity_sweeps\": %u, \"coherent\": %s, \"boxes\": %u, \"models\": %u, \"model_scale\": %g, \"sweep_entities_call_ms\": %.4f, "
                "\"sweep_boxes_call_ms\": %.4f, \"ratio\": %.2f, \"blocked_by_entity\": %llu, \"embedded_in_entity\": %llu, \"blocked_by_world\": %llu, "
                "\"sweep_entities_device_ms\": %.4f, \"sweep_boxes_device_ms\": %.4f}\n",
                n, o.coherent ? "true" : "false", nboxes, nmodels, (double)o.model_scale, ms[0], ms[1], ms[1] > 0.0 ? ms[0] / ms[1] : 0.0,
                (unsigned long long)by_entity, (unsigned long long)embedded, (unsigned long long)by_world, device_ms[0], device_ms[1]);
    return 0;
}

// --boxes N: entity boxes.  N entity-sized boxes are scattered deterministically in front of the camera (20 to 400 units away, over
// the whole view), their six face probes lit with rt_probe_light (4 samples, depth 2), and rt_draw_boxes composites them into a
// freshly drawn --width x --height frame, 20 times.  One JSON line: the device time of the pass, the call-to-return time of
// rt_draw_boxes and of the probes, and the pixels drawn.
int run_boxes(const Options& o, const World& w) {
    Session s;
    if (!open_session(&s, o, w, RT_FLAG_TIMING_ALL)) return 1;
    const uint32_t n = (uint32_t)o.boxes;
    std::vector<RtDrawBox> boxes(n);
    std::vector<RtLightProbe> probes(6u * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        float c[3];
        scatter_point(s.u(), s.rnd, 20.0f, c);
        player_box(c, &boxes[i]);
        boxes[i].material = material_word(i); boxes[i].emission = 0xFF000000u;
        face_probes(boxes[i], i, &probes[6u * (size_t)i]);
    }
    std::vector<RtProbeLight> lights(probes.size());
    const auto t = std::chrono::steady_clock::now();
    int rc = n ? rt_probe_light(s.ctx, &s.u(), probes.data(), (uint32_t)probes.size(), 4, 2, lights.data()) : RT_OK;
    const double probe_ms = ms_since(t);
    const size_t npix = (size_t)o.width * (size_t)o.height;
    std::vector<float> before(npix), after(npix);
    if (rc == RT_OK) rc = s.read_plane(RT_BUF_DEPTH_F32, &before);
    PassTime pt;
    rc = timed_pass(s, rc, &pt, [&] { return rt_draw_boxes(s.ctx, &s.u(), boxes.data(), lights.data(), n); });
    if (rc == RT_OK) rc = s.read_plane(RT_BUF_DEPTH_F32, &after);
    if (rc != RT_OK) return s.fail("entity boxes", rc);
    std::printf("{\"boxes\": %u, \"frame\": \"%dx%d spp %d depth %d\", \"draw_boxes_device_ms\": %.4f, \"draw_boxes_call_ms\": %.4f, "
                "\"launches_per_call\": %.2f, \"probe_light_call_ms\": %.3f, \"pixels_drawn\": %llu}\n",
                n, o.width, o.height, o.spp, o.depth, pt.device_ms, pt.call_ms, (double)pt.launches / PASS_REPS, probe_ms,
                (unsigned long long)changed_pixels(before, after, 1));
    return 0;
}

// --particles N [--particle-half H] [--particle-near D]: particles.  A seeded cloud of N cubes of half edge H (default 1/16) is
// scattered in front of the camera, D to 20 D units away (default 10 to 200, log-uniform) over the whole view, lit by 64 whole-sphere
// probes that the particles share, and drawn by rt_draw_particles into a freshly drawn --width x --height frame, 20 times; with
// N <= 4096, as a yardstick in the same process, rt_draw_boxes draws the derived boxes, 20 times.  One JSON line: the device time per
// call (the memset and the four launches bracketed by events), the call-to-return time and the pixels drawn, of both.
// (--particle-half 300 --particle-near 400 makes every particle wide: the worst path.)
int run_particles(const Options& o, const World& w) {
    Session s;
    if (!open_session(&s, o, w, RT_FLAG_TIMING_ALL)) return 1;
    const uint32_t n = (uint32_t)o.particles, nlights = SHARED_LIGHTS;
    std::vector<RtParticle> particles(n);
    std::vector<RtDrawBox> boxes(n <= 4096u ? n : 0u);            // the yardstick: rt_draw_boxes on the derived boxes
    std::vector<RtLightProbe> probes(nlights);
    for (uint32_t i = 0; i < n; i++) {
        RtParticle& q = particles[i];
        q = RtParticle{};
        scatter_point(s.u(), s.rnd, o.particle_near, q.center);
        q.half = o.particle_half; q.material = material_word(i); q.emission = 0xFF000000u; q.light = i % nlights;
        if (i < boxes.size()) {
            RtDrawBox& b = boxes[i];
            for (int a = 0; a < 3; a++) { b.lo[a] = q.center[a] - q.half; b.hi[a] = q.center[a] + q.half; }
            b.material = q.material; b.emission = q.emission;
        }
        if (i < nlights) probes[i] = sphere_probe(i, q.center);
    }
    std::vector<RtProbeLight> lights(nlights);
    int rc = n ? rt_probe_light(s.ctx, &s.u(), probes.data(), n < nlights ? n : nlights, 4, 2, lights.data()) : RT_OK;
    std::vector<RtProbeLight> face(6u * boxes.size());
    for (size_t i = 0; i < face.size(); i++) face[i] = lights[particles[i / 6u].light];
    const size_t npix = (size_t)o.width * (size_t)o.height;
    std::vector<float> before(npix), after(npix);
    if (rc == RT_OK) rc = s.read_plane(RT_BUF_DEPTH_F32, &before);
    PassTime pt[2];
    uint64_t drawn[2] = {0, 0};
    for (int pass = 0; pass < (boxes.empty() ? 1 : 2) && rc == RT_OK; pass++) {     // 0: the particles, 1: their boxes
        rc = timed_pass(s, rc, &pt[pass], [&] {
            return pass == 0 ? rt_draw_particles(s.ctx, &s.u(), particles.data(), n, lights.data(), nlights)
                             : rt_draw_boxes(s.ctx, &s.u(), boxes.data(), face.data(), n);
        });
        if (rc == RT_OK) rc = s.read_plane(RT_BUF_DEPTH_F32, &after);
        drawn[pass] = changed_pixels(before, after, 1);
    }
    if (rc != RT_OK) return s.fail("particles", rc);
    std::printf("{\"particles\": %u, \"half\": %g, \"near\": %g, \"frame\": \"%dx%d spp %d depth %d\", \"draw_particles_device_ms\": %.4f, "
                "\"draw_particles_call_ms\": %.4f, \"pixels_drawn\": %llu",
                n, (double)o.particle_half, (double)o.particle_near, o.width, o.height, o.spp, o.depth, pt[0].device_ms, pt[0].call_ms,
                (unsigned long long)drawn[0]);
    if (!boxes.empty())
        std::printf(", \"draw_boxes_device_ms\": %.4f, \"draw_boxes_call_ms\": %.4f, \"boxes_pixels_drawn\": %llu", pt[1].device_ms, pt[1].call_ms,
                    (unsigned long long)drawn[1]);
    std::printf("}\n");
    return 0;
}

// --particles N --simulate T [--sweeps S]: instead of drawing the cloud as it stands, simulate it.  The cloud's cubes become debris
// (RtParticleState: the cube as the swept box, a seeded velocity up to 12 units per second per axis — drawn axis by axis, after that
// particle's scatter — RT_PARTICLE_BOUNCE, gravity 32, dt 1/60, restitution 1/2, friction 3/4, S sub-sweeps per tick, default 3) in
// device buffers.  T ticks follow each other there without a host read: a frame, then rt_step_particles_async ->
// rt_draw_particles_async, the tick's two calls bracketed by events.  In the same process, between events of their own: the first
// tick alone, repeated, and rt_sweep_boxes_async — the yardstick — on the same boxes with that tick's motions; and the synchronous
// rt_sweep_boxes on those records, call to return: the host round trip a tick on the device replaces (without the upload of the
// draw records it would also need).
int run_simulate(const Options& o, const World& w) {
    Session s;
    if (!open_session(&s, o, w, 0u)) return 1;
    const HipEvents hip;
    if (!hip.ok) { std::fprintf(stderr, "--simulate needs the HIP runtime for its device buffers\n"); return 1; }
    const uint32_t n = (uint32_t)o.particles, nlights = SHARED_LIGHTS;
    const float half = o.particle_half;
    const int32_t* lr = s.u().lr;
    RtParticleStep step{};
    step.dt = 1.0f / 60.0f; step.accel[2] = -32.0f; step.damping = 1.0f; step.restitution = 0.5f; step.friction = 0.75f; step.rest_speed = 0.5f;
    for (int a = 0; a < 3; a++) step.lr[a] = lr[a];
    step.sweeps = (uint32_t)o.step_sweeps;
    // debris: --particles' scatter, every cube with a seeded velocity; and the same boxes with the first tick's motions as plain sweeps
    std::vector<RtParticleState> states(n);
    std::vector<RtBoxSweep> as_sweeps(n);
    std::vector<RtLightProbe> probes(nlights);
    for (uint32_t i = 0; i < n; i++) {
        float c[3], mid[3];
        scatter_point(s.u(), s.rnd, o.particle_near, c);
        RtParticleState& p = states[i];
        p = RtParticleState{};
        RtBoxSweep& b = as_sweeps[i];
        b = RtBoxSweep{};
        for (int a = 0; a < 3; a++) {
            p.lo[a] = b.lo[a] = c[a] - half; p.hi[a] = b.hi[a] = c[a] + half;
            p.velocity[a] = (s.rnd() * 2.0f - 1.0f) * 12.0f;
            const float m = (p.velocity[a] + step.accel[a] * step.dt) * step.damping * step.dt;
            b.motion[a] = m < -64.0f ? -64.0f : (m > 64.0f ? 64.0f : m);
            mid[a] = 0.5f * (p.lo[a] + p.hi[a]);
        }
        p.life = INFINITY; p.flags = RT_PARTICLE_BOUNCE; p.half = half; p.light = i % nlights;
        p.material = material_word(i); p.emission = 0xFF000000u;
        if (i < nlights) probes[i] = sphere_probe(i, mid);
    }
    std::vector<RtProbeLight> lights(nlights);
    int rc = n ? rt_probe_light(s.ctx, &s.u(), probes.data(), n < nlights ? n : nlights, 4, 2, lights.data()) : RT_OK;
    // the host round trip a tick on the device replaces, in part: the synchronous sweep of the same records
    std::vector<RtSweepHit> hits(n);
    const int reps = n >= (1u << 19) ? 5 : 20;
    double sync_ms = 0.0;
    for (int i = 0; i < 4 && rc == RT_OK; i++) {                  // (the first call warms the staging up)
        const auto t = std::chrono::steady_clock::now();
        rc = rt_sweep_boxes(s.ctx, as_sweeps.data(), n, lr, hits.data());
        if (i > 0) sync_ms += ms_since(t) / 3.0;
    }
    uint64_t blocked = 0;
    for (uint32_t i = 0; i < n; i++) blocked += hits[i].kind == RT_SWEEP_BLOCKED;
    if (rc != RT_OK) return s.fail("simulate", rc);
    DeviceRun run(hip, s.ctx);
    RtParticleState* d_a = (RtParticleState*)run.on_device(states.data(), (size_t)n * sizeof(RtParticleState));
    RtParticleState* d_b = (RtParticleState*)run.on_device(nullptr, (size_t)n * sizeof(RtParticleState));
    const RtParticleState* d_first = (const RtParticleState*)run.on_device(states.data(), (size_t)n * sizeof(RtParticleState));
    RtParticle* d_draw = (RtParticle*)run.on_device(nullptr, (size_t)n * sizeof(RtParticle));
    const RtBoxSweep* d_sweeps = (const RtBoxSweep*)run.on_device(as_sweeps.data(), (size_t)n * sizeof(RtBoxSweep));
    RtSweepHit* d_hits = (RtSweepHit*)run.on_device(nullptr, (size_t)n * sizeof(RtSweepHit));
    const RtProbeLight* d_lights = (const RtProbeLight*)run.on_device(lights.data(), (size_t)nlights * sizeof(RtProbeLight));
    run.start();
    // the first tick from the initial states and the plain sweep of the same boxes and motions: the same launch repeated between two events
    const double first_ms = run.repeat(reps, [&] { return rt_step_particles_async(s.ctx, &step, d_first, d_b, d_draw, n); });
    const double sweep_ms = run.repeat(reps, [&] { return rt_sweep_boxes_async(s.ctx, d_sweeps, n, lr, d_hits); });
    // T ticks chained on the device: the frame (not timed), then step -> draw between two events
    double tick_ms = 0.0;
    for (int t = 0; t < o.simulate && run.fine; t++) {
        run.fine = rt_draw_frame(s.ctx, &s.u()) == RT_OK && run.mark() && rt_step_particles_async(s.ctx, &step, d_a, d_b, d_draw, n) == RT_OK &&
                   rt_draw_particles_async(s.ctx, &s.u(), d_draw, n, d_lights, nlights) == RT_OK;
        float ms = 0.0f;
        run.fine = run.fine && run.lap(&ms);
        tick_ms += (double)ms / o.simulate;
        std::swap(d_a, d_b);
    }
    uint64_t alive = 0, contact = 0;
    if (run.fine && n) {
        run.fine = rt_sync(s.ctx) == RT_OK && hip.copy(states.data(), d_a, (size_t)n * sizeof(RtParticleState), 2 /* hipMemcpyDeviceToHost */) == 0;
        for (const RtParticleState& p : states) { alive += !(p.flags & (RT_PSTATE_DEAD | RT_PSTATE_INVALID)); contact += (p.flags & RT_PSTATE_CONTACT) != 0; }
    }
    if (!run.close()) { std::fprintf(stderr, "simulate failed: %s\n", rt_last_error(s.ctx)); return 1; }
    std::printf("{\"particles\": %u, \"half\": %g, \"simulate\": %d, \"sweeps\": %u, \"frame\": \"%dx%d spp %d depth %d\", \"step_device_ms\": %.4f, "
                "\"sweep_boxes_device_ms\": %.4f, \"step_over_sweep\": %.2f, \"tick_device_ms\": %.4f, \"sweep_boxes_sync_call_ms\": %.3f, "
                "\"first_tick_blocked\": %llu, \"alive\": %llu, \"in_contact_last_tick\": %llu}\n",
                n, (double)half, o.simulate, step.sweeps, o.width, o.height, o.spp, o.depth, first_ms, sweep_ms, sweep_ms > 0.0 ? first_ms / sweep_ms : 0.0,
                tick_ms, sync_ms, (unsigned long long)blocked, (unsigned long long)alive, (unsigned long long)contact);
    return 0;
}

// --debris RADIUS [--density D]: particle emitters.  An explosion where the view's centre pixel meets the terrain: a sphere of RADIUS
// round the hit voxel, every D-th of 256 of its occupied voxels (default all) becoming a particle.  Each of 20 ticks runs, with no
// host read, rt_emit_particles_async -> rt_edit_shapes (the carve) -> rt_step_particles_async -> rt_draw_particles_async into the
// frame drawn last, bracketed by events; between the ticks the sphere is filled again (not timed).  In the same process: the emit
// alone, repeated between two events; rt_stamp_capture of the sphere's bounding box — it reads the same voxels: a floor for the read
// side — by rt_get_timing's launch times; and the host path the emit replaces, call to usable device buffer: rt_read_box of the
// bounding box, membership, hash and states on the host, hipMemcpy.
static uint32_t debris_mix(uint32_t h) { h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16; return h; }
int run_debris(const Options& o, const World& w) {
    Session s;
    if (!open_session(&s, o, w, RT_FLAG_TIMING_ALL)) return 1;
    const HipEvents hip;
    if (!hip.ok) { std::fprintf(stderr, "--debris needs the HIP runtime for its device buffers\n"); return 1; }
    const int R = RT_ROOT_BLOCK_SIZE, radius = o.debris;
    const int32_t* lr = s.u().lr;
    const int32_t centre_px[2] = {o.width / 2, o.height / 2};
    RtRayHit hit{};
    int rc = rt_pick_pixels(s.ctx, &s.u(), centre_px, 1, &hit);
    if (rc != RT_OK) return s.fail("debris", rc);
    int c[3] = {R / 2, R / 2, R / 2};
    if (hit.kind == RT_HIT_SOLID) for (int a = 0; a < 3; a++) c[a] = hit.texel[a];
    RtParticleEmit e{};
    int32_t lo[3], ext[3];
    for (int a = 0; a < 3; a++) {
        e.a[a] = 2 * c[a] + 1;
        // world coordinates of the texel's centre under lr (the sweeps' addressing)
        e.origin[a] = (float)(lr[a] - R / 2 + (((c[a] - lr[a]) % R + R) % R)) + 0.5f;
        lo[a] = c[a] - radius < 0 ? 0 : c[a] - radius;
        const int hi = c[a] + radius > R - 1 ? R - 1 : c[a] + radius;
        ext[a] = hi - lo[a] + 1;
    }
    e.b[0] = 4 * radius * radius; e.kind = RT_SHAPE_SPHERE; e.response = RT_PARTICLE_BOUNCE; e.seed = 0x5EEDu;
    e.speed = 12.0f; e.spread = 3.0f; e.drift[2] = 4.0f; e.half = 0.125f; e.life_min = 1.0f; e.life_span = 2.0f;
    e.density = (uint32_t)o.debris_density; e.emission = 0xFF000000u;
    RtShapeEdit carve{}, fill{};
    for (int a = 0; a < 3; a++) { carve.a[a] = e.a[a]; carve.b[a] = e.b[a]; }
    carve.kind = RT_SHAPE_SPHERE; carve.where = RT_WHERE_ALL; carve.solid = 0;
    fill = carve; fill.solid = 1; fill.material = BRUSH_MATERIAL;
    RtParticleStep step{};
    step.dt = 1.0f / 60.0f; step.accel[2] = -32.0f; step.damping = 1.0f; step.restitution = 0.5f; step.friction = 0.75f; step.rest_speed = 0.5f;
    for (int a = 0; a < 3; a++) step.lr[a] = lr[a];
    step.sweeps = (uint32_t)o.step_sweeps;
    const uint32_t capacity = 1u << 20;

    // the host path: read the box back, select and build on the host, upload — three times, the first discarded
    const size_t nvox = (size_t)ext[0] * ext[1] * ext[2];
    std::vector<uint32_t> box_mats(nvox);
    std::vector<uint8_t> box_mine(nvox);
    std::vector<RtParticleState> built;
    void* d_host_ring = nullptr;
    if (hip.dev_malloc(&d_host_ring, (size_t)capacity * sizeof(RtParticleState)) != 0) { std::fprintf(stderr, "--debris: no device memory\n"); return 1; }
    double host_ms = 0.0;
    for (int i = 0; i < 3 && rc == RT_OK; i++) {
        const auto t = std::chrono::steady_clock::now();
        rc = rt_read_box(s.ctx, lo[0], lo[1], lo[2], ext[0], ext[1], ext[2], box_mats.data(), box_mine.data());
        built.clear();
        for (int z = 0; z < ext[2] && rc == RT_OK; z++)
            for (int y = 0; y < ext[1]; y++)
                for (int x = 0; x < ext[0]; x++) {
                    const size_t at = ((size_t)z * ext[1] + y) * ext[0] + x;
                    const int t3[3] = {lo[0] + x, lo[1] + y, lo[2] + z};
                    long long d2 = 0;
                    int v[3];
                    for (int a = 0; a < 3; a++) {
                        const long long d = 2 * t3[a] + 1 - e.a[a];
                        d2 += d * d;
                        v[a] = lr[a] - R / 2 + (((t3[a] - lr[a]) % R + R) % R);
                    }
                    if (d2 > e.b[0] || box_mine[at] != 0u) continue;
                    const uint32_t h = debris_mix(e.seed ^ debris_mix((uint32_t)v[0] ^ debris_mix((uint32_t)v[1] ^ debris_mix((uint32_t)v[2]))));
                    if ((h & 255u) >= e.density) continue;
                    RtParticleState p{};
                    float r[3], len2 = 0.0f;
                    for (int a = 0; a < 3; a++) {
                        const float cc = (float)v[a] + 0.5f;
                        p.lo[a] = cc - e.half; p.hi[a] = cc + e.half;
                        r[a] = cc - e.origin[a];
                        len2 += r[a] * r[a];
                    }
                    const float len = std::sqrt(len2);
                    for (int a = 0; a < 3; a++) {
                        const float u = (float)(debris_mix(h + 1u + (uint32_t)a) >> 8) * 5.9604644775390625e-08f;
                        p.velocity[a] = ((len > 0.0f ? r[a] / len : 0.0f) * e.speed + (u * 2.0f - 1.0f) * e.spread) + e.drift[a];
                    }
                    p.life = e.life_min + (float)(debris_mix(h + 4u) >> 8) * 5.9604644775390625e-08f * e.life_span;
                    p.flags = e.response; p.material = box_mats[at]; p.emission = e.emission; p.half = e.half;
                    built.push_back(p);
                }
        const size_t keep = built.size() < capacity ? built.size() : capacity;
        if (rc == RT_OK && keep && hip.copy(d_host_ring, built.data(), keep * sizeof(RtParticleState), 1 /* hipMemcpyHostToDevice */) != 0) rc = RT_ERR_HIP;
        if (i > 0) host_ms += ms_since(t) / 2.0;
    }
    (void)hip.dev_free(d_host_ring);
    if (rc != RT_OK) return s.fail("debris", rc);

    // rt_stamp_capture of the bounding box: its launch times alone (rt_get_timing), 5 captures after one that is discarded
    double capture_ms = -1.0;
    if (nvox <= (1u << 24)) {
        RtTiming tm{};
        capture_ms = 0.0;
        for (int i = 0; i < 6 && rc == RT_OK; i++) {
            uint32_t id = 0;
            rc = rt_sync(s.ctx);
            if (rc == RT_OK) rc = rt_get_timing(s.ctx, &tm);
            if (rc == RT_OK) rc = rt_stamp_capture(s.ctx, lo, ext, 0u, &id);
            if (rc == RT_OK) rc = rt_sync(s.ctx);
            if (rc == RT_OK) rc = rt_get_timing(s.ctx, &tm);
            if (rc == RT_OK) rc = rt_stamp_destroy(s.ctx, id);
            if (i > 0) capture_ms += tm.shade_ms / 5.0;
        }
        if (rc != RT_OK) return s.fail("debris", rc);
    }

    RtProbeLight light{};
    const RtLightProbe probe = sphere_probe(0, e.origin);
    rc = rt_probe_light(s.ctx, &s.u(), &probe, 1, 4, 2, &light);
    if (rc != RT_OK) return s.fail("debris", rc);
    DeviceRun run(hip, s.ctx);
    const RtEmitCursor zero{0u, 0u, 0u, 0u};
    RtParticleState* d_ring = (RtParticleState*)run.on_device(nullptr, (size_t)capacity * sizeof(RtParticleState));
    RtEmitCursor* d_cursor = (RtEmitCursor*)run.on_device(&zero, sizeof zero);
    RtParticle* d_draw = (RtParticle*)run.on_device(nullptr, (size_t)capacity * sizeof(RtParticle));
    const RtProbeLight* d_light = (const RtProbeLight*)run.on_device(&light, sizeof light);
    run.start();
    // the emit alone: the same call repeated between two events (the ring wraps; the world does not change)
    const int reps = 20;
    const double emit_ms = run.repeat(reps, [&] { return rt_emit_particles_async(s.ctx, &e, 1, lr, d_ring, capacity, capacity, d_cursor); });
    RtEmitCursor after{};
    if (run.fine) run.fine = rt_sync(s.ctx) == RT_OK && hip.copy(&after, d_cursor, sizeof after, 2 /* hipMemcpyDeviceToHost */) == 0;
    const uint32_t selected = (after.emitted + after.dropped) / (uint32_t)(reps + 1);
    const uint32_t live = selected < capacity ? selected : capacity;
    // the ticks: emit -> carve -> step -> draw between two events, the fill outside them
    double tick_ms = 0.0;
    const int ticks = 20;
    for (int t = 0; t < ticks && run.fine; t++) {
        run.fine = hip.copy(d_cursor, &zero, sizeof zero, 1) == 0 && rt_draw_frame(s.ctx, &s.u()) == RT_OK && run.mark() &&
                   rt_emit_particles_async(s.ctx, &e, 1, lr, d_ring, capacity, capacity, d_cursor) == RT_OK &&
                   rt_edit_shapes(s.ctx, &carve, 1) == RT_OK && rt_step_particles_async(s.ctx, &step, d_ring, d_ring, d_draw, live) == RT_OK &&
                   rt_draw_particles_async(s.ctx, &s.u(), d_draw, live, d_light, 1) == RT_OK;
        float ms = 0.0f;
        run.fine = run.fine && run.lap(&ms);
        tick_ms += (double)ms / ticks;
        run.fine = run.fine && rt_edit_shapes(s.ctx, &fill, 1) == RT_OK;
    }
    if (!run.close()) { std::fprintf(stderr, "debris failed: %s\n", rt_last_error(s.ctx)); return 1; }
    // the host path restates the selection: it is a baseline only while it selects what the library selects
    if (built.size() != (size_t)selected) { std::fprintf(stderr, "debris: the host path built %zu states, the library selected %u\n", built.size(), selected); return 1; }
    uint64_t bricks = 1;
    for (int a = 0; a < 3; a++) bricks *= (uint64_t)(((lo[a] + ext[a] - 1) >> 2) - (lo[a] >> 2) + 1);
    std::printf("{\"debris\": %d, \"density\": %d, \"centre\": [%d, %d, %d], \"box\": [%d, %d, %d], \"bricks\": %llu, \"selected\": %u, "
                "\"host_built\": %zu, \"frame\": \"%dx%d spp %d depth %d\", \"emit_device_ms\": %.4f, \"capture_device_ms\": %.4f, "
                "\"emit_over_capture\": %.2f, \"tick_device_ms\": %.4f, \"host_path_ms\": %.3f}\n",
                radius, o.debris_density, c[0], c[1], c[2], ext[0], ext[1], ext[2], (unsigned long long)bricks, selected, built.size(), o.width,
                o.height, o.spp, o.depth, emit_ms, capture_ms, capture_ms > 0.0 ? emit_ms / capture_ms : 0.0, tick_ms, host_ms);
    return 0;
}

// The scene of --debris RADIUS --settle T and of its --fall K: the explosion at the voxel under the frame's centre with RT_PARTICLE_STICK
// debris, the sphere that carves it, the step of a tick and the deposit box — the explosion's bounding box grown by 32 texels (lo, ext).
struct DebrisPile {
    int c[3];
    int32_t lo[3], ext[3];
    RtParticleEmit e{};
    RtParticleDeposit dep{};
    RtShapeEdit carve{};
    RtParticleStep step{};
};
static int make_debris_pile(const Options& o, const Session& s, DebrisPile* pile) {
    const int R = RT_ROOT_BLOCK_SIZE, radius = o.debris;
    const int32_t* lr = s.u().lr;
    const int32_t centre_px[2] = {o.width / 2, o.height / 2};
    RtRayHit hit{};
    int rc = rt_pick_pixels(s.ctx, &s.u(), centre_px, 1, &hit);
    if (rc != RT_OK) return rc;
    int (&c)[3] = pile->c;
    c[0] = c[1] = c[2] = R / 2;
    if (hit.kind == RT_HIT_SOLID) for (int a = 0; a < 3; a++) c[a] = hit.texel[a];
    RtParticleEmit& e = pile->e;
    RtParticleDeposit& dep = pile->dep;
    int32_t (&lo)[3] = pile->lo, (&ext)[3] = pile->ext;
    for (int a = 0; a < 3; a++) {
        e.a[a] = 2 * c[a] + 1;
        e.origin[a] = (float)(lr[a] - R / 2 + (((c[a] - lr[a]) % R + R) % R)) + 0.5f;
        lo[a] = c[a] - radius - 32 < 0 ? 0 : c[a] - radius - 32;
        const int hi = c[a] + radius + 32 > R - 1 ? R - 1 : c[a] + radius + 32;
        ext[a] = hi - lo[a] + 1;
        dep.lo[a] = lo[a]; dep.hi[a] = hi; dep.lr[a] = lr[a];
    }
    e.b[0] = 4 * radius * radius; e.kind = RT_SHAPE_SPHERE; e.response = RT_PARTICLE_STICK; e.seed = 0x5EEDu;
    e.speed = 12.0f; e.spread = 3.0f; e.drift[2] = 4.0f; e.half = 0.125f; e.life_min = 30.0f; e.life_span = 2.0f;
    e.density = (uint32_t)o.debris_density; e.emission = 0xFF000000u;
    RtShapeEdit& carve = pile->carve;
    for (int a = 0; a < 3; a++) { carve.a[a] = e.a[a]; carve.b[a] = e.b[a]; }
    carve.kind = RT_SHAPE_SPHERE; carve.where = RT_WHERE_ALL; carve.solid = 0;
    RtParticleStep& step = pile->step;
    step.dt = 1.0f / 60.0f; step.accel[2] = -32.0f; step.damping = 1.0f; step.restitution = 0.5f; step.friction = 0.75f; step.rest_speed = 0.5f;
    for (int a = 0; a < 3; a++) step.lr[a] = lr[a];
    step.sweeps = (uint32_t)o.step_sweeps;
    return RT_OK;
}

// --debris RADIUS --settle T [--density D]: particle deposits.  --debris' explosion with RT_PARTICLE_STICK debris: emit, carve, then T
// ticks of rt_step_particles_async -> rt_deposit_particles_async -> rt_draw_particles_async with no host read, each of the three
// calls between events of its own; the deposit box is the explosion's bounding box grown by 32 texels.  Then the region's box is put
// back as it was (a stamp captured before the run) and the same T ticks run with the host path the deposit replaces, call to usable
// device state: the ring read back, the box's minefield read back (rt_read_box), the resting particles selected and turned into
// RtVoxelEdit records, rt_edit_voxels, the ring uploaded again with the dead marked.  The mode fails if the host path deposits a
// different number of voxels than the device's counts say.
int run_settle(const Options& o, const World& w) {
    Session s;
    if (!open_session(&s, o, w, RT_FLAG_TIMING_ALL)) return 1;
    const HipEvents hip;
    if (!hip.ok) { std::fprintf(stderr, "--settle needs the HIP runtime for its device buffers\n"); return 1; }
    const int R = RT_ROOT_BLOCK_SIZE, radius = o.debris, ticks = o.settle;
    const int32_t* lr = s.u().lr;
    DebrisPile pile;
    int rc = make_debris_pile(o, s, &pile);
    if (rc != RT_OK) return s.fail("settle", rc);
    const int (&c)[3] = pile.c;
    const int32_t (&lo)[3] = pile.lo, (&ext)[3] = pile.ext;
    const RtParticleEmit& e = pile.e;
    const RtParticleDeposit& dep = pile.dep;
    const RtShapeEdit& carve = pile.carve;
    const RtParticleStep& step = pile.step;
    const uint32_t capacity = 1u << 20;

    uint32_t undo = 0;
    rc = rt_stamp_capture(s.ctx, lo, ext, 0u, &undo);
    RtProbeLight light{};
    const RtLightProbe probe = sphere_probe(0, e.origin);
    if (rc == RT_OK) rc = rt_probe_light(s.ctx, &s.u(), &probe, 1, 4, 2, &light);
    if (rc != RT_OK) return s.fail("settle", rc);
    RtStampPlace back{};
    for (int a = 0; a < 3; a++) back.at[a] = lo[a];
    back.stamp = undo; back.where = RT_WHERE_ALL;

    DeviceRun run(hip, s.ctx);
    const RtEmitCursor zero{0u, 0u, 0u, 0u};
    const RtDepositCount none{0u, 0u, 0u, 0u};
    RtParticleState* d_ring = (RtParticleState*)run.on_device(nullptr, (size_t)capacity * sizeof(RtParticleState));
    RtEmitCursor* d_cursor = (RtEmitCursor*)run.on_device(&zero, sizeof zero);
    RtParticle* d_draw = (RtParticle*)run.on_device(nullptr, (size_t)capacity * sizeof(RtParticle));
    RtDepositCount* d_counts = (RtDepositCount*)run.on_device(&none, sizeof none);
    const RtProbeLight* d_light = (const RtProbeLight*)run.on_device(&light, sizeof light);
    run.start();

    // ---- the device path -------------------------------------------------------------------------------------------------------
    RtEmitCursor after{};
    run.fine = run.fine && rt_draw_frame(s.ctx, &s.u()) == RT_OK &&
               rt_emit_particles_async(s.ctx, &e, 1, lr, d_ring, capacity, capacity, d_cursor) == RT_OK && rt_edit_shapes(s.ctx, &carve, 1) == RT_OK &&
               rt_sync(s.ctx) == RT_OK && hip.copy(&after, d_cursor, sizeof after, 2 /* hipMemcpyDeviceToHost */) == 0;
    const uint32_t live = after.emitted;
    double step_ms = 0.0, deposit_ms = 0.0, draw_ms = 0.0;
    for (int t = 0; t < ticks && run.fine && live; t++) {
        float ms[3] = {0.0f, 0.0f, 0.0f};
        run.fine = run.mark() && rt_step_particles_async(s.ctx, &step, d_ring, d_ring, d_draw, live) == RT_OK && run.lap(&ms[0]) &&
                   run.mark() && rt_deposit_particles_async(s.ctx, &dep, d_ring, d_draw, live, d_counts) == RT_OK && run.lap(&ms[1]) &&
                   run.mark() && rt_draw_particles_async(s.ctx, &s.u(), d_draw, live, d_light, 1) == RT_OK && run.lap(&ms[2]);
        step_ms += (double)ms[0] / ticks; deposit_ms += (double)ms[1] / ticks; draw_ms += (double)ms[2] / ticks;
    }
    RtDepositCount counts{};
    run.fine = run.fine && rt_sync(s.ctx) == RT_OK && hip.copy(&counts, d_counts, sizeof counts, 2) == 0;

    // ---- the host path, on the region as it was ----------------------------------------------------------------------------------
    run.fine = run.fine && rt_edit_stamps(s.ctx, &back, 1) == RT_OK && hip.copy(d_cursor, &zero, sizeof zero, 1) == 0 &&
               rt_emit_particles_async(s.ctx, &e, 1, lr, d_ring, capacity, capacity, d_cursor) == RT_OK && rt_edit_shapes(s.ctx, &carve, 1) == RT_OK &&
               rt_sync(s.ctx) == RT_OK;
    std::vector<RtParticleState> ring(live);
    const size_t nvox = (size_t)ext[0] * ext[1] * ext[2];
    std::vector<uint8_t> box_mine(nvox);
    std::vector<uint32_t> claim(nvox);
    std::vector<RtVoxelEdit> edits;
    uint64_t host_voxels = 0, host_deposited = 0;
    double host_ms = 0.0;
    for (int t = 0; t < ticks && run.fine && live; t++) {
        run.fine = rt_step_particles_async(s.ctx, &step, d_ring, d_ring, d_draw, live) == RT_OK && rt_sync(s.ctx) == RT_OK;
        const auto t0 = std::chrono::steady_clock::now();
        run.fine = run.fine && hip.copy(ring.data(), d_ring, (size_t)live * sizeof(RtParticleState), 2) == 0 &&
                   rt_read_box(s.ctx, lo[0], lo[1], lo[2], ext[0], ext[1], ext[2], nullptr, box_mine.data()) == RT_OK;
        std::fill(claim.begin(), claim.end(), UINT32_MAX);
        edits.clear();
        for (uint32_t i = 0; i < live && run.fine; i++) {
            RtParticleState& p = ring[i];
            if ((p.flags & (RT_PSTATE_DEAD | RT_PSTATE_INVALID)) != 0u || (p.flags & RT_PSTATE_CONTACT) == 0u) continue;
            bool ok = true;
            int x[3];
            for (int a = 0; a < 3 && ok; a++) {
                ok = std::fabs(p.velocity[a]) <= dep.max_speed && std::fabs(p.lo[a]) <= 4194304.0f && std::fabs(p.hi[a]) <= 4194304.0f;
                if (!ok) break;
                const int v = (int)std::floor((p.lo[a] + p.hi[a]) * 0.5f);
                ok = v >= lr[a] - R / 2 && v < lr[a] + R / 2;
                x[a] = (v + R / 2) & (R - 1);
                ok = ok && x[a] >= dep.lo[a] && x[a] <= dep.hi[a];
            }
            if (!ok) continue;
            const size_t at = ((size_t)(x[2] - lo[2]) * ext[1] + (size_t)(x[1] - lo[1])) * ext[0] + (size_t)(x[0] - lo[0]);
            if (box_mine[at] == 0u) continue;
            p.flags |= RT_PSTATE_DEAD;
            host_deposited++;
            if (claim[at] != UINT32_MAX) continue;                     // (ascending i: the first is the lowest index)
            claim[at] = i;
            RtVoxelEdit ed{};
            ed.x = (uint16_t)x[0]; ed.y = (uint16_t)x[1]; ed.z = (uint16_t)x[2]; ed.solid = 1; ed.material = p.material;
            edits.push_back(ed);
        }
        host_voxels += edits.size();
        run.fine = run.fine && rt_edit_voxels(s.ctx, edits.data(), (uint32_t)edits.size()) == RT_OK &&
                   hip.copy(d_ring, ring.data(), (size_t)live * sizeof(RtParticleState), 1) == 0;
        host_ms += ms_since(t0) / ticks;
    }
    if (run.fine) run.fine = rt_sync(s.ctx) == RT_OK && rt_stamp_destroy(s.ctx, undo) == RT_OK;
    if (!run.close()) { std::fprintf(stderr, "settle failed: %s\n", rt_last_error(s.ctx)); return 1; }
    // the host path restates the rules: it is a baseline only while it deposits what the library deposits
    if (host_voxels != counts.voxels || host_deposited != counts.deposited) {
        std::fprintf(stderr, "settle: the host path deposited %llu particles into %llu voxels, the device %u into %u\n", (unsigned long long)host_deposited,
                     (unsigned long long)host_voxels, counts.deposited, counts.voxels);
        return 1;
    }
    const double tick_ms = step_ms + deposit_ms + draw_ms;
    std::printf("{\"debris\": %d, \"settle\": %d, \"density\": %d, \"centre\": [%d, %d, %d], \"deposit_box\": [%d, %d, %d], \"particles\": %u, "
                "\"frame\": \"%dx%d spp %d depth %d\", \"deposited\": %u, \"voxels\": %u, \"occupied\": %u, \"outside\": %u, \"host_voxels\": %llu, "
                "\"step_device_ms\": %.4f, \"deposit_device_ms\": %.4f, \"draw_device_ms\": %.4f, \"tick_device_ms\": %.4f, \"deposit_share\": %.3f, "
                "\"host_path_ms\": %.3f}\n",
                radius, ticks, o.debris_density, c[0], c[1], c[2], ext[0], ext[1], ext[2], live, o.width, o.height, o.spp, o.depth, counts.deposited,
                counts.voxels, counts.occupied, counts.outside, (unsigned long long)host_voxels, step_ms, deposit_ms, draw_ms, tick_ms,
                tick_ms > 0.0 ? deposit_ms / tick_ms : 0.0, host_ms);
    return 0;
}

// --debris RADIUS --settle T --fall K [--density D]: voxel settling.  --settle's explosion and its T ticks of step and deposit, then a slab
// four texels thick is carved under the crater across the whole deposit box (rt_edit_shapes), so that the rubble and the ground over
// the slab hang in the air, and FALL_TICKS ticks of rt_settle_voxels_async run with max_fall = K over the deposit box (every occupied
// voxel loose, down z), each between events of its own, with no host read.  Then the box is put back as it was after the carve (a
// stamp) and the same ticks run with the host path the call replaces, call to usable device state: the box read back (rt_read_box,
// words and minefield), the columns walked in C++ by the header's rule, one RtVoxelEdit record per source and per target,
// rt_edit_voxels.  The mode fails if the host path's moved or distance differ from the device's counts.
constexpr int FALL_TICKS = 8;
int run_fall(const Options& o, const World& w) {
    Session s;
    if (!open_session(&s, o, w, RT_FLAG_TIMING_ALL)) return 1;
    const HipEvents hip;
    if (!hip.ok) { std::fprintf(stderr, "--fall needs the HIP runtime for its device buffers\n"); return 1; }
    const int radius = o.debris, ticks = o.settle;
    const int32_t* lr = s.u().lr;
    DebrisPile pile;
    int rc = make_debris_pile(o, s, &pile);
    if (rc != RT_OK) return s.fail("fall", rc);
    const int32_t (&lo)[3] = pile.lo, (&ext)[3] = pile.ext;
    const uint32_t capacity = 1u << 20;
    RtShapeEdit slab{};
    for (int a = 0; a < 3; a++) { slab.a[a] = lo[a]; slab.b[a] = lo[a] + ext[a] - 1; }
    slab.b[2] = pile.c[2] - radius - 2 < lo[2] + 4 ? lo[2] + 4 : pile.c[2] - radius - 2;
    slab.a[2] = slab.b[2] - 3;
    slab.kind = RT_SHAPE_BOX; slab.where = RT_WHERE_ALL; slab.solid = 0;
    RtVoxelSettle fall{};
    for (int a = 0; a < 3; a++) { fall.lo[a] = lo[a]; fall.hi[a] = lo[a] + ext[a] - 1; }
    fall.max_fall = (uint32_t)o.fall; fall.axis = 2; fall.toward = 0;

    DeviceRun run(hip, s.ctx);
    const RtEmitCursor zero{0u, 0u, 0u, 0u};
    const RtSettleCount none{0u, 0u, 0u, 0u};
    RtParticleState* d_ring = (RtParticleState*)run.on_device(nullptr, (size_t)capacity * sizeof(RtParticleState));
    RtEmitCursor* d_cursor = (RtEmitCursor*)run.on_device(&zero, sizeof zero);
    RtSettleCount* d_counts = (RtSettleCount*)run.on_device(&none, sizeof none);
    run.start();

    // ---- the pile: emit, carve, T ticks of step and deposit, then the slab under it ------------------------------------------------
    RtEmitCursor after{};
    run.fine = run.fine && rt_emit_particles_async(s.ctx, &pile.e, 1, lr, d_ring, capacity, capacity, d_cursor) == RT_OK &&
               rt_edit_shapes(s.ctx, &pile.carve, 1) == RT_OK && rt_sync(s.ctx) == RT_OK && hip.copy(&after, d_cursor, sizeof after, 2) == 0;
    const uint32_t live = after.emitted;
    for (int t = 0; t < ticks && run.fine && live; t++)
        run.fine = rt_step_particles_async(s.ctx, &pile.step, d_ring, d_ring, nullptr, live) == RT_OK &&
                   rt_deposit_particles_async(s.ctx, &pile.dep, d_ring, nullptr, live, nullptr) == RT_OK;
    uint32_t undo = 0;
    run.fine = run.fine && rt_edit_shapes(s.ctx, &slab, 1) == RT_OK && rt_stamp_capture(s.ctx, lo, ext, 0u, &undo) == RT_OK;
    RtStampPlace back{};
    for (int a = 0; a < 3; a++) back.at[a] = lo[a];
    back.stamp = undo; back.where = RT_WHERE_ALL;

    // ---- the device path -------------------------------------------------------------------------------------------------------
    double settle_ms = 0.0;
    for (int t = 0; t < FALL_TICKS && run.fine; t++) {
        float ms = 0.0f;
        run.fine = run.mark() && rt_settle_voxels_async(s.ctx, &fall, d_counts) == RT_OK && run.lap(&ms);
        settle_ms += (double)ms / FALL_TICKS;
    }
    RtSettleCount counts{};
    run.fine = run.fine && rt_sync(s.ctx) == RT_OK && hip.copy(&counts, d_counts, sizeof counts, 2) == 0;

    // ---- the host path, on the box as it was after the slab was carved -----------------------------------------------------------
    run.fine = run.fine && rt_edit_stamps(s.ctx, &back, 1) == RT_OK && rt_sync(s.ctx) == RT_OK;
    const size_t nvox = (size_t)ext[0] * ext[1] * ext[2], plane = (size_t)ext[0] * ext[1];
    std::vector<uint8_t> box_mine(nvox);
    std::vector<uint32_t> box_mats(nvox);
    std::vector<RtVoxelEdit> edits;
    uint64_t host_moved = 0, host_distance = 0, host_records = 0;
    double host_ms = 0.0;
    for (int t = 0; t < FALL_TICKS && run.fine; t++) {
        const auto t0 = std::chrono::steady_clock::now();
        run.fine = rt_read_box(s.ctx, lo[0], lo[1], lo[2], ext[0], ext[1], ext[2], box_mats.data(), box_mine.data()) == RT_OK;
        edits.clear();
        for (size_t col = 0; col < plane && run.fine; col++) {
            uint32_t gap = 0;   // unoccupied cells under the cell (every occupied voxel is loose: no fixed cell restarts it)
            for (int h = 0; h < ext[2]; h++) {
                const size_t at = (size_t)h * plane + col;
                if (box_mine[at] != 0u) { gap++; continue; }
                const uint32_t drop = gap < fall.max_fall ? gap : fall.max_fall;
                if (drop == 0u) continue;
                host_moved++; host_distance += drop;
                RtVoxelEdit ed{};
                ed.x = (uint16_t)(lo[0] + (int)(col % (size_t)ext[0])); ed.y = (uint16_t)(lo[1] + (int)(col / (size_t)ext[0])); ed.z = (uint16_t)(lo[2] + h);
                ed.solid = 0; ed.material = fall.air_material;
                edits.push_back(ed);                                   // the source; a later voxel's target may fill it again
                ed.z = (uint16_t)(lo[2] + h - (int)drop); ed.solid = 1; ed.material = box_mats[at];
                edits.push_back(ed);
            }
        }
        host_records += edits.size();
        run.fine = run.fine && rt_edit_voxels(s.ctx, edits.data(), (uint32_t)edits.size()) == RT_OK && rt_sync(s.ctx) == RT_OK;
        host_ms += ms_since(t0) / FALL_TICKS;
    }
    if (run.fine) run.fine = rt_stamp_destroy(s.ctx, undo) == RT_OK;
    if (!run.close()) { std::fprintf(stderr, "fall failed: %s\n", rt_last_error(s.ctx)); return 1; }
    // the host path restates the rule: it is a baseline only while it moves what the library moves
    if (host_moved != counts.moved || host_distance != counts.distance) {
        std::fprintf(stderr, "fall: the host path moved %llu voxels by %llu cells, the device %u by %u\n", (unsigned long long)host_moved,
                     (unsigned long long)host_distance, counts.moved, counts.distance);
        return 1;
    }
    std::printf("{\"debris\": %d, \"settle\": %d, \"fall\": %u, \"ticks\": %d, \"density\": %d, \"box\": [%d, %d, %d], \"slab_z\": [%d, %d], \"particles\": %u, "
                "\"moved\": %u, \"falling\": %u, \"distance\": %u, \"chunks\": %u, \"host_moved\": %llu, \"host_distance\": %llu, \"host_records\": %llu, "
                "\"settle_device_ms\": %.4f, \"host_path_ms\": %.3f}\n",
                radius, ticks, fall.max_fall, FALL_TICKS, o.debris_density, ext[0], ext[1], ext[2], slab.a[2], slab.b[2], live, counts.moved, counts.falling,
                counts.distance, counts.chunks, (unsigned long long)host_moved, (unsigned long long)host_distance, (unsigned long long)host_records,
                settle_ms, host_ms);
    return 0;
}

// --collapse RADIUS: voxel detachment.  Under the texel at the frame's centre a block of RADIUS x RADIUS texels' footprint is cut
// out of the terrain: a slab four texels thick RADIUS texels below the surface and four trenches two texels wide round the footprint, up to
// 32 texels over the surface (rt_edit_shapes), so that a body of about RADIUS^3 voxels hangs free.  The detach box is the footprint grown by
// six texels from under the slab to the trenches' top; every face but the top anchors.  The timed call, COLLAPSE_REPS times between
// events of its own with the box put back as it was after the carve (a stamp) in front of each: rt_detach_voxels_async with
// RT_DETACH_CARVE | RT_DETACH_CAPTURE, then one rt_draw_stamps of the result into the frame drawn before.  Then the same with the host path
// the call replaces, call to usable device state: the box read back (rt_read_box, words and minefield), a flood fill in C++ from the
// anchors, one RtVoxelEdit record per detached voxel, rt_edit_voxels, rt_stamp_create from host arrays and the same draw.  The mode fails
// unless both paths detach the same voxels with the same words.
constexpr int COLLAPSE_REPS = 4;
int run_collapse(const Options& o, const World& w) {
    Session s;
    if (!open_session(&s, o, w, RT_FLAG_TIMING_ALL)) return 1;
    const HipEvents hip;
    if (!hip.ok) { std::fprintf(stderr, "--collapse needs the HIP runtime for its device buffers\n"); return 1; }
    const int R = RT_ROOT_BLOCK_SIZE, radius = o.collapse;
    const int32_t* lr = s.u().lr;
    const int32_t centre_px[2] = {o.width / 2, o.height / 2};
    RtRayHit hit{};
    int rc = rt_pick_pixels(s.ctx, &s.u(), centre_px, 1, &hit);
    if (rc != RT_OK) return s.fail("collapse", rc);
    int c[3] = {R / 2, R / 2, R / 2};
    if (hit.kind == RT_HIT_SOLID) for (int a = 0; a < 3; a++) c[a] = hit.texel[a];
    auto clamp = [R](int v) { return v < 0 ? 0 : v > R - 1 ? R - 1 : v; };
    // the footprint f0..f1 (x, y), the slab's z range, the trenches' top and the detach box
    int f0[2], f1[2];
    for (int a = 0; a < 2; a++) { f0[a] = clamp(c[a] - radius / 2); f1[a] = clamp(f0[a] + radius - 1); }
    const int slab_hi = clamp(c[2] - radius), slab_lo = clamp(slab_hi - 3), top = clamp(c[2] + 32);
    RtVoxelDetach det{};
    for (int a = 0; a < 2; a++) { det.lo[a] = clamp(f0[a] - 6); det.hi[a] = clamp(f1[a] + 6); }
    det.lo[2] = clamp(slab_lo - 2); det.hi[2] = top;
    det.flags = RT_DETACH_CARVE | RT_DETACH_CAPTURE; det.max_passes = 32; det.anchor_faces = 0x1F;
    int32_t lo[3], ext[3];
    for (int a = 0; a < 3; a++) { lo[a] = det.lo[a]; ext[a] = det.hi[a] - det.lo[a] + 1; }
    RtShapeEdit cuts[5] = {};
    for (RtShapeEdit& e : cuts) {
        e.kind = RT_SHAPE_BOX; e.where = RT_WHERE_ALL; e.solid = 0;
        e.a[0] = clamp(f0[0] - 2); e.a[1] = clamp(f0[1] - 2); e.a[2] = slab_lo;
        e.b[0] = clamp(f1[0] + 2); e.b[1] = clamp(f1[1] + 2); e.b[2] = top;
    }
    cuts[0].b[2] = slab_hi;                                   // the slab; then the trenches at low x, high x, low y, high y
    cuts[1].b[0] = cuts[1].a[0] + 1; cuts[2].a[0] = cuts[2].b[0] - 1; cuts[3].b[1] = cuts[3].a[1] + 1; cuts[4].a[1] = cuts[4].b[1] - 1;

    uint32_t undo = 0;
    rc = rt_edit_shapes(s.ctx, cuts, 5);
    if (rc == RT_OK) rc = rt_stamp_capture(s.ctx, lo, ext, 0u, &undo);
    // the body is drawn one texel above where it was, lit by one probe at the block's centre
    RtProbeLight light{};
    const float centre[3] = {(float)(lr[0] - R / 2 + c[0]) + 0.5f, (float)(lr[1] - R / 2 + c[1]) + 0.5f, (float)(lr[2] - R / 2 + top) + 0.5f};
    const RtLightProbe probe = sphere_probe(0, centre);
    if (rc == RT_OK) rc = rt_probe_light(s.ctx, &s.u(), &probe, 1, 4, 2, &light);
    if (rc != RT_OK) return s.fail("collapse", rc);
    const RtProbeLight faces[6] = {light, light, light, light, light, light};
    RtStampPlace back{};
    for (int a = 0; a < 3; a++) back.at[a] = lo[a];
    back.stamp = undo; back.where = RT_WHERE_ALL;
    RtDrawStamp model{};
    for (int a = 0; a < 3; a++) model.origin[a] = (float)(lr[a] - R / 2 + lo[a]);
    model.origin[2] += 1.0f; model.scale = 1.0f; model.emission = 0xFF000000u;

    DeviceRun run(hip, s.ctx);
    RtDetachResult none{};
    for (int a = 0; a < 3; a++) { none.lo[a] = INT32_MAX; none.hi[a] = INT32_MIN; }
    RtDetachResult* d_result = (RtDetachResult*)run.on_device(&none, sizeof none);
    run.start();

    // ---- the device path -------------------------------------------------------------------------------------------------------
    const size_t nvox = (size_t)ext[0] * ext[1] * ext[2];
    std::vector<uint32_t> dev_mats(nvox), host_mats(nvox, 0u);
    std::vector<uint8_t> dev_state(nvox), host_state(nvox, (uint8_t)RT_STAMP_ABSENT);
    RtDetachResult result{};
    double device_ms = 0.0;
    for (int t = 0; t < COLLAPSE_REPS + 1 && run.fine; t++) {   // (the first warms the scratch and the staging up)
        uint32_t body = 0;
        float ms = 0.0f;
        run.fine = hip.copy(d_result, &none, sizeof none, 1) == 0 && rt_edit_stamps(s.ctx, &back, 1) == RT_OK && rt_draw_frame(s.ctx, &s.u()) == RT_OK &&
                   run.mark() && rt_detach_voxels_async(s.ctx, &det, d_result, &body) == RT_OK;
        if (run.fine) {
            model.stamp = body;
            run.fine = rt_draw_stamps(s.ctx, &s.u(), &model, faces, 1) == RT_OK && run.lap(&ms);
        }
        if (t > 0) device_ms += (double)ms / COLLAPSE_REPS;
        if (run.fine && t == COLLAPSE_REPS)
            run.fine = rt_sync(s.ctx) == RT_OK && hip.copy(&result, d_result, sizeof result, 2) == 0 &&
                       rt_stamp_read(s.ctx, body, dev_mats.data(), dev_state.data()) == RT_OK;
        if (run.fine) run.fine = rt_stamp_destroy(s.ctx, body) == RT_OK;
    }

    // ---- the host path, on the box as it was after the carve ---------------------------------------------------------------------
    std::vector<uint8_t> box_mine(nvox), reached(nvox);
    std::vector<uint32_t> box_mats(nvox), queue;
    std::vector<RtVoxelEdit> edits;
    uint64_t host_detached = 0;
    double host_ms = 0.0;
    const size_t sx = 1, sy = (size_t)ext[0], sz = (size_t)ext[0] * ext[1];
    for (int t = 0; t < COLLAPSE_REPS && run.fine; t++) {
        run.fine = rt_edit_stamps(s.ctx, &back, 1) == RT_OK && rt_draw_frame(s.ctx, &s.u()) == RT_OK && rt_sync(s.ctx) == RT_OK;
        const auto t0 = std::chrono::steady_clock::now();
        run.fine = run.fine && rt_read_box(s.ctx, lo[0], lo[1], lo[2], ext[0], ext[1], ext[2], box_mats.data(), box_mine.data()) == RT_OK;
        std::fill(reached.begin(), reached.end(), (uint8_t)0);
        queue.clear();
        for (int z = 0; z < ext[2]; z++)                       // the anchors: occupied cells of every face but the top
            for (int y = 0; y < ext[1]; y++)
                for (int x = 0; x < ext[0]; x++) {
                    if (!(x == 0 || x == ext[0] - 1 || y == 0 || y == ext[1] - 1 || z == 0)) continue;
                    const size_t at = z * sz + y * sy + x * sx;
                    if (box_mine[at] == 0u) { reached[at] = 1; queue.push_back((uint32_t)at); }
                }
        for (size_t head = 0; head < queue.size(); head++) {
            const size_t at = queue[head];
            const int x = (int)(at % sy), y = (int)(at / sy % (size_t)ext[1]), z = (int)(at / sz);
            const size_t next[6] = {at - sx, at + sx, at - sy, at + sy, at - sz, at + sz};
            const bool inside[6] = {x > 0, x < ext[0] - 1, y > 0, y < ext[1] - 1, z > 0, z < ext[2] - 1};
            for (int k = 0; k < 6; k++)
                if (inside[k] && box_mine[next[k]] == 0u && !reached[next[k]]) { reached[next[k]] = 1; queue.push_back((uint32_t)next[k]); }
        }
        edits.clear();
        std::fill(host_mats.begin(), host_mats.end(), 0u);
        std::fill(host_state.begin(), host_state.end(), (uint8_t)RT_STAMP_ABSENT);
        for (size_t at = 0; at < nvox; at++) {
            if (box_mine[at] != 0u || reached[at]) continue;
            RtVoxelEdit ed{};
            ed.x = (uint16_t)(lo[0] + (int)(at % sy)); ed.y = (uint16_t)(lo[1] + (int)(at / sy % (size_t)ext[1])); ed.z = (uint16_t)(lo[2] + (int)(at / sz));
            ed.solid = 0; ed.material = det.air_material;
            edits.push_back(ed);
            host_mats[at] = box_mats[at];
            host_state[at] = (uint8_t)RT_STAMP_SOLID;
        }
        host_detached = edits.size();
        uint32_t body = 0;
        run.fine = run.fine && rt_edit_voxels(s.ctx, edits.data(), (uint32_t)edits.size()) == RT_OK &&
                   rt_stamp_create(s.ctx, ext, host_mats.data(), host_state.data(), &body) == RT_OK;
        if (run.fine) {
            model.stamp = body;
            run.fine = rt_draw_stamps(s.ctx, &s.u(), &model, faces, 1) == RT_OK && rt_sync(s.ctx) == RT_OK;
        }
        host_ms += ms_since(t0) / COLLAPSE_REPS;
        if (run.fine) run.fine = rt_stamp_destroy(s.ctx, body) == RT_OK;
    }
    if (run.fine) run.fine = rt_stamp_destroy(s.ctx, undo) == RT_OK;
    if (!run.close()) { std::fprintf(stderr, "collapse failed: %s\n", rt_last_error(s.ctx)); return 1; }
    // the host path restates the rule: it is a baseline only while it detaches what the library detaches
    if (host_detached != result.detached || result.unconverged != 0u || dev_state != host_state || dev_mats != host_mats) {
        std::fprintf(stderr, "collapse: the host path detached %llu voxels, the device %u (unconverged %u); the stamps %s\n", (unsigned long long)host_detached,
                     result.detached, result.unconverged, dev_state == host_state && dev_mats == host_mats ? "agree" : "differ");
        return 1;
    }
    std::printf("{\"collapse\": %d, \"centre\": [%d, %d, %d], \"box\": [%d, %d, %d], \"slab_z\": [%d, %d], \"frame\": \"%dx%d spp %d depth %d\", "
                "\"detached\": %u, \"supported\": %u, \"passes\": %u, \"chunks\": %u, \"bounds\": [%d, %d, %d, %d, %d, %d], \"host_detached\": %llu, "
                "\"detach_device_ms\": %.4f, \"host_path_ms\": %.3f}\n",
                radius, c[0], c[1], c[2], ext[0], ext[1], ext[2], slab_lo, slab_hi, o.width, o.height, o.spp, o.depth, result.detached, result.supported,
                result.passes, result.chunks, result.lo[0], result.lo[1], result.lo[2], result.hi[0], result.hi[1], result.hi[2],
                (unsigned long long)host_detached, device_ms, host_ms);
    return 0;
}

// --flood EXTENT [--ticks K]: fluid flow.  A box of EXTENT x EXTENT x min(EXTENT, 128) texels round the column under the frame's centre,
// its top layer eight texels over the highest voxel of its footprint, with a row of sources along one top edge (rt_edit_voxels).  rt_flow_voxels_async with K ticks a call runs until a call adds 0 to `active`,
// or FLOOD_CALLS times, each call between events of its own; the counts come back after every call, as a host that wants to stop needs
// them.  Then the box is put back as it was (a stamp) and the same calls run with the host path the call replaces, call to usable
// device state: the box read back (rt_read_box, words and minefield), the header's rule in C++ for K ticks, one RtVoxelEdit per cell
// whose occupancy or word changed, rt_edit_voxels.  The mode fails unless both paths leave equal box bytes.  One JSON line.
constexpr int FLOOD_CALLS = 64;
namespace {
constexpr uint32_t FLOOD_WORD = 0x40A0E0C0u, FLOOD_MASK = 0xFFFFFFF0u, FLOOD_LEVEL = 7u;   // a blue albedo; the level in the low nibble
// one tick of the header's rule over states [z][y][x] (0 empty, 1..13 a strength, 14 source, 15 fixed); returns the cells that changed
uint64_t flood_tick(const std::vector<uint8_t>& in, std::vector<uint8_t>* out, const int32_t ext[3], uint32_t max_level) {
    const int ex = ext[0], ey = ext[1], ez = ext[2];
    auto at = [&](int x, int y, int z) -> uint32_t {
        return x < 0 || y < 0 || z < 0 || x >= ex || y >= ey || z >= ez ? 15u : in[((size_t)z * ey + y) * ex + x];
    };
    uint64_t changed = 0;
    for (int z = 0; z < ez; z++)
        for (int y = 0; y < ey; y++)
            for (int x = 0; x < ex; x++) {
                const size_t i = ((size_t)z * ey + y) * ex + x;
                const uint32_t s = in[i];
                uint32_t ns = s;
                if (s < 14u) {
                    const uint32_t up = at(x, y, z + 1);
                    ns = up >= 1u && up <= 14u ? max_level : 0u;
                    const int dx[4] = {-1, 1, 0, 0}, dy[4] = {0, 0, -1, 1};
                    for (int k = 0; k < 4; k++) {
                        const uint32_t n = at(x + dx[k], y + dy[k], z);
                        if (n < 1u || n > 14u) continue;
                        if (n != 14u && at(x + dx[k], y + dy[k], z - 1) != 15u) continue;   // not spreading
                        const uint32_t e1 = n == 14u ? max_level : n - 1u;
                        if (e1 > ns) ns = e1;
                    }
                }
                (*out)[i] = (uint8_t)ns;
                changed += ns != s;
            }
    return changed;
}
}  // namespace

int run_flood(const Options& o, const World& w) {
    Session s;
    if (!open_session(&s, o, w, RT_FLAG_TIMING_ALL)) return 1;
    const HipEvents hip;
    if (!hip.ok) { std::fprintf(stderr, "--flood needs the HIP runtime for its device buffers\n"); return 1; }
    const int R = RT_ROOT_BLOCK_SIZE, E = o.flood, EZ = E < 128 ? E : 128;
    const int32_t centre_px[2] = {o.width / 2, o.height / 2};
    RtRayHit hit{};
    int rc = rt_pick_pixels(s.ctx, &s.u(), centre_px, 1, &hit);
    if (rc != RT_OK) return s.fail("flood", rc);
    int c[3] = {R / 2, R / 2, R / 2};
    if (hit.kind == RT_HIT_SOLID) for (int a = 0; a < 3; a++) c[a] = hit.texel[a];
    auto clamp = [](int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; };
    const int32_t ext[3] = {E, E, EZ};
    int32_t lo[3] = {clamp(c[0] - E / 2, R - E), clamp(c[1] - E / 2, R - E), 0};
    {   // the box's top layer lies eight texels over the highest voxel of its footprint, so that the springs stand in the air
        std::vector<uint8_t> column((size_t)E * E * R);
        rc = rt_read_box(s.ctx, lo[0], lo[1], 0, E, E, R, nullptr, column.data());
        if (rc != RT_OK) return s.fail("flood", rc);
        int top = 0;
        for (size_t i = 0; i < column.size(); i++)
            if (column[i] == 0u) top = (int)(i / ((size_t)E * E));
        lo[2] = clamp(top + 8 - (EZ - 1), R - EZ);
    }
    RtVoxelFlow flow{};
    for (int a = 0; a < 3; a++) { flow.lo[a] = lo[a]; flow.hi[a] = lo[a] + ext[a] - 1; }
    flow.ticks = (uint32_t)(o.flood_ticks ? o.flood_ticks : 8); flow.air_material = 0u; flow.fluid_mask = FLOOD_MASK; flow.fluid_value = FLOOD_WORD; flow.fluid_word = FLOOD_WORD;
    flow.level_shift = 0; flow.max_level = (uint8_t)FLOOD_LEVEL;
    // the springs: a row of sources along the box's top edge at x = lo
    std::vector<RtVoxelEdit> springs((size_t)E);
    for (int y = 0; y < E; y++) {
        RtVoxelEdit& ed = springs[(size_t)y];
        ed = RtVoxelEdit{};
        ed.x = (uint16_t)lo[0]; ed.y = (uint16_t)(lo[1] + y); ed.z = (uint16_t)(lo[2] + EZ - 1); ed.solid = 1; ed.material = FLOOD_WORD | 0xFu;
    }
    uint32_t undo = 0;
    rc = rt_edit_voxels(s.ctx, springs.data(), (uint32_t)springs.size());
    if (rc == RT_OK) rc = rt_stamp_capture(s.ctx, lo, ext, 0u, &undo);
    if (rc != RT_OK) return s.fail("flood", rc);
    RtStampPlace back{};
    for (int a = 0; a < 3; a++) back.at[a] = lo[a];
    back.stamp = undo; back.where = RT_WHERE_ALL;

    DeviceRun run(hip, s.ctx);
    const RtFlowCount none{};
    RtFlowCount* d_counts = (RtFlowCount*)run.on_device(&none, sizeof none);
    run.start();

    // ---- the device path -------------------------------------------------------------------------------------------------------
    const size_t nvox = (size_t)ext[0] * ext[1] * ext[2];
    RtFlowCount counts{};
    double flow_ms = 0.0, first_ms = 0.0;
    int calls = 0;
    for (; calls < FLOOD_CALLS && run.fine; calls++) {
        float ms = 0.0f;
        const uint32_t before = counts.active;
        run.fine = run.mark() && rt_flow_voxels_async(s.ctx, &flow, d_counts) == RT_OK && run.lap(&ms) && hip.copy(&counts, d_counts, sizeof counts, 2) == 0;
        flow_ms += (double)ms;
        if (calls == 0) first_ms = (double)ms;
        if (counts.active == before) { calls++; break; }
    }
    std::vector<uint32_t> dev_mats(nvox), host_mats(nvox);
    std::vector<uint8_t> dev_mine(nvox), host_mine(nvox);
    run.fine = run.fine && rt_read_box(s.ctx, lo[0], lo[1], lo[2], ext[0], ext[1], ext[2], dev_mats.data(), dev_mine.data()) == RT_OK;

    // ---- the host path, on the box as it was ----------------------------------------------------------------------------------------
    run.fine = run.fine && rt_edit_stamps(s.ctx, &back, 1) == RT_OK && rt_sync(s.ctx) == RT_OK;
    std::vector<uint8_t> st0(nvox), st1(nvox), start(nvox);
    std::vector<RtVoxelEdit> edits;
    uint64_t host_records = 0, host_active = 1;
    double host_ms = 0.0;
    int host_calls = 0;
    for (; host_calls < calls && run.fine; host_calls++) {
        const auto t0 = std::chrono::steady_clock::now();
        run.fine = rt_read_box(s.ctx, lo[0], lo[1], lo[2], ext[0], ext[1], ext[2], host_mats.data(), host_mine.data()) == RT_OK;
        for (size_t i = 0; i < nvox; i++) {
            const uint32_t wd = host_mats[i], v = wd & 0xFu;
            st0[i] = host_mine[i] != 0u ? 0u : (wd & FLOOD_MASK) != FLOOD_WORD ? 15u : v == 15u ? 14u : (uint8_t)(v < FLOOD_LEVEL ? v : FLOOD_LEVEL);
        }
        start = st0;
        for (uint32_t t = 0; t < flow.ticks; t++) { flood_tick(st0, &st1, ext, FLOOD_LEVEL); st0.swap(st1); }
        host_active = flood_tick(st0, &st1, ext, FLOOD_LEVEL);
        edits.clear();
        for (size_t i = 0; i < nvox; i++) {
            const bool occupied = host_mine[i] == 0u, flowing0 = occupied && start[i] < 14u, flows = st0[i] >= 1u && st0[i] <= 13u;
            RtVoxelEdit ed{};
            ed.x = (uint16_t)(lo[0] + (int)(i % (size_t)ext[0])); ed.y = (uint16_t)(lo[1] + (int)(i / (size_t)ext[0] % (size_t)ext[1]));
            ed.z = (uint16_t)(lo[2] + (int)(i / ((size_t)ext[0] * ext[1])));
            if (flows) {
                ed.solid = 1; ed.material = ((flowing0 ? host_mats[i] : FLOOD_WORD) & ~0xFu) | st0[i];
                if (occupied && ed.material == host_mats[i]) continue;
            } else if (flowing0) {
                ed.solid = 0; ed.material = flow.air_material;
            } else continue;
            edits.push_back(ed);
        }
        host_records += edits.size();
        run.fine = run.fine && rt_edit_voxels(s.ctx, edits.data(), (uint32_t)edits.size()) == RT_OK && rt_sync(s.ctx) == RT_OK;
        host_ms += ms_since(t0);
    }
    run.fine = run.fine && rt_read_box(s.ctx, lo[0], lo[1], lo[2], ext[0], ext[1], ext[2], host_mats.data(), host_mine.data()) == RT_OK;
    if (run.fine) run.fine = rt_stamp_destroy(s.ctx, undo) == RT_OK;
    if (!run.close()) { std::fprintf(stderr, "flood failed: %s\n", rt_last_error(s.ctx)); return 1; }
    // the host path restates the rule: it is a baseline only while it leaves what the library leaves
    if (dev_mats != host_mats || dev_mine != host_mine) {
        std::fprintf(stderr, "flood: after %d calls the words %s and the minefield %s\n", calls, dev_mats == host_mats ? "agree" : "differ",
                     dev_mine == host_mine ? "agree" : "differ");
        return 1;
    }
    std::printf("{\"flood\": %d, \"ticks\": %u, \"lo\": [%d, %d, %d], \"box\": [%d, %d, %d], \"calls\": %d, \"at_rest\": %d, \"wetted\": %u, \"dried\": %u, "
                "\"changed\": %u, \"chunks\": %u, \"host_records\": %llu, \"first_call_device_ms\": %.4f, \"flow_device_ms\": %.4f, \"host_path_ms\": %.3f}\n",
                E, flow.ticks, lo[0], lo[1], lo[2], ext[0], ext[1], ext[2], calls, host_active == 0u ? 1 : 0, counts.wetted, counts.dried, counts.changed,
                counts.chunks, (unsigned long long)host_records, first_ms, calls ? flow_ms / calls : 0.0, calls ? host_ms / calls : 0.0);
    return 0;
}

// --navigate EXTENT [--agents N]: navigation fields.  A field of EXTENT x EXTENT x 128 cells round the texel at the frame's centre
// is built towards that texel's column (goal records nine apart with goal_snap 8 cover it) with max_dist 2 EXTENT, and N agents
// scattered over the box are sampled; build and sample run between events of their own, NAV_REPS times.  Beside it the host path,
// timed from the call to usable device state: rt_read_box of the box's minefield, the same search and sample in C++, an upload of the
// steps.  The mode fails unless both give the same dist, move and step bytes.  One JSON line.
constexpr int NAV_REPS = 10;
int run_navigate(const Options& o, const World& w) {
    Session s;
    if (!open_session(&s, o, w, RT_FLAG_TIMING_ALL)) return 1;
    const HipEvents hip;
    if (!hip.ok) { std::fprintf(stderr, "--navigate needs the HIP runtime for its device buffers\n"); return 1; }
    const int R = RT_ROOT_BLOCK_SIZE, E = o.navigate, EZ = 128;
    const int32_t centre_px[2] = {o.width / 2, o.height / 2};
    RtRayHit hit{};
    int rc = rt_pick_pixels(s.ctx, &s.u(), centre_px, 1, &hit);
    if (rc != RT_OK) return s.fail("navigate", rc);
    int c[3] = {R / 2, R / 2, R / 2};
    if (hit.kind == RT_HIT_SOLID) for (int a = 0; a < 3; a++) c[a] = hit.texel[a];
    auto clamp = [](int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; };
    const int32_t ext[3] = {E, E, EZ};
    RtNavBuild p{};
    p.lo[0] = clamp(c[0] - E / 2, R - E); p.lo[1] = clamp(c[1] - E / 2, R - E); p.lo[2] = clamp(c[2] - EZ / 2, R - EZ);
    p.max_dist = 2u * (uint32_t)E; p.height = 2; p.max_climb = 1; p.max_drop = 3; p.goal_snap = 8;
    std::vector<RtNavGoal> goals;
    for (int z = 8; z < EZ + 8; z += 9) { RtNavGoal g{}; g.cell[0] = c[0]; g.cell[1] = c[1]; g.cell[2] = p.lo[2] + (z < EZ ? z : EZ - 1); goals.push_back(g); }
    const uint32_t nagents = (uint32_t)o.agents;
    std::vector<RtNavAgent> agents(nagents);
    uint32_t seed = 12345u;
    auto next = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (RtNavAgent& a : agents) {
        a.pos[0] = (float)p.lo[0] + (float)(next() % (uint32_t)(E * 16)) / 16.0f;
        a.pos[1] = (float)p.lo[1] + (float)(next() % (uint32_t)(E * 16)) / 16.0f;
        a.pos[2] = (float)p.lo[2] + (float)(next() % (uint32_t)(EZ * 16)) / 16.0f;
        a.snap_down = 8; a.snap_up = 2;
    }
    uint32_t field = 0;
    rc = rt_nav_create(s.ctx, ext, &field);
    if (rc != RT_OK) return s.fail("navigate", rc);

    DeviceRun run(hip, s.ctx);
    const RtNavResult none{};
    RtNavResult* d_result = (RtNavResult*)run.on_device(&none, sizeof none);
    RtNavGoal* d_goals = (RtNavGoal*)run.on_device(goals.data(), goals.size() * sizeof(RtNavGoal));
    RtNavAgent* d_agents = (RtNavAgent*)run.on_device(agents.data(), (size_t)nagents * sizeof(RtNavAgent));
    RtNavStep* d_steps = (RtNavStep*)run.on_device(nullptr, (size_t)nagents * sizeof(RtNavStep));
    RtNavStep* d_host_steps = (RtNavStep*)run.on_device(nullptr, (size_t)nagents * sizeof(RtNavStep));
    run.start();

    // ---- the device path -------------------------------------------------------------------------------------------------------
    const size_t ncell = (size_t)E * E * EZ;
    double build_ms = 0.0, sample_ms = 0.0;
    for (int t = 0; t < NAV_REPS + 1 && run.fine; t++) {   // (the first warms up)
        float ms = 0.0f;
        run.fine = hip.copy(d_result, &none, sizeof none, 1) == 0 && run.mark() &&
                   rt_nav_build_async(s.ctx, field, &p, d_goals, (uint32_t)goals.size(), d_result) == RT_OK && run.lap(&ms);
        if (t > 0) build_ms += (double)ms / NAV_REPS;
        if (run.fine && nagents > 0u) {
            run.fine = run.mark() && rt_nav_sample_async(s.ctx, field, d_agents, nagents, d_steps) == RT_OK && run.lap(&ms);
            if (t > 0) sample_ms += (double)ms / NAV_REPS;
        }
    }
    RtNavResult result{};
    std::vector<uint16_t> dev_dist(ncell), host_dist(ncell);
    std::vector<uint8_t> dev_move(ncell), host_move(ncell);
    std::vector<RtNavStep> dev_steps(nagents), host_steps(nagents);
    if (run.fine)
        run.fine = rt_sync(s.ctx) == RT_OK && hip.copy(&result, d_result, sizeof result, 2) == 0 && rt_nav_read(s.ctx, field, dev_dist.data(), dev_move.data()) == RT_OK &&
                   (nagents == 0u || hip.copy(dev_steps.data(), d_steps, (size_t)nagents * sizeof(RtNavStep), 2) == 0);

    // ---- the host path: read the box back, search and sample in C++, send the steps -----------------------------------------------
    std::vector<uint8_t> mine(ncell), clear(ncell), stand(ncell);
    std::vector<uint32_t> queue;
    const int sy = E, sz = E * E, H = p.height;
    const int dxs[4] = {1, -1, 0, 0}, dys[4] = {0, 0, 1, -1};
    double host_ms = 0.0;
    for (int t = 0; t < NAV_REPS && run.fine; t++) {
        const auto t0 = std::chrono::steady_clock::now();
        run.fine = rt_read_box(s.ctx, p.lo[0], p.lo[1], p.lo[2], E, E, EZ, nullptr, mine.data()) == RT_OK;
        for (int z = EZ - 1; z >= 0; z--)
            for (int i = 0; i < sz; i++) {
                const size_t at = (size_t)z * sz + i;
                const int above = z + 1 < EZ ? clear[at + sz] : 255;
                clear[at] = mine[at] == 0u ? 0 : (uint8_t)(above < 255 ? above + 1 : 255);
                stand[at] = mine[at] != 0u && (z == 0 || mine[at - sz] == 0u) && clear[at] >= H;
            }
        std::fill(host_dist.begin(), host_dist.end(), (uint16_t)0xFFFF);
        std::fill(host_move.begin(), host_move.end(), (uint8_t)0xFF);
        queue.clear();
        for (const RtNavGoal& g : goals) {
            const int x = g.cell[0] - p.lo[0], y = g.cell[1] - p.lo[1];
            if (x < 0 || x >= E || y < 0 || y >= E) continue;
            for (int k = 0; k <= p.goal_snap; k++) {
                const int z = g.cell[2] - p.lo[2] - k;
                if (z < 0) break;
                if (z >= EZ) continue;
                const size_t at = (size_t)z * sz + (size_t)y * sy + x;
                if (!stand[at]) continue;
                if (host_dist[at] != 0) { host_dist[at] = 0; queue.push_back((uint32_t)at); }
                break;
            }
        }
        // the move a -> b with b = a + (dx, dy, k): both standable and the lower of the two clear for |k| + height cells
        auto move_ok = [&](size_t a, size_t b, int k) { return stand[a] && stand[b] && clear[k >= 0 ? a : b] >= (k < 0 ? -k : k) + H; };
        for (size_t head = 0; head < queue.size(); head++) {
            const size_t b = queue[head];
            const int bx = (int)(b % (size_t)sy), by = (int)(b / (size_t)sy % (size_t)E), bz = (int)(b / (size_t)sz);
            if (host_dist[b] >= p.max_dist) continue;
            for (int h = 0; h < 4; h++) {
                const int ax = bx - dxs[h], ay = by - dys[h];
                if (ax < 0 || ax >= E || ay < 0 || ay >= E) continue;
                for (int k = -(int)p.max_drop; k <= (int)p.max_climb; k++) {
                    const int az = bz - k;
                    if (az < 0 || az >= EZ) continue;
                    const size_t a = (size_t)az * sz + (size_t)ay * sy + ax;
                    if (host_dist[a] != 0xFFFF || !move_ok(a, b, k)) continue;
                    host_dist[a] = (uint16_t)(host_dist[b] + 1);
                    queue.push_back((uint32_t)a);
                }
            }
        }
        for (const uint32_t a : queue) {
            const int d = host_dist[a];
            if (d == 0) continue;
            const int ax = (int)(a % (size_t)sy), ay = (int)(a / (size_t)sy % (size_t)E), az = (int)(a / (size_t)sz);
            for (int h = 0; h < 4 && host_move[a] == 0xFF; h++) {
                const int bx = ax + dxs[h], by = ay + dys[h];
                if (bx < 0 || bx >= E || by < 0 || by >= E) continue;
                for (int k = (int)p.max_climb; k >= -(int)p.max_drop; k--) {
                    const int bz = az + k;
                    if (bz < 0 || bz >= EZ) continue;
                    const size_t b = (size_t)bz * sz + (size_t)by * sy + bx;
                    if (host_dist[b] != d - 1 || !move_ok(a, b, k)) continue;
                    host_move[a] = (uint8_t)(h | ((k + 8) << 2));
                    break;
                }
            }
        }
        for (uint32_t i = 0; i < nagents; i++) {
            const RtNavAgent& a = agents[i];
            RtNavStep st{};
            const int c0[3] = {(int)std::floor(a.pos[0]), (int)std::floor(a.pos[1]), (int)std::floor(a.pos[2])};
            for (int k = 0; k < 3; k++) st.cell[k] = st.next[k] = c0[k];
            st.dist = 0xFFFFFFFFu; st.move = 0xFFu;
            const int x = c0[0] - p.lo[0], y = c0[1] - p.lo[1];
            for (int j = 0; j <= a.snap_down + a.snap_up && x >= 0 && x < E && y >= 0 && y < E; j++) {
                const int z = c0[2] - p.lo[2] + (j <= a.snap_down ? -j : j - a.snap_down);
                if (z < 0 || z >= EZ) continue;
                const size_t at = (size_t)z * sz + (size_t)y * sy + x;
                if (host_dist[at] == 0xFFFF) continue;
                st.dist = host_dist[at];
                st.cell[2] = st.next[2] = z + p.lo[2];
                if (st.dist > 0u) {
                    st.move = host_move[at];
                    st.next[0] += dxs[st.move & 3u]; st.next[1] += dys[st.move & 3u]; st.next[2] += (int)(st.move >> 2) - 8;
                }
                break;
            }
            host_steps[i] = st;
        }
        run.fine = run.fine && (nagents == 0u || hip.copy(d_host_steps, host_steps.data(), (size_t)nagents * sizeof(RtNavStep), 1) == 0);
        host_ms += ms_since(t0) / NAV_REPS;
    }
    if (run.fine) run.fine = rt_nav_destroy(s.ctx, field) == RT_OK;
    if (!run.close()) { std::fprintf(stderr, "navigate failed: %s\n", rt_last_error(s.ctx)); return 1; }
    // the host path restates the rules: it is a baseline only while it gives what the library gives
    const bool same_steps = nagents == 0u || std::memcmp(dev_steps.data(), host_steps.data(), (size_t)nagents * sizeof(RtNavStep)) == 0;
    if (dev_dist != host_dist || dev_move != host_move || !same_steps) {
        std::fprintf(stderr, "navigate: dist %s, move %s, steps %s\n", dev_dist == host_dist ? "agree" : "differ", dev_move == host_move ? "agree" : "differ",
                     same_steps ? "agree" : "differ");
        return 1;
    }
    std::printf("{\"navigate\": %d, \"agents\": %u, \"centre\": [%d, %d, %d], \"lo\": [%d, %d, %d], \"max_dist\": %u, \"standable\": %u, \"reached\": %u, "
                "\"levels\": %u, \"truncated\": %u, \"goals_used\": %u, \"build_device_ms\": %.4f, \"sample_device_ms\": %.4f, \"host_path_ms\": %.3f, "
                "\"equal_bytes\": true}\n",
                E, nagents, c[0], c[1], c[2], p.lo[0], p.lo[1], p.lo[2], p.max_dist, result.standable, result.reached, result.levels, result.truncated,
                result.goals_used, build_ms, sample_ms, host_ms);
    return 0;
}

// --models N [--model-scale S]: voxel-model entities.  One built-in 9 x 9 x 12 sparse stamp (about a third of its voxels solid; its
// values are the generator's first) is drawn N times at scale S (default 1/8) — scattered like --boxes' boxes, in seeded
// orientations, lit by their bounding boxes' face probes — by rt_draw_stamps into a freshly drawn --width x --height frame, 20 times;
// and, as a yardstick in the same process, rt_draw_boxes draws the bounding boxes of the same records, 20 times.  One JSON line: the
// device time of both passes, their ratio, the call-to-return time of rt_draw_stamps and the pixels drawn.
int run_models(const Options& o, const World& w) {
    Session s;
    if (!open_session(&s, o, w, RT_FLAG_TIMING_ALL)) return 1;
    const uint32_t n = (uint32_t)o.models;
    SparseStamp stamp = sparse_stamp(s.rnd, 9, 9, 12);
    if (!s.create_stamp(&stamp)) return 1;
    std::vector<RtDrawStamp> models(n);
    std::vector<RtDrawBox> boxes(n);
    std::vector<RtLightProbe> probes(6u * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        float c[3];
        scatter_point(s.u(), s.rnd, 20.0f, c);
        models[i] = model_at(stamp, o.model_scale, i, c, &boxes[i]);
        boxes[i].material = stamp.mats[0]; boxes[i].emission = models[i].emission;
        face_probes(boxes[i], i, &probes[6u * (size_t)i]);
    }
    std::vector<RtProbeLight> lights(probes.size());
    int rc = n ? rt_probe_light(s.ctx, &s.u(), probes.data(), (uint32_t)probes.size(), 4, 2, lights.data()) : RT_OK;
    const size_t npix = (size_t)o.width * (size_t)o.height;
    std::vector<float> before(npix), after(npix);
    if (rc == RT_OK) rc = s.read_plane(RT_BUF_DEPTH_F32, &before);
    PassTime pt[2];
    uint64_t drawn[2] = {0, 0};
    for (int pass = 0; pass < 2 && rc == RT_OK; pass++) {       // 0: the models, 1: their bounding boxes
        rc = timed_pass(s, rc, &pt[pass], [&] {
            return pass == 0 ? rt_draw_stamps(s.ctx, &s.u(), models.data(), lights.data(), n) : rt_draw_boxes(s.ctx, &s.u(), boxes.data(), lights.data(), n);
        });
        if (rc == RT_OK) rc = s.read_plane(RT_BUF_DEPTH_F32, &after);
        drawn[pass] = changed_pixels(before, after, 1);
    }
    if (rc != RT_OK) return s.fail("voxel-model entities", rc);
    std::printf("{\"models\": %u, \"model_scale\": %g, \"frame\": \"%dx%d spp %d depth %d\", \"draw_stamps_device_ms\": %.4f, "
                "\"bounding_boxes_device_ms\": %.4f, \"ratio\": %.2f, \"draw_stamps_call_ms\": %.4f, \"draw_boxes_call_ms\": %.4f, "
                "\"pixels_drawn\": %llu, \"bounding_box_pixels\": %llu}\n",
                n, (double)o.model_scale, o.width, o.height, o.spp, o.depth, pt[0].device_ms, pt[1].device_ms,
                pt[1].device_ms > 0.0 ? pt[0].device_ms / pt[1].device_ms : 0.0, pt[0].call_ms, pt[1].call_ms, (unsigned long long)drawn[0],
                (unsigned long long)drawn[1]);
    return 0;
}

// n seeded pixels and what they show (rt_pick_pixels): where --lights, --shadows and --light-shadows put their records
struct Picks {
    std::vector<int32_t> xy;
    std::vector<RtRayHit> hits;
};
static int pick_pixels(Session& s, uint32_t n, Picks* out) {
    out->xy = pixel_list(s.view, s.rnd, n);
    out->hits.resize(n);
    return n ? rt_pick_pixels(s.ctx, &s.u(), out->xy.data(), n, out->hits.data()) : RT_OK;
}

// --lights N: point lights.  N lights of radius 8 are scattered deterministically just off visible surfaces — rt_pick_pixels on N
// pixels spread over the view, each light 1 to 4 units off its hit point along the face's normal (30 units along the ray where the
// pixel shows sky) — and rt_add_lights adds them to a freshly drawn --width x --height frame, 20 times.  One JSON line: the device
// time of the pass, the call-to-return time of rt_add_lights and the pixels lit.
int run_lights(const Options& o, const World& w) {
    Session s;
    if (!open_session(&s, o, w, RT_FLAG_TIMING_ALL)) return 1;
    const uint32_t n = (uint32_t)o.lights;
    Picks picks;
    int rc = pick_pixels(s, n, &picks);
    if (rc != RT_OK) return s.fail("point lights", rc);
    const std::vector<RtPointLight> lights = lights_off_hits(s.view, s.rnd, picks.xy, picks.hits);
    std::vector<float> before(4u * (size_t)o.width * (size_t)o.height), after(before.size());
    PassTime pt;
    rc = timed_pass(s, rc, &pt, [&] { return rt_add_lights(s.ctx, &s.u(), lights.data(), n); },
                    [&] { return s.read_plane(RT_BUF_LIGHTING_F32, &before); });
    if (rc == RT_OK) rc = s.read_plane(RT_BUF_LIGHTING_F32, &after);
    if (rc != RT_OK) return s.fail("point lights", rc);
    std::printf("{\"lights\": %u, \"frame\": \"%dx%d spp %d depth %d\", \"add_lights_device_ms\": %.4f, \"add_lights_call_ms\": %.4f, "
                "\"launches_per_call\": %.2f, \"pixels_lit\": %llu}\n",
                n, o.width, o.height, o.spp, o.depth, pt.device_ms, pt.call_ms, (double)pt.launches / PASS_REPS,
                (unsigned long long)changed_pixels(before, after, 4));
    return 0;
}

// --shadows N [--shadow-models [--model-scale S]]: entity shadows.  N occluders stand 0.5 to 6 units above what N random pixels show
// — player-sized boxes, or with --shadow-models the 9 x 9 x 12 stamp of --models at scale S in the 48 orientations in turn — and
// rt_shadow_entities shades a freshly drawn --width x --height frame with them, 20 times.  (The stamp's values are the generator's
// first, with or without --shadow-models; the pixels follow.)  As yardsticks in the same process rt_draw_boxes draws the same boxes
// (the models' bounding boxes) and rt_add_lights adds as many lights (at most 1024) at the occluders' centres.  One JSON line: the
// device time of each launch, the call-to-return time of rt_shadow_entities and the pixels it changed.
int run_shadows(const Options& o, const World& w) {
    Session s;
    if (!open_session(&s, o, w, RT_FLAG_TIMING_ALL)) return 1;
    const uint32_t n = (uint32_t)o.shadows;
    const bool as_models = o.shadow_models;
    SparseStamp stamp = sparse_stamp(s.rnd, 9, 9, 12);
    if (as_models && !s.create_stamp(&stamp)) return 1;
    Picks picks;
    int rc = pick_pixels(s, n, &picks);
    std::vector<RtDrawBox> boxes(n);
    std::vector<RtDrawStamp> models(as_models ? n : 0u);
    const uint32_t nlights = std::min(n, 1024u);
    std::vector<RtPointLight> lights(nlights);
    for (uint32_t i = 0; i < n && rc == RT_OK; i++) {
        float c[3];
        if (picks.hits[i].kind == RT_HIT_SOLID) {
            for (int a = 0; a < 3; a++) c[a] = picks.hits[i].position[a];
            c[2] += 0.5f + 5.5f * s.rnd();
        } else {
            pixel_point(s.view, &picks.xy[2u * i], 30.0f, c);
        }
        if (as_models) models[i] = model_at(stamp, o.model_scale, i, c, &boxes[i]);
        else player_box(c, &boxes[i]);
        boxes[i].material = material_word(i); boxes[i].emission = 0xFF000000u;
        if (i < nlights) {
            RtPointLight& l = lights[i];
            l = RtPointLight{};
            for (int a = 0; a < 3; a++) { l.position[a] = c[a]; l.color[a] = 20.0f; }
            l.radius = 8.0f;
        }
    }
    std::vector<float> before(4u * (size_t)o.width * (size_t)o.height), after(before.size());
    std::vector<RtProbeLight> face(6u * (size_t)n);
    for (RtProbeLight& f : face) { f = RtProbeLight{}; f.light[0] = f.light[1] = f.light[2] = 8.0f; }
    PassTime pt[3];   // 0: the shadows; the yardsticks: 1 rt_draw_boxes of the same boxes, 2 rt_add_lights of as many lights
    rc = timed_pass(s, rc, &pt[0], [&] { return rt_shadow_entities(s.ctx, &s.u(), as_models ? nullptr : boxes.data(), as_models ? 0u : n, models.data(), as_models ? n : 0u, 1.0f); },
                    [&] { return s.read_plane(RT_BUF_LIGHTING_F32, &before); });
    if (rc == RT_OK) rc = s.read_plane(RT_BUF_LIGHTING_F32, &after);
    rc = timed_pass(s, rc, &pt[1], [&] { return rt_draw_boxes(s.ctx, &s.u(), boxes.data(), face.data(), n); });
    rc = timed_pass(s, rc, &pt[2], [&] { return rt_add_lights(s.ctx, &s.u(), lights.data(), nlights); });
    if (rc != RT_OK) return s.fail("entity shadows", rc);
    std::printf("{\"shadows\": %u, \"shadow_models\": %d, \"model_scale\": %g, \"frame\": \"%dx%d spp %d depth %d\", \"shadow_entities_device_ms\": %.4f, "
                "\"shadow_entities_call_ms\": %.4f, \"launches_per_call\": %.2f, \"draw_boxes_device_ms\": %.4f, \"add_lights_device_ms\": %.4f, "
                "\"add_lights_count\": %u, \"pixels_changed\": %llu}\n",
                n, as_models ? 1 : 0, (double)o.model_scale, o.width, o.height, o.spp, o.depth, pt[0].device_ms, pt[0].call_ms,
                (double)pt[0].launches / PASS_REPS, pt[1].device_ms, pt[2].device_ms, nlights, (unsigned long long)changed_pixels(before, after, 4));
    return 0;
}

// --light-shadows [--lights N] [--boxes B] [--models M]: point-light shadows of entities.  --lights' N lights (64 without --lights),
// built first, so that the two runs light the same frame; then the models' stamp (5 x 4 x 6, at --model-scale, the 48 orientations
// in turn), then the occluders' centres — B player-sized boxes first, the M models from index B — each within --occluder-spread
// units (3) of a light, in turn, or, with --occluders-far, 400 units above it, where no segment of the frame passes.
// rt_add_lights_occluded lights a freshly drawn frame with them 20 times, then rt_add_lights does as the yardstick.  One JSON line:
// device time and call-to-return time of both, and the pixels the entities changed.
int run_light_shadows(const Options& o, const World& w) {
    Session s;
    if (!open_session(&s, o, w, RT_FLAG_TIMING_ALL)) return 1;
    const uint32_t nlights = (uint32_t)(o.lights < 0 ? 64 : o.lights), nboxes = (uint32_t)std::max(o.boxes, 0ll), nmodels = (uint32_t)std::max(o.models, 0ll);
    Picks picks;
    int rc = pick_pixels(s, nlights, &picks);
    if (rc != RT_OK) return s.fail("point-light shadows", rc);
    const std::vector<RtPointLight> lights = lights_off_hits(s.view, s.rnd, picks.xy, picks.hits);
    SparseStamp stamp = sparse_stamp(s.rnd, 5, 4, 6);
    if (nmodels && !s.create_stamp(&stamp)) return 1;
    auto centre = [&](uint32_t i, float c[3]) {
        const float* at = nlights ? lights[i % nlights].position : s.u().origin;   // (--lights 0: round the camera)
        for (int a = 0; a < 3; a++) c[a] = at[a] + o.occluder_spread * (2.0f * s.rnd() - 1.0f);
        if (o.occluders_far) c[2] += 400.0f;
    };
    std::vector<RtDrawBox> boxes(nboxes);   // (their material stays 0: a shadow has none)
    for (uint32_t i = 0; i < nboxes; i++) {
        float c[3];
        centre(i, c);
        player_box(c, &boxes[i]);
        boxes[i].emission = 0xFF000000u;
    }
    std::vector<RtDrawStamp> models(nmodels);
    for (uint32_t i = 0; i < nmodels; i++) {
        float c[3];
        centre(i + nboxes, c);
        models[i] = model_at(stamp, o.model_scale, i, c, nullptr);
    }
    std::vector<float> plain(4u * (size_t)o.width * (size_t)o.height), shaded(plain.size());
    PassTime pt[2];   // 0: rt_add_lights_occluded; the yardstick: 1 rt_add_lights of the same lights
    rc = timed_pass(s, rc, &pt[0], [&] { return rt_add_lights_occluded(s.ctx, &s.u(), lights.data(), nlights, boxes.data(), nboxes, models.data(), nmodels); });
    if (rc == RT_OK) rc = s.read_plane(RT_BUF_LIGHTING_F32, &shaded);
    rc = timed_pass(s, rc, &pt[1], [&] { return rt_add_lights(s.ctx, &s.u(), lights.data(), nlights); });
    if (rc == RT_OK) rc = s.read_plane(RT_BUF_LIGHTING_F32, &plain);
    if (rc != RT_OK) return s.fail("point-light shadows", rc);
    std::printf("{\"light_shadows\": %u, \"boxes\": %u, \"models\": %u, \"model_scale\": %g, \"spread\": %g, \"far\": %d, \"frame\": \"%dx%d spp %d depth %d\", "
                "\"add_lights_occluded_device_ms\": %.4f, \"add_lights_occluded_call_ms\": %.4f, \"launches_per_call\": %.2f, "
                "\"add_lights_device_ms\": %.4f, \"add_lights_call_ms\": %.4f, \"pixels_shadowed\": %llu}\n",
                nlights, nboxes, nmodels, (double)o.model_scale, (double)o.occluder_spread, o.occluders_far ? 1 : 0, o.width, o.height, o.spp, o.depth,
                pt[0].device_ms, pt[0].call_ms, (double)pt[0].launches / PASS_REPS, pt[1].device_ms, pt[1].call_ms,
                (unsigned long long)changed_pixels(plain, shaded, 4));
    return 0;
}

}  // namespace bench
