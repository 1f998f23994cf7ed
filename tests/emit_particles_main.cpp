// emit_particles_main.cpp — the host half of rt_emit_particles (raytrace_amd/csrc/api/emit_check.hpp) as a program of its own, built
// with the address and undefined-behaviour sanitizers by tests/test_emit_particles_host.py.
//
//     emit_particles_main RECORDS LOGR [BATCH ...]
//
// RECORDS is a file of RtParticleEmit records (the table of tests/emit_particles_sets.py, written by the test); a BATCH is a
// comma-separated list of indices into it.  The program prints one line "verdicts 1011..." with emitter_valid's answer per record,
// "first_invalid K", one line "plan B: items N; emitter blo.x blo.y blo.z nbx nby nbz first; ..." per batch, the windows' verdicts,
// the cursor's, the ring runs and one line per case of emit_args_error; the test holds them against tests/emit_particles_ref.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytrace_amd/csrc/api/emit_check.hpp"

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s RECORDS LOGR [BATCH ...]\n", argv[0]); return 2; }
    const int logr = std::atoi(argv[2]);
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<RtParticleEmit> recs;
    RtParticleEmit one;
    while (std::fread(&one, sizeof one, 1, fp) == 1) recs.push_back(one);
    std::fclose(fp);
    static_assert(sizeof(RtParticleEmit) == 96 && sizeof(RtEmitCursor) == 16, "the records are 96 and 16 bytes");

    std::printf("records %zu\nverdicts ", recs.size());
    for (const RtParticleEmit& e : recs) std::putchar(rta::emitter_valid(e, 1 << logr) ? '1' : '0');
    const uint32_t bad = rta::first_invalid_emitter(recs.data(), (uint32_t)recs.size(), logr);
    std::printf("\nfirst_invalid %u\n", bad);
    bool prefixes = rta::first_invalid_emitter(nullptr, 0, logr) == 0u;
    for (uint32_t n = 0; n <= bad; n++) prefixes = prefixes && rta::first_invalid_emitter(recs.data(), n, logr) == n;
    std::printf("prefixes %d\n", prefixes ? 1 : 0);

    for (int b = 3; b < argc; b++) {
        std::vector<RtParticleEmit> batch;
        for (const char* p = argv[b]; *p;) {
            char* end;
            batch.push_back(recs.at(std::strtoul(p, &end, 10)));
            p = *end ? end + 1 : end;
        }
        const rta::EmitPlan plan = rta::emit_plan(batch.data(), (uint32_t)batch.size(), logr);
        std::printf("plan %d: items %llu", b - 3, (unsigned long long)plan.items);
        for (const rta::EmitRecord& r : plan.recs) {
            uint32_t which = 0;   // the record's emitter, by its bytes
            while (std::memcmp(&batch[which], &r.e, sizeof r.e) != 0) which++;
            std::printf("; %u %u %u %u %u %u %u %u", which, r.blo[0], r.blo[1], r.blo[2], r.nbx, r.nby, r.nbz, r.first);
        }
        std::printf("\n");
    }
    {   // five emitters over the whole region: more bricks than a call takes
        RtParticleEmit whole{};
        whole.b[0] = whole.b[1] = whole.b[2] = (1 << logr) - 1;
        const std::vector<RtParticleEmit> five(5, whole);
        const rta::EmitPlan plan = rta::emit_plan(five.data(), 5, logr);
        std::printf("whole items %llu limit %u\n", (unsigned long long)plan.items, rta::kMaxEmitBricks);
    }

    const int32_t edge = (1 << 22) - (1 << logr);
    const int32_t windows[][3] = {{0, 0, 0}, {edge, -edge, 0}, {edge + 1, 0, 0}, {0, 0, -edge - 1}, {0, INT32_MIN, 0}};
    std::printf("windows ");
    for (const auto& w : windows) std::putchar(rta::emit_window_valid(w, logr) ? '1' : '0');
    std::printf("\ncursors %d%d%d%d\n", rta::emit_cursor_valid(RtEmitCursor{0, 0, 0, 0}, 1), rta::emit_cursor_valid(RtEmitCursor{63, 9, 9, 0}, 64),
                rta::emit_cursor_valid(RtEmitCursor{64, 0, 0, 0}, 64), rta::emit_cursor_valid(RtEmitCursor{3, 0, 0, 1}, 64));
    const uint32_t rings[][3] = {{60, 60, 64}, {0, 64, 64}, {5, 0, 64}, {63, 1, 64}, {63, 2, 64}, {10, 20, 64}};
    for (const auto& r : rings) {
        rta::EmitRun runs[2];
        const uint32_t n = rta::emit_ring_runs(r[0], r[1], r[2], runs);
        std::printf("runs %u %u %u:", r[0], r[1], r[2]);
        for (uint32_t i = 0; i < n; i++) std::printf(" %u+%u@%u", runs[i].slot, runs[i].count, runs[i].first);
        std::printf("\n");
    }

    // the plain arguments
    const int a = 0;
    struct { const char* name; const char* verdict; } cases[] = {
        {"fine", rta::emit_args_error(&a, 1, &a, &a, 64, 64, &a)},
        {"empty", rta::emit_args_error(nullptr, 0, nullptr, nullptr, 0, 0, nullptr)},
        {"at the limits", rta::emit_args_error(&a, 256, &a, &a, 1u << 20, 1u << 20, &a)},
        {"null emitters", rta::emit_args_error(nullptr, 1, &a, &a, 64, 64, &a)},
        {"null lr", rta::emit_args_error(&a, 1, nullptr, &a, 64, 64, &a)},
        {"null states", rta::emit_args_error(&a, 1, &a, nullptr, 64, 64, &a)},
        {"null cursor", rta::emit_args_error(&a, 1, &a, &a, 64, 64, nullptr)},
        {"count beyond", rta::emit_args_error(&a, 257, &a, &a, 64, 64, &a)},
        {"capacity beyond", rta::emit_args_error(&a, 1, &a, &a, (1u << 20) + 1u, 64, &a)},
        {"capacity 0", rta::emit_args_error(&a, 1, &a, &a, 0, 0, &a)},
        {"max_emit 0", rta::emit_args_error(&a, 1, &a, &a, 64, 0, &a)},
        {"max_emit beyond", rta::emit_args_error(&a, 1, &a, &a, 64, 65, &a)},
    };
    for (const auto& c : cases) std::printf("args %s: %s\n", c.name, c.verdict ? c.verdict : "ok");
    return 0;
}
