// particle_step_main.cpp — the host half of rt_step_particles (raytrace_amd/csrc/api/particle_step_check.hpp) as a program of its
// own, built with the address and undefined-behaviour sanitizers by tests/test_particle_step_host.py.
//
//     particle_step_main RECORDS PARAMS
//
// RECORDS is a file of RtParticleState records and PARAMS one of RtParticleStep records (the tables of tests/particle_step_sets.py,
// written by the test).  The program prints one line "verdicts viv..." with v = valid, i = invalid, x = inactive per record, one
// line "first_invalid K" with first_invalid_particle_state's answer, one line "params 10..." with whether
// particle_step_params_error accepts each parameter record, and one line per case of particle_step_args_error; the test holds them
// against tests/particle_step_ref.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytrace_amd/csrc/api/particle_step_check.hpp"

template <typename T>
static bool read_all(const char* path, std::vector<T>& out) {
    FILE* fp = std::fopen(path, "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", path); return false; }
    T one;
    while (std::fread(&one, sizeof one, 1, fp) == 1) out.push_back(one);
    std::fclose(fp);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s RECORDS PARAMS\n", argv[0]); return 2; }
    static_assert(sizeof(RtParticleState) == 64 && sizeof(RtParticleStep) == 48, "the records are 64 and 48 bytes");
    std::vector<RtParticleState> recs;
    std::vector<RtParticleStep> params;
    if (!read_all(argv[1], recs) || !read_all(argv[2], params)) return 2;

    std::printf("records %zu\nverdicts ", recs.size());
    for (const RtParticleState& s : recs) std::putchar(rta::particle_state_inactive(s) ? 'x' : (rta::particle_state_valid(s) ? 'v' : 'i'));
    const uint32_t bad = rta::first_invalid_particle_state(recs.data(), (uint32_t)recs.size());
    std::printf("\nfirst_invalid %u\n", bad);

    // every batch that ends before the first invalid record is valid; an empty batch reads nothing
    bool prefixes = rta::first_invalid_particle_state(nullptr, 0) == 0u;
    for (uint32_t n = 0; n <= bad; n++) prefixes = prefixes && rta::first_invalid_particle_state(recs.data(), n) == n;
    std::printf("prefixes %d\n", prefixes ? 1 : 0);

    std::printf("params ");
    for (const RtParticleStep& p : params) std::putchar(rta::particle_step_params_error(p) ? '0' : '1');
    std::putchar('\n');

    // the plain arguments: 8 states of 64 bytes and their 8 draw records of 32 in one block
    alignas(16) static unsigned char block[4096];
    const RtParticleStep p{};
    unsigned char* a = block;
    struct { const char* name; const char* verdict; } cases[] = {
        {"fine", rta::particle_step_args_error(&p, a, a + 1024, a + 2048, 8)},
        {"in place", rta::particle_step_args_error(&p, a, a, a + 2048, 8)},
        {"no draw", rta::particle_step_args_error(&p, a, a + 512, nullptr, 8)},
        {"empty", rta::particle_step_args_error(nullptr, nullptr, nullptr, nullptr, 0)},
        {"null params", rta::particle_step_args_error(nullptr, a, a + 1024, nullptr, 8)},
        {"null in", rta::particle_step_args_error(&p, nullptr, a + 1024, nullptr, 8)},
        {"null out", rta::particle_step_args_error(&p, a, nullptr, nullptr, 8)},
        {"count at the limit", rta::particle_step_args_error(&p, a, a, nullptr, 1u << 20)},
        {"count beyond", rta::particle_step_args_error(&p, a, a, nullptr, (1u << 20) + 1u)},
        {"out one record into in", rta::particle_step_args_error(&p, a, a + 64, nullptr, 8)},
        {"in one record into out", rta::particle_step_args_error(&p, a + 64, a, nullptr, 8)},
        {"out just behind in", rta::particle_step_args_error(&p, a, a + 512, nullptr, 8)},
        {"draw inside in", rta::particle_step_args_error(&p, a, a + 1024, a + 256, 8)},
        {"draw reaches into out", rta::particle_step_args_error(&p, a, a + 1024, a + 1024 - 16, 8)},
        {"draw just in front of in", rta::particle_step_args_error(&p, a + 256, a + 1024, a, 8)},
    };
    for (const auto& c : cases) std::printf("args %s: %s\n", c.name, c.verdict ? c.verdict : "ok");
    return 0;
}
