// draw_particles_main.cpp — the host half of rt_draw_particles (raytrace_amd/csrc/api/particles_check.hpp) as a program of its own,
// built with the address and undefined-behaviour sanitizers by tests/test_draw_particles_host.py.
//
//     draw_particles_main RECORDS NLIGHTS
//
// RECORDS is a file of RtParticle records (the table of tests/draw_particles_sets.py, written by the test).  The program prints one
// line "verdicts 1011..." with particle_valid's answer per record, one line "first_invalid K" with first_invalid_particle's, and
// one line per case of particle_args_error; the test holds them against tests/draw_particles_ref.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytrace_amd/csrc/api/particles_check.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s RECORDS NLIGHTS\n", argv[0]); return 2; }
    const uint32_t nlights = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<RtParticle> recs;
    RtParticle one;
    while (std::fread(&one, sizeof one, 1, fp) == 1) recs.push_back(one);
    std::fclose(fp);
    static_assert(sizeof(RtParticle) == 32, "the record is 32 bytes");

    std::printf("records %zu\nverdicts ", recs.size());
    for (const RtParticle& p : recs) std::putchar(rta::particle_valid(p, nlights) ? '1' : '0');
    std::printf("\nfirst_invalid %u\n", rta::first_invalid_particle(recs.data(), (uint32_t)recs.size(), nlights));

    // every batch that ends before the first invalid record is valid; an empty batch reads nothing
    const uint32_t bad = rta::first_invalid_particle(recs.data(), (uint32_t)recs.size(), nlights);
    bool prefixes = rta::first_invalid_particle(nullptr, 0, nlights) == 0u;
    for (uint32_t n = 0; n <= bad; n++) prefixes = prefixes && rta::first_invalid_particle(recs.data(), n, nlights) == n;
    std::printf("prefixes %d\n", prefixes ? 1 : 0);

    // the plain arguments
    const int u = 0, a = 0;
    struct { const char* name; const char* verdict; } cases[] = {
        {"fine", rta::particle_args_error(&u, &a, 3, &a, 1)},
        {"empty", rta::particle_args_error(&u, nullptr, 0, nullptr, 0)},
        {"null uniforms", rta::particle_args_error(nullptr, &a, 3, &a, 1)},
        {"null particles", rta::particle_args_error(&u, nullptr, 3, &a, 1)},
        {"null lights", rta::particle_args_error(&u, &a, 3, nullptr, 1)},
        {"no lights", rta::particle_args_error(&u, &a, 3, &a, 0)},
        {"count at the limit", rta::particle_args_error(&u, &a, 1u << 20, &a, 1u << 20)},
        {"count beyond", rta::particle_args_error(&u, &a, (1u << 20) + 1u, &a, 1)},
        {"lights beyond", rta::particle_args_error(&u, &a, 3, &a, (1u << 20) + 1u)},
    };
    for (const auto& c : cases) std::printf("args %s: %s\n", c.name, c.verdict ? c.verdict : "ok");
    return 0;
}
