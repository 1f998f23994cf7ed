// sweep_entities_main.cpp — the host half of rt_sweep_entities (raytrace_amd/csrc/api/sweep_entities_check.hpp) as a program of its
// own, built with the address and undefined-behaviour sanitizers by tests/test_sweep_entities_host.py.
//
//     sweep_entities_main SWEEPS BOXES
//
// SWEEPS is a file of RtBoxSweep records and BOXES one of RtDrawBox records, written by the test.  The program prints one line
// "sweeps 10..." with whether each sweep lies in the validated domain, "first_invalid_sweep K", "boxes 10...", "first_invalid_box K",
// "prefixes 1" when every batch that ends before the first invalid record is accepted, one line "models 10..." for a table of
// RtDrawStamp records judged against a 3 x 11 x 4 stamp, and one line per case of sweep_entities_args_error; the test holds them
// against tests/sweep_entities_ref.py and tests/sweep_ref.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytrace_amd/csrc/api/sweep_entities_check.hpp"

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
    if (argc != 3) { std::fprintf(stderr, "usage: %s SWEEPS BOXES\n", argv[0]); return 2; }
    std::vector<RtBoxSweep> sweeps;
    std::vector<RtDrawBox> boxes;
    if (!read_all(argv[1], sweeps) || !read_all(argv[2], boxes)) return 2;

    std::printf("sweeps ");
    for (const RtBoxSweep& s : sweeps) std::putchar(rta::sweep_in_domain(s) ? '1' : '0');
    const uint32_t bad_sweep = rta::first_invalid_sweep(sweeps.data(), (uint32_t)sweeps.size());
    std::printf("\nfirst_invalid_sweep %u\nboxes ", bad_sweep);
    for (const RtDrawBox& b : boxes) std::putchar(rta::draw_box_valid(b) ? '1' : '0');
    const uint32_t bad_box = rta::first_invalid_draw_box(boxes.data(), (uint32_t)boxes.size());
    std::printf("\nfirst_invalid_box %u\n", bad_box);

    // every batch that ends before the first invalid record is valid; an empty batch reads nothing
    bool prefixes = rta::first_invalid_sweep(nullptr, 0) == 0u && rta::first_invalid_draw_box(nullptr, 0) == 0u;
    for (uint32_t n = 0; n <= bad_sweep; n++) prefixes = prefixes && rta::first_invalid_sweep(sweeps.data(), n) == n;
    for (uint32_t n = 0; n <= bad_box; n++) prefixes = prefixes && rta::first_invalid_draw_box(boxes.data(), n) == n;
    std::printf("prefixes %d\n", prefixes ? 1 : 0);

    // the models' record rule, which the calls reuse from the draw: a 3 x 11 x 4 stamp
    const int32_t E[3] = {3, 11, 4};
    RtDrawStamp fine{};
    fine.origin[0] = 1.5f; fine.origin[1] = -2.0f; fine.origin[2] = 0.25f;
    fine.scale = 0.5f; fine.stamp = 1u; fine.orient = 13;
    std::vector<RtDrawStamp> models(8, fine);
    models[1].orient = 48;
    models[2].scale = 1.0f / 512.0f;
    models[3].scale = 65.0f;
    models[4].reserved = 1u;
    models[5].reserved0[1] = 1u;
    models[6].origin[2] = 4194304.0f;             // the high plane passes 2^22
    models[7].origin[0] = -4194304.0f; models[7].scale = 64.0f;
    std::printf("models ");
    for (const RtDrawStamp& m : models) std::putchar(rta::draw_stamp_valid(m, E) ? '1' : '0');
    std::putchar('\n');

    alignas(16) static unsigned char block[1024];
    const int32_t lr[3] = {0, 0, 0};
    unsigned char* a = block;
    struct { const char* name; const char* verdict; } cases[] = {
        {"fine", rta::sweep_entities_args_error(8, a, lr, a + 512, a + 128, 2, a + 256, 2)},
        {"no entities", rta::sweep_entities_args_error(8, a, lr, a + 512, nullptr, 0, nullptr, 0)},
        {"empty", rta::sweep_entities_args_error(0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0)},
        {"empty with entities", rta::sweep_entities_args_error(0, nullptr, nullptr, nullptr, a, 1, a, 1)},
        {"counts at the limits", rta::sweep_entities_args_error(1u << 24, a, lr, a, a, 4096, a, 4096)},
        {"sweeps beyond", rta::sweep_entities_args_error((1u << 24) + 1u, a, lr, a, nullptr, 0, nullptr, 0)},
        {"boxes beyond", rta::sweep_entities_args_error(8, a, lr, a, a, 4097, nullptr, 0)},
        {"models beyond", rta::sweep_entities_args_error(8, a, lr, a, nullptr, 0, a, 4097)},
        {"null sweeps", rta::sweep_entities_args_error(8, nullptr, lr, a, nullptr, 0, nullptr, 0)},
        {"null lr", rta::sweep_entities_args_error(8, a, nullptr, a, nullptr, 0, nullptr, 0)},
        {"null hits", rta::sweep_entities_args_error(8, a, lr, nullptr, nullptr, 0, nullptr, 0)},
        {"null boxes", rta::sweep_entities_args_error(8, a, lr, a, nullptr, 1, nullptr, 0)},
        {"null models", rta::sweep_entities_args_error(8, a, lr, a, nullptr, 0, nullptr, 1)},
    };
    for (const auto& c : cases) std::printf("args %s: %s\n", c.name, c.verdict ? c.verdict : "ok");
    return 0;
}
