// deposit_particles_main.cpp — the host half of rt_deposit_particles (raytrace_amd/csrc/api/deposit_check.hpp) as a program of its
// own, built with the address and undefined-behaviour sanitizers by tests/test_deposit_particles_host.py.
//
//     deposit_particles_main RECORDS LOGR [LIMIT ...]
//
// RECORDS is a file of RtParticleDeposit records (the table of tests/deposit_particles_sets.py, written by the test); a LIMIT is
// "logr,lox,loy,loz,hix,hiy,hiz".  The program prints one line "verdicts 1011..." with deposit_params_error's answer per record, one
// line "plan I: ..." per valid record with the clipped box, its texels, the chunks per axis, the staging bytes, the scratch words and
// the chunk ids, one line "limit ..." per LIMIT, the overlap test's answers and one line per case of deposit_args_error; the test
// holds them against tests/deposit_particles_ref.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytrace_amd/csrc/api/deposit_check.hpp"

static void print_plan(const rta::DepositPlan& d, int logr) {
    if (d.empty) { std::printf("empty\n"); return; }
    std::printf("box %u %u %u %u %u %u texels %llu chunks %u %u %u need %zu scratch %zu ids", d.box.lo[0], d.box.lo[1], d.box.lo[2], d.box.hi[0], d.box.hi[1],
                d.box.hi[2], (unsigned long long)d.texels, d.nc[0], d.nc[1], d.nc[2], d.need, rta::deposit_scratch_need(d));
    std::vector<uint32_t> ids(d.nchunks);
    const uint32_t n = rta::deposit_fill_chunks(d, logr, ids.data());
    for (uint32_t i = 0; i < n && i < 64u; i++) std::printf(" %u", ids[i]);
    std::printf(" (%u)\n", n);
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s RECORDS LOGR [LIMIT ...]\n", argv[0]); return 2; }
    const int logr = std::atoi(argv[2]);
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<RtParticleDeposit> recs;
    RtParticleDeposit one;
    while (std::fread(&one, sizeof one, 1, fp) == 1) recs.push_back(one);
    std::fclose(fp);
    static_assert(sizeof(RtParticleDeposit) == 48 && sizeof(RtDepositCount) == 16, "the records are 48 and 16 bytes");

    std::printf("records %zu\nverdicts ", recs.size());
    for (const RtParticleDeposit& p : recs) std::putchar(rta::deposit_params_error(p, logr) ? '0' : '1');
    std::printf("\n");
    for (size_t i = 0; i < recs.size(); i++) {
        if (rta::deposit_params_error(recs[i], logr)) continue;
        std::printf("plan %zu: ", i);
        print_plan(rta::deposit_plan(recs[i], logr), logr);
    }
    for (int b = 3; b < argc; b++) {
        int v[7] = {};
        if (std::sscanf(argv[b], "%d,%d,%d,%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]) != 7) return 2;
        RtParticleDeposit p{};
        for (int k = 0; k < 3; k++) { p.lo[k] = v[1 + k]; p.hi[k] = v[4 + k]; }
        const rta::DepositPlan d = rta::deposit_plan(p, v[0]);
        std::printf("limit %d: valid %d texels %llu allowed %d chunks %u\n", b - 3, rta::deposit_params_error(p, v[0]) ? 0 : 1, (unsigned long long)d.texels,
                    d.texels <= rta::kMaxDepositBoxTexels ? 1 : 0, d.nchunks);
    }

    // the overlap test and the plain arguments, on one block of memory: 4 states, 4 draw records, a count record
    alignas(16) static unsigned char block[4 * 64 + 4 * 32 + 16 + 64];
    unsigned char *states = block, *draw = block + 256, *counts = block + 384;
    const RtParticleDeposit p{};
    struct { const char* name; const char* verdict; } cases[] = {
        {"fine", rta::deposit_args_error(&p, states, draw, 4, counts)},
        {"no draw no counts", rta::deposit_args_error(&p, states, nullptr, 4, nullptr)},
        {"empty", rta::deposit_args_error(&p, nullptr, nullptr, 0, nullptr)},
        {"at the limit", rta::deposit_args_error(&p, states, nullptr, 1u << 20, nullptr)},
        {"null params", rta::deposit_args_error(nullptr, states, draw, 4, counts)},
        {"null params empty", rta::deposit_args_error(nullptr, nullptr, nullptr, 0, nullptr)},
        {"null states", rta::deposit_args_error(&p, nullptr, draw, 4, counts)},
        {"count beyond", rta::deposit_args_error(&p, states, nullptr, (1u << 20) + 1u, nullptr)},
        {"draw in states", rta::deposit_args_error(&p, states, states + 64, 4, counts)},
        {"draw touches the last state", rta::deposit_args_error(&p, states, states + 255, 4, nullptr)},
        {"draw behind states", rta::deposit_args_error(&p, states, states + 256, 4, nullptr)},
        {"states in draw", rta::deposit_args_error(&p, draw + 32, draw, 4, nullptr)},
        {"counts in states", rta::deposit_args_error(&p, states, draw, 4, states + 28)},
        {"counts in draw", rta::deposit_args_error(&p, states, draw, 4, draw + 127)},
        {"counts ends at states", rta::deposit_args_error(&p, states + 16, nullptr, 3, states)},
        {"counts over the start of states", rta::deposit_args_error(&p, states + 15, nullptr, 3, states)},
    };
    for (const auto& c : cases) std::printf("args %s: %s\n", c.name, c.verdict ? c.verdict : "ok");

    const int32_t edge = (1 << 22) - (1 << logr);
    const int32_t windows[][3] = {{0, 0, 0}, {edge, -edge, 0}, {edge + 1, 0, 0}, {0, 0, -edge - 1}, {0, INT32_MIN, 0}};
    std::printf("windows ");
    for (const auto& w : windows) {
        RtParticleDeposit q{};
        for (int k = 0; k < 3; k++) q.lr[k] = w[k];
        std::putchar(rta::deposit_params_error(q, logr) ? '0' : '1');
    }
    std::printf("\n");
    return 0;
}
