// settle_voxels_main.cpp — the host half of rt_settle_voxels (raytrace_amd/csrc/api/settle_check.hpp) as a program of its own, built
// with the address and undefined-behaviour sanitizers by tests/test_settle_voxels_host.py.
//
//     settle_voxels_main RECORDS LOGR
//
// RECORDS is a file of RtVoxelSettle records (the table of tests/settle_voxels_sets.py, written by the test).  The program prints one
// line "verdicts 1011..." with settle_params_error's answer per record, one line "plan I: ..." per valid record with the clipped
// box, its columns and their height, the chunks per axis, the staging bytes, the scratch words and the chunk ids, and one line per
// case of settle_args_error; the test holds them against tests/settle_voxels_ref.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytrace_amd/csrc/api/settle_check.hpp"

static void print_plan(const rta::SettlePlan& s, int logr) {
    if (s.empty) { std::printf("empty\n"); return; }
    std::printf("box %u %u %u %u %u %u columns %llu height %u chunks %u %u %u need %zu scratch %zu ids", s.box.lo[0], s.box.lo[1], s.box.lo[2], s.box.hi[0],
                s.box.hi[1], s.box.hi[2], (unsigned long long)s.columns, s.height, s.nc[0], s.nc[1], s.nc[2], s.need, rta::settle_scratch_need(s));
    std::vector<uint32_t> ids(s.nchunks);
    const uint32_t n = rta::deposit_fill_chunks(s, logr, ids.data());
    for (uint32_t i = 0; i < n && i < 64u; i++) std::printf(" %u", ids[i]);
    std::printf(" (%u)\n", n);
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s RECORDS LOGR\n", argv[0]); return 2; }
    const int logr = std::atoi(argv[2]);
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<RtVoxelSettle> recs;
    RtVoxelSettle one;
    while (std::fread(&one, sizeof one, 1, fp) == 1) recs.push_back(one);
    std::fclose(fp);
    static_assert(sizeof(RtVoxelSettle) == 48 && sizeof(RtSettleCount) == 16, "the records are 48 and 16 bytes");

    std::printf("records %zu\nverdicts ", recs.size());
    for (const RtVoxelSettle& p : recs) std::putchar(rta::settle_params_error(p, logr) ? '0' : '1');
    std::printf("\n");
    for (size_t i = 0; i < recs.size(); i++) {
        if (rta::settle_params_error(recs[i], logr)) continue;
        std::printf("plan %zu: ", i);
        print_plan(rta::settle_plan(recs[i], logr), logr);
    }
    const RtVoxelSettle p{};
    std::printf("args params: %s\n", rta::settle_args_error(&p) ? rta::settle_args_error(&p) : "ok");
    std::printf("args null params: %s\n", rta::settle_args_error(nullptr) ? rta::settle_args_error(nullptr) : "ok");
    // the whole region at the largest size: no texel limit, 4096 chunks
    RtVoxelSettle all{};
    for (int k = 0; k < 3; k++) { all.lo[k] = -4096; all.hi[k] = 4096; }
    all.max_fall = rta::kSettleUnlimited;
    const rta::SettlePlan big = rta::settle_plan(all, 10);
    std::printf("whole 1024: valid %d columns %llu height %u chunks %u scratch %zu\n", rta::settle_params_error(all, 10) ? 0 : 1, (unsigned long long)big.columns,
                big.height, big.nchunks, rta::settle_scratch_need(big));
    return 0;
}
