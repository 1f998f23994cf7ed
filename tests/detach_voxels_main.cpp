// detach_voxels_main.cpp — the host half of rt_detach_voxels (raytrace_amd/csrc/api/detach_check.hpp) as a program of its own, built
// with the address and undefined-behaviour sanitizers by tests/test_detach_voxels_host.py.
//
//     detach_voxels_main RECORDS LOGR
//
// RECORDS is a file of RtVoxelDetach records (the table of tests/detach_voxels_sets.py, written by the test).  The program prints one
// line "verdicts 1011..." with the answer of detach_args_error (a stamp_out given) and detach_params_error per record, one line
// "plan I: ..." per valid record with the clipped box, the stamp's extent, the chunks per axis, the staging bytes, the scratch words
// and the chunk ids, and one line per case of detach_args_error; the test holds them against tests/detach_voxels_ref.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytrace_amd/csrc/api/detach_check.hpp"

static void print_plan(const rta::DetachPlan& s, int logr) {
    if (s.empty) { std::printf("empty\n"); return; }
    std::printf("box %u %u %u %u %u %u extent %d %d %d chunks %u %u %u need %zu scratch %zu ids", s.box.lo[0], s.box.lo[1], s.box.lo[2], s.box.hi[0],
                s.box.hi[1], s.box.hi[2], s.ext[0], s.ext[1], s.ext[2], s.nc[0], s.nc[1], s.nc[2], s.need, rta::detach_scratch_need(s));
    std::vector<uint32_t> ids(s.nchunks);
    const uint32_t n = rta::deposit_fill_chunks(s, logr, ids.data());
    for (uint32_t i = 0; i < n && i < 128u; i++) std::printf(" %u", ids[i]);
    std::printf(" (%u)\n", n);
}

static const char* verdict(const RtVoxelDetach& p, const uint32_t* stamp_out, int logr) {
    const char* e = rta::detach_args_error(&p, stamp_out);
    return e ? e : rta::detach_params_error(p, logr);
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s RECORDS LOGR\n", argv[0]); return 2; }
    const int logr = std::atoi(argv[2]);
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<RtVoxelDetach> recs;
    RtVoxelDetach one;
    while (std::fread(&one, sizeof one, 1, fp) == 1) recs.push_back(one);
    std::fclose(fp);
    static_assert(sizeof(RtVoxelDetach) == 48 && sizeof(RtDetachResult) == 48, "the records are 48 bytes each");

    uint32_t stamp = 0;
    std::printf("records %zu\nverdicts ", recs.size());
    for (const RtVoxelDetach& p : recs) std::putchar(verdict(p, &stamp, logr) ? '0' : '1');
    std::printf("\n");
    for (size_t i = 0; i < recs.size(); i++) {
        if (verdict(recs[i], &stamp, logr)) continue;
        std::printf("plan %zu: ", i);
        print_plan(rta::detach_plan(recs[i], logr), logr);
    }
    RtVoxelDetach p{};
    p.max_passes = 1;
    std::printf("args query: %s\n", rta::detach_args_error(&p, nullptr) ? rta::detach_args_error(&p, nullptr) : "ok");
    std::printf("args null params: %s\n", rta::detach_args_error(nullptr, &stamp) ? rta::detach_args_error(nullptr, &stamp) : "ok");
    p.flags = RT_DETACH_CAPTURE;
    std::printf("args capture: %s\n", rta::detach_args_error(&p, &stamp) ? rta::detach_args_error(&p, &stamp) : "ok");
    std::printf("args capture without stamp_out: %s\n", rta::detach_args_error(&p, nullptr) ? rta::detach_args_error(&p, nullptr) : "ok");
    p.flags = 8u;
    std::printf("args unknown flag: %s\n", rta::detach_args_error(&p, &stamp) ? rta::detach_args_error(&p, &stamp) : "ok");
    // the largest box: 256^3 texels that lie across the chunk grid, 5 x 5 x 5 chunks, at the largest region size
    RtVoxelDetach all{};
    for (int k = 0; k < 3; k++) { all.lo[k] = 33; all.hi[k] = 288; }
    all.max_passes = rta::kDetachMaxPasses;
    const rta::DetachPlan big = rta::detach_plan(all, 10);
    std::printf("largest: valid %d extent %d chunks %u scratch %zu\n", rta::detach_params_error(all, 10) ? 0 : 1, big.ext[0], big.nchunks,
                rta::detach_scratch_need(big));
    all.hi[1] = 289;
    std::printf("one more: valid %d\n", rta::detach_params_error(all, 10) ? 0 : 1);
    return 0;
}
