// flow_voxels_main.cpp — the host half of rt_flow_voxels (raytrace_amd/csrc/api/flow_check.hpp) as a program of its own, built with
// the address and undefined-behaviour sanitizers by tests/test_flow_voxels_host.py.
//
//     flow_voxels_main RECORDS LOGR [EXTENTS]
//
// RECORDS is a file of RtVoxelFlow records (the table of tests/flow_voxels_sets.py, written by the test).  The program prints one line
// "verdicts 1011..." with flow_params_error's answer per record, one line "plan I: ..." per valid record with the clipped box, its
// extent, the chunks per axis, the staging bytes, the tiles, the cells of a state array, the launches for 1, 2, 4 and 8 ticks per
// launch, the scratch words and the chunk ids, one line per case of flow_args_error, one line "extent ..." per row of EXTENTS (lines
// "lo hi logr") and the plan of the largest box; the test holds them against tests/flow_voxels_ref.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytrace_amd/csrc/api/flow_check.hpp"

static void print_plan(const RtVoxelFlow& p, const rta::FlowPlan& s, int logr) {
    if (s.empty) { std::printf("empty\n"); return; }
    std::printf("box %u %u %u %u %u %u ext %d %d %d chunks %u %u %u need %zu tiles %u %u %u = %u cells %llu launches %u %u %u %u scratch %zu ids", s.box.lo[0],
                s.box.lo[1], s.box.lo[2], s.box.hi[0], s.box.hi[1], s.box.hi[2], s.ext[0], s.ext[1], s.ext[2], s.nc[0], s.nc[1], s.nc[2], s.need, s.tiles[0],
                s.tiles[1], s.tiles[2], s.ntiles, (unsigned long long)s.cells, rta::flow_launches(p.ticks, 1), rta::flow_launches(p.ticks, 2),
                rta::flow_launches(p.ticks, 4), rta::flow_launches(p.ticks, 8), rta::flow_scratch_need(s));
    std::vector<uint32_t> ids(s.nchunks);
    const uint32_t n = rta::deposit_fill_chunks(s, logr, ids.data());
    for (uint32_t i = 0; i < n && i < 64u; i++) std::printf(" %u", ids[i]);
    std::printf(" (%u)\n", n);
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s RECORDS LOGR [EXTENTS]\n", argv[0]); return 2; }
    const int logr = std::atoi(argv[2]);
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<RtVoxelFlow> recs;
    RtVoxelFlow one;
    while (std::fread(&one, sizeof one, 1, fp) == 1) recs.push_back(one);
    std::fclose(fp);
    static_assert(sizeof(RtVoxelFlow) == 64 && sizeof(RtFlowCount) == 32, "the records are 64 and 32 bytes");

    std::printf("records %zu\nverdicts ", recs.size());
    for (const RtVoxelFlow& p : recs) std::putchar(rta::flow_params_error(p, logr) ? '0' : '1');
    std::printf("\n");
    for (size_t i = 0; i < recs.size(); i++) {
        if (rta::flow_params_error(recs[i], logr)) continue;
        std::printf("plan %zu: ", i);
        print_plan(recs[i], rta::flow_plan(recs[i], logr), logr);
    }
    const RtVoxelFlow p{};
    std::printf("args params: %s\n", rta::flow_args_error(&p) ? rta::flow_args_error(&p) : "ok");
    std::printf("args null params: %s\n", rta::flow_args_error(nullptr) ? rta::flow_args_error(nullptr) : "ok");
    if (argc > 3) {
        FILE* fe = std::fopen(argv[3], "r");
        if (!fe) { std::fprintf(stderr, "cannot open %s\n", argv[3]); return 2; }
        RtVoxelFlow q = recs.empty() ? RtVoxelFlow{} : recs[0];   // the first record is the plain, valid one
        int lr = 0;
        while (std::fscanf(fe, "%d %d %d %d %d %d %d", &q.lo[0], &q.lo[1], &q.lo[2], &q.hi[0], &q.hi[1], &q.hi[2], &lr) == 7)
            std::printf("extent %d\n", rta::flow_params_error(q, lr) ? 0 : 1);
        std::fclose(fe);
    }
    // the largest box: 256^3 cells of a region of 512, off the chunk grid — 125 chunks, 2048 tiles, 256 launches at one tick each
    RtVoxelFlow all = recs.empty() ? RtVoxelFlow{} : recs[0];
    for (int k = 0; k < 3; k++) { all.lo[k] = 10; all.hi[k] = 265; }
    all.ticks = rta::kFlowMaxTicks;
    const rta::FlowPlan big = rta::flow_plan(all, 9);
    std::printf("largest: valid %d chunks %u tiles %u cells %llu launches %u %u scratch %zu\n", rta::flow_params_error(all, 9) ? 0 : 1, big.nchunks, big.ntiles,
                (unsigned long long)big.cells, rta::flow_launches(all.ticks, 1), rta::flow_launches(all.ticks, rta::kFlowGroup), rta::flow_scratch_need(big));
    return 0;
}
