// nav_field_main.cpp — the host half of the navigation fields (raytrace_amd/csrc/api/nav_check.hpp) as a program of its own, built
// with the address and undefined-behaviour sanitizers by tests/test_nav_field_host.py.
//
//     nav_field_main TABLE
//
// TABLE is a text file written by the test from tests/nav_field_sets.py, one row per line:
//     build MAX_DIST HEIGHT MAX_CLIMB MAX_DROP GOAL_SNAP R0 R1 R2 GOAL_COUNT GOALS_NULL
//     box LOX LOY LOZ EX EY EZ LOGR
//     plan EX EY EZ MAX_DIST LEVELS
//     sample COUNT AGENTS_NULL STEPS_NULL
// The program answers each row with one line: "build V" (1 = refused), "box V" (1 = inside), "plan ..." with the tiles, the pieces
// per row, the words of one bitmap and of the scratch, the bytes of the block and the level launches, "sample V"; then the store's
// behaviour (64 entries, the 65th, ids) on lines of their own.  The test holds them against tests/nav_field_ref.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "../raytrace_amd/csrc/api/nav_check.hpp"

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s TABLE\n", argv[0]); return 2; }
    FILE* fp = std::fopen(argv[1], "r");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char kind[16];
    while (std::fscanf(fp, "%15s", kind) == 1) {
        if (!std::strcmp(kind, "build")) {
            unsigned v[10];
            for (unsigned& x : v)
                if (std::fscanf(fp, "%u", &x) != 1) return 3;
            RtNavBuild p{};
            p.max_dist = v[0];
            p.height = (uint8_t)v[1]; p.max_climb = (uint8_t)v[2]; p.max_drop = (uint8_t)v[3]; p.goal_snap = (uint8_t)v[4];
            p.reserved[0] = v[5]; p.reserved[1] = v[6]; p.reserved[2] = v[7];
            const RtNavGoal goal{};
            std::printf("build %d\n", rta::nav_build_error(&p, v[9] ? nullptr : &goal, v[8]) ? 1 : 0);
        } else if (!std::strcmp(kind, "box")) {
            long long v[7];
            for (long long& x : v)
                if (std::fscanf(fp, "%lld", &x) != 1) return 3;
            const int32_t lo[3] = {(int32_t)v[0], (int32_t)v[1], (int32_t)v[2]}, ext[3] = {(int32_t)v[3], (int32_t)v[4], (int32_t)v[5]};
            std::printf("box %d\n", rta::nav_extent_valid(ext) && rta::nav_box_inside(lo, ext, (int)v[6]) ? 1 : 0);
        } else if (!std::strcmp(kind, "plan")) {
            unsigned v[5];
            for (unsigned& x : v)
                if (std::fscanf(fp, "%u", &x) != 1) return 3;
            const int32_t ext[3] = {(int32_t)v[0], (int32_t)v[1], (int32_t)v[2]};
            const rta::NavPlan p = rta::nav_plan(ext, v[3], v[4]);
            std::printf("plan %u %u %u %zu %zu %zu %u tiles %u\n", p.tiles_x, p.tiles_y, p.row_halves, p.bitmap_words, p.scratch_words, p.block_bytes,
                        p.launches, p.tiles);
        } else if (!std::strcmp(kind, "sample")) {
            unsigned v[3];
            for (unsigned& x : v)
                if (std::fscanf(fp, "%u", &x) != 1) return 3;
            const int here = 0;
            std::printf("sample %d\n", rta::nav_sample_error(v[1] ? nullptr : &here, v[0], v[2] ? nullptr : &here) ? 1 : 0);
        } else {
            return 3;
        }
    }
    std::fclose(fp);
    std::printf("null params %d\n", rta::nav_build_error(nullptr, nullptr, 0) ? 1 : 0);

    // the store: 64 live entries with ids of their own, none 0; the 65th is refused; a destroyed id stays unknown when its slot is reused
    rta::NavStore st;
    std::set<uint32_t> ids;
    const int32_t ext[3] = {3, 4, 5};
    for (uint32_t i = 0; i < rta::kMaxNavFields; i++) ids.insert(st.add(ext)->id);
    std::printf("store %zu zero %d full %d\n", ids.size(), (int)ids.count(0u), st.add(ext) == nullptr ? 1 : 0);
    const uint32_t old = *ids.begin();
    st.remove(st.find(old));
    const rta::NavEntry* again = st.add(ext);
    std::printf("reuse %d %d %d live %u cells %zu\n", again->id != old ? 1 : 0, st.find(old) == nullptr ? 1 : 0, st.find(again->id) == again ? 1 : 0, st.live,
                again->cells());
    return 0;
}
