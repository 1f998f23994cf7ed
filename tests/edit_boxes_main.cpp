// Stand-alone check of rta::edit_chunk_boxes (raytrace_amd/csrc/api/edit_binning.hpp: the boxes rt_edit_voxels records on a
// context with RtConfig.edit_radius > 0) against a brute-force model: per touched chunk in ascending chunk id, the texel min / max
// over every record of the chunk.  Built and run by tests/test_edit_boxes.py, with the sanitizers where the compiler has them.
#include <cstdio>
#include <map>
#include <vector>

#include "../raytrace_amd/csrc/api/edit_binning.hpp"

namespace {

int g_failures = 0;

struct Rng {   // xorshift64*
    uint64_t s;
    uint32_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32); }
    uint32_t below(uint32_t n) { return next() % n; }
};

RtVoxelEdit edit(uint32_t x, uint32_t y, uint32_t z, uint32_t solid) {
    RtVoxelEdit e{};
    e.x = (uint16_t)x; e.y = (uint16_t)y; e.z = (uint16_t)z; e.solid = (uint16_t)solid; e.material = 0x55u;
    return e;
}

void run(rta::EditBinning& b, const std::vector<RtVoxelEdit>& edits, int logr, const char* what) {
    const uint32_t per_axis = (1u << logr) / 64u;
    std::map<uint32_t, rta::EditBox> model;
    for (const RtVoxelEdit& e : edits) {
        const uint32_t chunk = ((e.z / 64u) * per_axis + e.y / 64u) * per_axis + e.x / 64u;
        const uint16_t p[3] = {e.x, e.y, e.z};
        auto it = model.find(chunk);
        if (it == model.end()) it = model.insert({chunk, rta::EditBox{{p[0], p[1], p[2]}, {p[0], p[1], p[2]}}}).first;
        for (int k = 0; k < 3; k++) {
            if (p[k] < it->second.lo[k]) it->second.lo[k] = p[k];
            if (p[k] > it->second.hi[k]) it->second.hi[k] = p[k];
        }
    }
    rta::EditBins bins;
    const uint32_t r = rta::edit_bin(b, edits.data(), (uint32_t)edits.size(), logr, &bins);
    if (r != edits.size() || bins.touched != model.size()) { fprintf(stderr, "FAIL %s: binned %u touched %u, model %zu\n", what, r, bins.touched, model.size()); g_failures++; return; }
    std::vector<rta::EditBox> got(bins.touched);   // exactly `touched` boxes: the sanitizer sees a write past them
    const uint32_t n = rta::edit_chunk_boxes(b, edits.data(), logr, got.data());
    if (n != bins.touched) { fprintf(stderr, "FAIL %s: %u boxes for %u chunks\n", what, n, bins.touched); g_failures++; return; }
    uint32_t t = 0;
    for (const auto& m : model) {
        for (int k = 0; k < 3; k++)
            if (got[t].lo[k] != m.second.lo[k] || got[t].hi[k] != m.second.hi[k]) {
                fprintf(stderr, "FAIL %s logr %d: chunk %u axis %d is %u..%u, model %u..%u\n", what, logr, m.first, k, got[t].lo[k], got[t].hi[k], m.second.lo[k], m.second.hi[k]);
                g_failures++;
            }
        t++;
    }
}

void run_all(int logr) {
    const uint32_t R = 1u << logr;
    Rng rng{0xD1B54A32D192ED03ull + (uint64_t)logr};
    rta::EditBinning b;
    run(b, {edit(R - 1u, 0, R / 2u, 1)}, logr, "one edit");
    run(b, {edit(70, 5, 3, 1), edit(70, 5, 3, 0), edit(64, 63, 0, 0)}, logr, "a voxel twice and an edit that changes nothing");
    run(b, {edit(126, 10, 10, 1), edit(129, 12, 11, 1), edit(127, 9, 13, 1), edit(128, 9, 13, 1)}, logr, "a block across a chunk face");
    {
        std::vector<RtVoxelEdit> v;
        for (uint32_t i = 0; i < 5000; i++) v.push_back(edit(rng.below(R), rng.below(R), rng.below(R), rng.below(2)));
        run(b, v, logr, "5000 random edits");
        for (uint32_t i = 0; i < 300; i++) v[i] = edit(200u + rng.below(30), 100u + rng.below(40), 17u + rng.below(90), 1);
        v.resize(300);
        run(b, v, logr, "300 edits in a few chunks");
    }
}

}  // namespace

int main() {
    run_all(8);
    run_all(9);
    run_all(10);
    if (g_failures) { fprintf(stderr, "%d checks failed\n", g_failures); return 1; }
    puts("edit boxes: all cases match the model");
    return 0;
}
