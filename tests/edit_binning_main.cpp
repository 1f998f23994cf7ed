// Stand-alone check of raytrace_amd/csrc/api/edit_binning.hpp (the host half of rt_edit_voxels) against a brute-force model:
// for each touched chunk in ascending chunk id, the set of (local voxel -> last edit in batch order).  Built and run by
// tests/test_edit_binning.py, with the sanitizers where the compiler has them.  Exit status 0 = every case passed.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../raytrace_amd/csrc/api/edit_binning.hpp"

namespace {

int g_failures = 0;
#define CHECK(cond, ...)                                                            \
    do {                                                                            \
        if (!(cond)) {                                                              \
            if (g_failures++ < 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } \
        }                                                                           \
    } while (0)

struct Rng {   // xorshift64*
    uint64_t s;
    uint32_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32); }
    uint32_t below(uint32_t n) { return next() % n; }
};

RtVoxelEdit edit(uint32_t x, uint32_t y, uint32_t z, uint32_t solid, uint32_t material) {
    RtVoxelEdit e{};
    e.x = (uint16_t)x; e.y = (uint16_t)y; e.z = (uint16_t)z; e.solid = (uint16_t)solid; e.material = material;
    return e;
}

struct Kept { bool solid; uint32_t material; };
using Model = std::map<uint32_t, std::map<uint32_t, Kept>>;   // chunk id -> local voxel -> its last edit

// The model, from the ABI's words alone: chunks of 64^3 in x-fastest order, a voxel's last edit in batch order wins.
Model model_of(const std::vector<RtVoxelEdit>& edits, int logr) {
    const uint32_t per_axis = (1u << logr) / 64u;
    Model m;
    for (const RtVoxelEdit& e : edits) {
        const uint32_t chunk = ((e.z / 64u) * per_axis + e.y / 64u) * per_axis + e.x / 64u;
        const uint32_t local = ((e.z % 64u) * 64u + e.y % 64u) * 64u + e.x % 64u;
        m[chunk][local] = Kept{e.solid != 0, e.material};
    }
    return m;
}

size_t round16(size_t n) { return (n + 15u) / 16u * 16u; }

// Bins and stages a valid batch as rt_edit_voxels does and compares every word with the model.
void run_valid(rta::EditBinning& b, const std::vector<RtVoxelEdit>& edits, int logr, const char* what) {
    const uint32_t count = (uint32_t)edits.size();
    const Model m = model_of(edits, logr);
    rta::EditBins bins;
    const uint32_t r = rta::edit_bin(b, edits.data(), count, logr, &bins);
    CHECK(r == count, "%s logr %d: valid batch rejected at %u", what, logr, r);
    if (r != count) return;
    size_t distinct = 0;
    for (const auto& c : m) distinct += c.second.size();
    CHECK(bins.touched == m.size(), "%s logr %d: touched %u, model %zu", what, logr, bins.touched, m.size());
    CHECK(bins.off_offs == round16(4u * m.size()), "%s: off_offs %zu", what, bins.off_offs);
    CHECK(bins.off_recs == bins.off_offs + round16(4u * (m.size() + 1u)), "%s: off_recs %zu", what, bins.off_recs);
    CHECK(bins.need == bins.off_recs + 8u * (size_t)count, "%s: need %zu", what, bins.need);
    if (bins.touched != m.size()) return;
    // exactly `need` bytes, as three heap blocks of their own so that the sanitizer sees a write past any of them
    std::vector<uint32_t> chunks(bins.touched), offs((size_t)bins.touched + 1u), recs(2u * (size_t)count);
    const uint32_t nrec = rta::edit_fill(b, edits.data(), logr, chunks.data(), offs.data(), recs.data());
    CHECK(nrec == distinct, "%s logr %d: %u records, model %zu", what, logr, nrec, distinct);
    CHECK(offs[bins.touched] == nrec, "%s: last offset %u, records %u", what, offs[bins.touched], nrec);
    if (nrec != distinct) return;
    uint32_t t = 0;
    for (const auto& c : m) {   // ascending chunk id
        CHECK(chunks[t] == c.first, "%s logr %d: chunk[%u] = %u, model %u", what, logr, t, chunks[t], c.first);
        const uint32_t lo = offs[t], hi = offs[t + 1u];
        CHECK(lo <= hi && hi <= nrec && hi - lo == c.second.size(), "%s: chunk %u has records %u..%u, model %zu", what, c.first, lo, hi, c.second.size());
        if (!(lo <= hi && hi <= nrec)) return;
        std::map<uint32_t, Kept> got;
        for (uint32_t k = lo; k < hi; k++) {
            const uint32_t w = recs[2u * k], local = w & 0x3FFFFu;
            CHECK((w >> 19) == 0u, "%s: record word %08x has bits above the solid bit", what, w);
            CHECK(got.find(local) == got.end(), "%s: chunk %u voxel %u recorded twice", what, c.first, local);
            got[local] = Kept{((w >> 18) & 1u) != 0u, recs[2u * k + 1u]};
        }
        for (const auto& v : c.second) {
            const auto it = got.find(v.first);
            CHECK(it != got.end(), "%s: chunk %u voxel %u missing", what, c.first, v.first);
            if (it == got.end()) continue;
            CHECK(it->second.solid == v.second.solid && it->second.material == v.second.material,
                  "%s: chunk %u voxel %u holds (%d, %08x), its last edit is (%d, %08x)", what, c.first, v.first, (int)it->second.solid,
                  it->second.material, (int)v.second.solid, v.second.material);
        }
        t++;
    }
}

std::vector<RtVoxelEdit> random_batch(Rng& rng, uint32_t n, uint32_t R, double repeat) {
    std::vector<RtVoxelEdit> v;
    for (uint32_t i = 0; i < n; i++) {
        if (i > 0 && rng.below(1000) < (uint32_t)(repeat * 1000)) {   // an earlier voxel again, with another value
            RtVoxelEdit e = v[rng.below(i)];
            e.solid = (uint16_t)rng.below(3); e.material = rng.next();
            v.push_back(e);
        } else {
            v.push_back(edit(rng.below(R), rng.below(R), rng.below(R), rng.below(2), rng.next()));
        }
    }
    return v;
}

// A batch with one bad edit at `at`: the function reports that index and leaves `out` alone.
void run_bad(rta::EditBinning& b, std::vector<RtVoxelEdit> edits, size_t at, bool reserved, int axis, int logr) {
    const uint32_t R = 1u << logr;
    if (reserved) edits[at].reserved = 1u;
    else (axis == 0 ? edits[at].x : axis == 1 ? edits[at].y : edits[at].z) = (uint16_t)R;
    rta::EditBins bins;
    bins.touched = 0xABCDu; bins.off_offs = 1; bins.off_recs = 2; bins.need = 3;
    const uint32_t r = rta::edit_bin(b, edits.data(), (uint32_t)edits.size(), logr, &bins);
    CHECK(r == at, "bad edit at %zu (reserved %d, axis %d, logr %d) reported as %u", at, (int)reserved, axis, logr, r);
    CHECK(bins.touched == 0xABCDu && bins.off_offs == 1 && bins.off_recs == 2 && bins.need == 3, "a rejected batch wrote its result");
}

void run_all(int logr) {
    const uint32_t R = 1u << logr, per_axis = R / 64u;
    Rng rng{0x9E3779B97F4A7C15ull + (uint64_t)logr};
    rta::EditBinning b;   // one for the whole sequence, as the context keeps it

    run_valid(b, {edit(R - 1u, 0, R / 2u, 1, 0x11u)}, logr, "one edit");
    run_valid(b, {edit(70, 5, 3, 1, 0xAAu), edit(70, 5, 3, 0, 0xBBu)}, logr, "same voxel, solid then air");
    run_valid(b, {edit(70, 5, 3, 0, 0xAAu), edit(70, 5, 3, 2, 0xBBu)}, logr, "same voxel, air then solid");
    {   // 1000 edits in one chunk, drawn from 50 distinct voxels
        std::vector<RtVoxelEdit> pool, v;
        while (pool.size() < 50) {
            const RtVoxelEdit e = edit(R - 64u + rng.below(64), 64u + rng.below(64), rng.below(64), 0, 0);
            bool seen = false;
            for (const RtVoxelEdit& p : pool) seen = seen || (p.x == e.x && p.y == e.y && p.z == e.z);
            if (!seen) pool.push_back(e);
        }
        for (int i = 0; i < 1000; i++) { RtVoxelEdit e = pool[i < 50 ? (uint32_t)i : rng.below(50)]; e.solid = (uint16_t)rng.below(2); e.material = rng.next(); v.push_back(e); }
        run_valid(b, v, logr, "1000 edits of 50 voxels in one chunk");
    }
    {   // one edit in every chunk, in descending chunk order
        std::vector<RtVoxelEdit> v;
        for (uint32_t c = per_axis * per_axis * per_axis; c-- > 0;)
            v.push_back(edit((c % per_axis) * 64u + rng.below(64), (c / per_axis % per_axis) * 64u + rng.below(64), (c / per_axis / per_axis) * 64u + rng.below(64),
                             rng.below(2), rng.next()));
        run_valid(b, v, logr, "one edit in every chunk");
    }
    run_valid(b, random_batch(rng, 5000, R, 0.3), logr, "5000 random edits, 30 % repeats");

    // rejected batches: an out-of-range coordinate on each axis and reserved != 0, first, in the middle and last
    const std::vector<RtVoxelEdit> good = random_batch(rng, 101, R, 0.3);
    for (size_t at : {(size_t)0, good.size() / 2u, good.size() - 1u}) {
        for (int axis = 0; axis < 3; axis++) run_bad(b, good, at, false, axis, logr);
        run_bad(b, good, at, true, 0, logr);
    }
    run_valid(b, good, logr, "a valid batch after the rejected ones");

    // the stamp generation wraps: the voxels of `first` hold generation 1 from a fresh scratch; three batches from 0xFFFFFFFE on
    // cross the wrap, and the second runs under generation 1 again — it keeps its voxels only if the stamps were refilled
    rta::EditBinning w;
    const std::vector<RtVoxelEdit> first = {edit(1, 2, 3, 1, 7u), edit(4, 5, 6, 1, 8u), edit(1, 2, 3, 0, 9u)};
    run_valid(w, first, logr, "wrap: fresh scratch");
    CHECK(w.gen == 1u, "generation after the first chunk run is %u", w.gen);
    w.gen = 0xFFFFFFFEu;
    run_valid(w, {edit(9, 9, 9, 1, 1u), edit(9, 9, 9, 0, 2u)}, logr, "wrap: batch 1");
    CHECK(w.gen == 0xFFFFFFFFu, "generation before the wrap is %08x", w.gen);
    run_valid(w, first, logr, "wrap: batch 2");
    CHECK(w.gen == 1u, "generation after the wrap is %u", w.gen);
    run_valid(w, random_batch(rng, 300, R, 0.3), logr, "wrap: batch 3");
}

}  // namespace

int main() {
    run_all(8);
    run_all(9);
    if (g_failures) { fprintf(stderr, "%d checks failed\n", g_failures); return 1; }
    puts("edit binning: all cases match the model");
    return 0;
}
