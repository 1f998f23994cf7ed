// Stand-alone check of raytrace_amd/csrc/api/edit_stamps.hpp (the host half of the voxel stamps) against a brute-force model written
// from the ABI's words alone: a placement's verdict, its placed extent and clipped bounding box in 64-bit arithmetic, the set of
// 64^3 chunks the boxes meet, the boxes that wait for the next frame, the device records, the store of ids, and the index mapping of
// every orientation over odd extents, voxel by voxel.  Built and run by tests/test_edit_stamps_host.py, with the sanitizers where the
// compiler has them.  Exit status 0 = every case passed.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../raytrace_amd/csrc/api/edit_stamps.hpp"

namespace {

int g_failures = 0;
long g_places = 0, g_boxed = 0, g_rejected = 0, g_voxels = 0;
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
    int32_t between(int32_t lo, int32_t hi) { return lo + (int32_t)below((uint32_t)(hi - lo + 1)); }
};

RtStampPlace place(uint32_t id, int32_t x, int32_t y, int32_t z, uint8_t orient = 0, uint8_t where = RT_WHERE_ALL) {
    RtStampPlace p{};
    p.at[0] = x; p.at[1] = y; p.at[2] = z; p.stamp = id; p.orient = orient; p.where = where;
    return p;
}

// ---- the model: the header's words ------------------------------------------------------------------------------------------
const int kPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

bool model_valid(const RtStampPlace& p, int64_t R, const std::set<uint32_t>& ids) {
    if (!ids.count(p.stamp) || p.orient >= 48 || p.where > 2 || p.reserved0[0] || p.reserved0[1] || p.reserved[0] || p.reserved[1] || p.reserved[2])
        return false;
    for (int k = 0; k < 3; k++)
        if ((int64_t)p.at[k] < -4 * R || (int64_t)p.at[k] > 4 * R) return false;
    return true;
}
struct Box { int64_t lo[3], hi[3]; };
bool model_box(const RtStampPlace& p, const int32_t E[3], int64_t R, Box* out) {
    for (int k = 0; k < 3; k++) {
        const int64_t ext = E[kPerm[p.orient >> 3][k]];
        int64_t lo = -1, hi = -1;
        for (int64_t x = 0; x < R; x++)
            if (x >= (int64_t)p.at[k] && x < (int64_t)p.at[k] + ext) { if (lo < 0) lo = x; hi = x; }
        if (lo < 0) return false;
        out->lo[k] = lo; out->hi[k] = hi;
    }
    return true;
}
// the stamp voxel (x, y, z) that placed-local cell d shows
void model_source(const int32_t E[3], uint32_t orient, const int64_t d[3], int64_t s[3]) {
    const int* perm = kPerm[orient >> 3];
    const uint32_t f = orient & 7u;
    for (int k = 0; k < 3; k++) s[perm[k]] = ((f >> perm[k]) & 1u) ? (int64_t)E[perm[k]] - 1 - d[k] : d[k];
}

// ---- the mapping: every orientation of a few odd extents, every voxel ------------------------------------------------------------
void run_mapping(const int32_t E[3]) {
    for (uint32_t orient = 0; orient < 48; orient++) {
        const rta::StampMap m = rta::stamp_map(E, orient);
        std::vector<uint8_t> seen((size_t)E[0] * E[1] * E[2], 0);
        for (int k = 0; k < 3; k++) CHECK(m.ext[k] == E[kPerm[orient >> 3][k]], "orient %u: E'[%d] = %d", orient, k, m.ext[k]);
        for (int64_t dz = 0; dz < m.ext[2]; dz++)
            for (int64_t dy = 0; dy < m.ext[1]; dy++)
                for (int64_t dx = 0; dx < m.ext[0]; dx++) {
                    const int64_t d[3] = {dx, dy, dz};
                    int64_t s[3];
                    model_source(E, orient, d, s);
                    const int64_t want = s[0] + (int64_t)E[0] * (s[1] + (int64_t)E[1] * s[2]);
                    const int32_t got = rta::stamp_source_index(m, (int32_t)dx, (int32_t)dy, (int32_t)dz);
                    CHECK(got == want, "orient %u cell (%lld, %lld, %lld): index %d, the model says %lld", orient, (long long)dx, (long long)dy, (long long)dz, got, (long long)want);
                    if (got >= 0 && (size_t)got < seen.size()) seen[(size_t)got]++;
                    g_voxels++;
                }
        for (uint8_t v : seen) CHECK(v == 1, "orient %u is no bijection", orient);
    }
}

// ---- a valid batch: plan, chunk list, pending boxes and device records against the model --------------------------------------------
void run_valid(rta::ShapeScratch& sc, const rta::StampStore& store, const std::vector<RtStampPlace>& places, int logr, const char* what) {
    const int64_t R = (int64_t)1 << logr, n = R / 64;
    const uint32_t count = (uint32_t)places.size();
    std::set<uint32_t> ids, want;
    for (const rta::StampEntry& e : store.slots) if (e.id) ids.insert(e.id);
    std::vector<Box> boxes;
    std::vector<int> has(count, 0);
    for (uint32_t i = 0; i < count; i++) {
        const RtStampPlace& p = places[i];
        CHECK(model_valid(p, R, ids), "%s: the case holds a placement the model rejects", what);
        Box b;
        g_places++;
        if (!model_box(p, store.find(p.stamp)->ext, R, &b)) continue;
        g_boxed++;
        has[i] = 1;
        boxes.push_back(b);
        for (int64_t cz = b.lo[2] / 64; cz <= b.hi[2] / 64; cz++)
            for (int64_t cy = b.lo[1] / 64; cy <= b.hi[1] / 64; cy++)
                for (int64_t cx = b.lo[0] / 64; cx <= b.hi[0] / 64; cx++) want.insert((uint32_t)((cz * n + cy) * n + cx));
    }
    CHECK(rta::places_validate(store, places.data(), count, logr) == count, "%s: a valid batch is rejected", what);
    const rta::StampPlan plan = rta::stamps_touched(sc, store, places.data(), count, logr);
    CHECK(plan.touched == want.size(), "%s: %u chunks touched, the model says %zu", what, plan.touched, want.size());
    CHECK(plan.boxes == boxes.size(), "%s: %u boxes, the model says %zu", what, plan.boxes, boxes.size());
    CHECK(plan.off_recs % 16 == 0 && plan.off_recs >= (size_t)plan.touched * 4 && plan.need == plan.off_recs + (size_t)count * 64, "%s: layout", what);
    std::vector<uint32_t> chunks(plan.touched + 1u, 0xDEADu);
    CHECK(rta::shapes_fill_chunks(sc, chunks.data()) == plan.touched && chunks[plan.touched] == 0xDEADu, "%s: chunk list length", what);
    CHECK(std::set<uint32_t>(chunks.begin(), chunks.begin() + plan.touched) == want, "%s: chunk list", what);
    std::vector<rta::EditBox> got(boxes.size() + 1u);
    CHECK(rta::stamp_pending_boxes(store, places.data(), count, logr, got.data()) == boxes.size(), "%s: pending boxes", what);
    for (size_t i = 0; i < boxes.size(); i++)
        for (int k = 0; k < 3; k++)
            CHECK(got[i].lo[k] == boxes[i].lo[k] && got[i].hi[k] == boxes[i].hi[k], "%s: box %zu axis %d: %u..%u, the model says %lld..%lld", what, i, k,
                  got[i].lo[k], got[i].hi[k], (long long)boxes[i].lo[k], (long long)boxes[i].hi[k]);
    // the device records: the box, and the folded mapping at the box's corners and a few cells between
    std::vector<rta::StampRecord> recs(count);
    rta::stamp_fill_records(store, places.data(), count, logr, recs.data());
    size_t bi = 0;
    for (uint32_t i = 0; i < count; i++) {
        const rta::StampRecord& r = recs[i];
        const rta::StampEntry* e = store.find(places[i].stamp);
        CHECK(r.mats == e->mats && r.state == e->state && r.where == places[i].where && r.reserved == 0u, "%s: record %u fields", what, i);
        if (!has[i]) {
            // no chunk's rejection test lets it through: lo > every texel, hi < every texel
            for (int k = 0; k < 3; k++) CHECK(r.lo[k] >= R && r.hi[k] < 0, "%s: record %u of a placement without a box", what, i);
            continue;
        }
        const Box& b = boxes[bi++];
        for (int k = 0; k < 3; k++) CHECK(r.lo[k] == b.lo[k] && r.hi[k] == b.hi[k], "%s: record %u box axis %d", what, i, k);
        for (int corner = 0; corner < 27; corner++) {
            int64_t w[3], d[3], s[3];
            for (int k = 0; k < 3; k++) {
                const int sel = (corner / (k == 0 ? 1 : k == 1 ? 3 : 9)) % 3;
                w[k] = sel == 0 ? b.lo[k] : sel == 1 ? b.hi[k] : (b.lo[k] + b.hi[k]) / 2;
                d[k] = w[k] - (int64_t)places[i].at[k];
            }
            model_source(e->ext, places[i].orient, d, s);
            const int64_t want_idx = s[0] + (int64_t)e->ext[0] * (s[1] + (int64_t)e->ext[1] * s[2]);
            const int64_t got_idx = (int64_t)r.base + (int64_t)r.stride[0] * w[0] + (int64_t)r.stride[1] * w[1] + (int64_t)r.stride[2] * w[2];
            CHECK(got_idx == want_idx && got_idx >= 0 && got_idx < (int64_t)e->voxels(), "%s: record %u maps a texel to %lld, the model says %lld", what, i,
                  (long long)got_idx, (long long)want_idx);
            // the same in the kernel's own 32-bit arithmetic
            const int32_t k32 = r.base + r.stride[1] * (int32_t)w[1] + r.stride[0] * (int32_t)w[0] + r.stride[2] * (int32_t)w[2];
            CHECK((int64_t)k32 == want_idx, "%s: record %u in 32 bits", what, i);
        }
    }
}

void run_invalid(const rta::StampStore& store, RtStampPlace bad, int logr, const char* what) {
    const int64_t R = (int64_t)1 << logr;
    std::set<uint32_t> ids;
    for (const rta::StampEntry& e : store.slots) if (e.id) ids.insert(e.id);
    CHECK(!model_valid(bad, R, ids), "%s: the model accepts it", what);
    const RtStampPlace good = place(*ids.begin(), 1, 2, 3);
    const RtStampPlace a[3] = {good, good, bad}, b[3] = {bad, good, good};
    CHECK(rta::places_validate(store, a, 3, logr) == 2, "%s: last of three", what);
    CHECK(rta::places_validate(store, b, 3, logr) == 0, "%s: first of three", what);
    g_rejected++;
}

}  // namespace

int main() {
    // ---- the mapping -------------------------------------------------------------------------------------------------------
    const int32_t odd[4][3] = {{5, 3, 7}, {1, 1, 1}, {1, 9, 3}, {7, 1, 5}};
    for (const auto& E : odd) run_mapping(E);

    // ---- the store ---------------------------------------------------------------------------------------------------------
    rta::StampStore store;
    const int32_t exts[6][3] = {{5, 3, 7}, {1, 1, 1}, {65, 4, 3}, {70, 2, 9}, {256, 256, 256}, {9, 9, 12}};
    std::vector<uint32_t> ids;
    for (const auto& e : exts) {
        rta::StampEntry* s = store.add(e);
        CHECK(s && s->id != 0u && store.find(s->id) == s, "add");
        s = store.find(s->id);
        s->mats = 0x1000u * (ids.size() + 1u); s->state = 0x77000u * (ids.size() + 1u);
        for (uint32_t other : ids) CHECK(other != s->id, "ids repeat");
        ids.push_back(s->id);
    }
    CHECK(!store.find(0u) && !store.find(ids[0] + 1u) && !store.find(ids[0] ^ (1u << 20)) && !store.find(0xFFFFFFFFu), "unknown ids");
    {   // a destroyed id stays unknown when its slot is used again; the limit is 1024 live stamps
        rta::StampStore t;
        const int32_t one[3] = {1, 1, 1};
        std::vector<uint32_t> all;
        for (uint32_t i = 0; i < rta::kMaxStamps; i++) all.push_back(t.add(one)->id);
        CHECK(t.live == rta::kMaxStamps && t.add(one) == nullptr, "the 1025th stamp");
        const uint32_t gone = all[500];
        t.remove(t.find(gone));
        CHECK(!t.find(gone) && t.live == rta::kMaxStamps - 1u, "remove");
        rta::StampEntry* again = t.add(one);
        CHECK(again && again->id != gone && !t.find(gone) && t.find(again->id) == again && t.add(one) == nullptr, "a slot used again");
        std::set<uint32_t> distinct(all.begin(), all.end());
        CHECK(distinct.size() == all.size() && !distinct.count(0u), "1024 distinct non-zero ids");
    }
    const int32_t bad_ext[4][3] = {{0, 1, 1}, {1, 257, 1}, {1, 1, -1}, {256, 256, 257}};
    for (const auto& e : bad_ext) CHECK(!rta::stamp_extent_valid(e), "extent");
    CHECK(rta::stamp_extent_valid(exts[4]) && rta::stamp_extent_valid(exts[1]), "extent limits");

    // ---- valid batches -------------------------------------------------------------------------------------------------------
    rta::ShapeScratch sc;
    for (int logr = 8; logr <= 10; logr++) {
        const int32_t R = 1 << logr;
        run_valid(sc, store, {place(ids[1], 5, 6, 7)}, logr, "one voxel");
        run_valid(sc, store, {place(ids[1], R - 1, R - 1, R - 1), place(ids[1], 0, 0, 0)}, logr, "the corners");
        run_valid(sc, store, {place(ids[1], R, 0, 0), place(ids[1], 0, -1, 0), place(ids[0], -5, 0, 0), place(ids[0], 0, 0, -7, 0)}, logr, "wholly outside");
        run_valid(sc, store, {place(ids[0], -4, 0, 0), place(ids[0], 0, 0, R - 1, 47), place(ids[0], -4 * R, 4 * R, 0, 13)}, logr, "clipped to one layer, and the limits of at");
        run_valid(sc, store, {place(ids[3], 60, 63, 60, 0), place(ids[3], 60, 63, 60, 19), place(ids[3], 60, 63, 60, 38)}, logr, "70 long across a chunk corner");
        run_valid(sc, store, {place(ids[4], 0, 0, 0), place(ids[4], -100, 30, R - 200, 21)}, logr, "256^3");
        std::vector<RtStampPlace> all48;
        for (uint8_t o = 0; o < 48; o++) all48.push_back(place(ids[0], 8 * o, 100, 120, o, (uint8_t)(o % 3)));
        run_valid(sc, store, all48, logr, "48 orientations side by side");
        Rng rng{0x9E3779B97F4A7C15ull + (uint64_t)logr};
        for (int round = 0; round < 40; round++) {
            std::vector<RtStampPlace> batch;
            const uint32_t cnt = 1u + rng.below(40);
            for (uint32_t i = 0; i < cnt; i++) {
                const uint32_t id = ids[rng.below(6)];
                const bool far = rng.below(8) == 0;
                batch.push_back(place(id, far ? rng.between(-4 * R, 4 * R) : rng.between(-80, R + 20), rng.between(-80, R + 20),
                                      far ? rng.between(-4 * R, 4 * R) : rng.between(-300, R + 20), (uint8_t)rng.below(48), (uint8_t)rng.below(3)));
            }
            run_valid(sc, store, batch, logr, "random");
        }
    }

    // ---- rejections ----------------------------------------------------------------------------------------------------------
    for (int logr = 8; logr <= 10; logr += 2) {
        const int32_t R = 1 << logr;
        RtStampPlace p = place(ids[0], 1, 2, 3);
        p.stamp = 0; run_invalid(store, p, logr, "id 0");
        p.stamp = ids[0] ^ (1u << 12); run_invalid(store, p, logr, "another serial");
        p = place(ids[0], 1, 2, 3, 48); run_invalid(store, p, logr, "orient 48");
        p = place(ids[0], 1, 2, 3, 255); run_invalid(store, p, logr, "orient 255");
        p = place(ids[0], 1, 2, 3, 0, 3); run_invalid(store, p, logr, "where 3");
        for (int k = 0; k < 2; k++) { p = place(ids[0], 1, 2, 3); p.reserved0[k] = 1; run_invalid(store, p, logr, "reserved byte"); }
        for (int k = 0; k < 3; k++) { p = place(ids[0], 1, 2, 3); p.reserved[k] = 0x80000000u; run_invalid(store, p, logr, "reserved word"); }
        for (int k = 0; k < 3; k++) {
            p = place(ids[0], 1, 2, 3); p.at[k] = 4 * R + 1; run_invalid(store, p, logr, "at above 4R");
            p = place(ids[0], 1, 2, 3); p.at[k] = -4 * R - 1; run_invalid(store, p, logr, "at below -4R");
            p = place(ids[0], 1, 2, 3); p.at[k] = INT32_MIN; run_invalid(store, p, logr, "at INT32_MIN");
        }
    }
    CHECK(rta::places_validate(store, nullptr, 0, 8) == 0, "an empty batch");

    printf("%ld placements (%ld with a box), %ld rejections, %ld mapped voxels\n", g_places, g_boxed, g_rejected, g_voxels);
    if (g_failures) { fprintf(stderr, "%d checks failed\n", g_failures); return 1; }
    printf("all cases match the model\n");
    return 0;
}
