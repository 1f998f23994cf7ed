// Stand-alone check of raytrace_amd/csrc/api/draw_stamps.hpp (the host half of the voxel-model entities) against a brute-force model
// written from the ABI's words alone: a record's verdict with the high corner computed in extended precision, the device record's
// fields, the packing of strides and extents at their extremes, and — voxel by voxel, for every orientation of a few odd extents —
// that the cell a record's base and strides address is the stamp voxel the header names.  Built and run by
// tests/test_draw_stamps_host.py, with the sanitizers where the compiler has them.  Exit status 0 = every case passed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytrace_amd/csrc/api/draw_stamps.hpp"

namespace {

int g_failures = 0;
long g_records = 0, g_rejected = 0, g_voxels = 0;
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
    float unit() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }
};

// ---- the model: the header's words ------------------------------------------------------------------------------------------
const int kPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
const float kBig = 4194304.0f;

// rtm_fma(float(e), scale, origin) without an fma: the product is exact in 64 bits of mantissa, the sum rounded once more only
// when origin and the product are more than 30 binary orders apart
float model_hi(int e, float scale, float origin) { return (float)((long double)e * (long double)scale + (long double)origin); }

bool model_valid(const RtDrawStamp& m, const int32_t* E /* null: no such stamp */) {
    if (!E || m.orient >= 48 || m.reserved0[0] || m.reserved0[1] || m.reserved0[2] || m.reserved) return false;
    if (!std::isfinite(m.scale) || m.scale < 1.0f / 256.0f || m.scale > 64.0f) return false;
    for (int k = 0; k < 3; k++) {
        if (!std::isfinite(m.origin[k]) || std::fabs(m.origin[k]) > kBig) return false;
        const float hi = model_hi(E[kPerm[m.orient >> 3][k]], m.scale, m.origin[k]);
        if (std::fabs(hi) > kBig) return false;
    }
    return true;
}
// the stamp voxel (x, y, z) that placed-local cell c shows
void model_source(const int32_t E[3], uint32_t orient, const int c[3], int s[3]) {
    const int* perm = kPerm[orient >> 3];
    const uint32_t f = orient & 7u;
    for (int k = 0; k < 3; k++) s[perm[k]] = ((f >> perm[k]) & 1u) ? E[perm[k]] - 1 - c[k] : c[k];
}

RtDrawStamp record(uint32_t id, float x, float y, float z, float scale, uint8_t orient, uint32_t emission = 0xFF000000u) {
    RtDrawStamp m{};
    m.origin[0] = x; m.origin[1] = y; m.origin[2] = z; m.scale = scale; m.stamp = id; m.orient = orient; m.emission = emission;
    return m;
}

// ---- packing ----------------------------------------------------------------------------------------------------------------
void run_packing() {
    const int32_t strides[] = {1, -1, 2, -2, 255, -255, 256, -256, 65535, -65535, 65536, -65536};
    for (int32_t s : strides)
        for (int32_t e : {1, 2, 3, 128, 255, 256}) {
            const uint32_t w = rta::draw_stamp_pack(s, e);
            CHECK(rta::draw_stamp_stride(w) == s && rta::draw_stamp_ext(w) == e, "stride %d ext %d -> %08x -> %d %d", s, e, w,
                  rta::draw_stamp_stride(w), rta::draw_stamp_ext(w));
            CHECK((w >> 26) == 0u, "bits above the extent are clear");
        }
}

// ---- every orientation of a few extents, every voxel ---------------------------------------------------------------------------
void run_mapping(rta::StampStore& st, const int32_t E[3]) {
    rta::StampEntry* e = st.add(E);
    e->mats = 0x100000000ull + 4096u * (uint64_t)g_voxels;
    e->state = 0x200000000ull + 4096u * (uint64_t)g_voxels;
    for (uint32_t orient = 0; orient < 48; orient++) {
        const RtDrawStamp m = record(e->id, 1.5f, -2.25f, 3.0f, 0.37f, (uint8_t)orient, 0x80402010u + orient);
        CHECK(rta::draw_stamps_validate(st, &m, 1) == 1u, "orient %u is valid", orient);
        rta::DrawStampRecord r;
        memset(&r, 0xAB, sizeof r);
        rta::draw_stamp_fill_records(st, &m, 1, &r);
        CHECK(r.mats == e->mats && r.state == e->state && r.emission == m.emission && r.scale == m.scale, "orient %u: copied fields", orient);
        int ext[3], stride[3];
        for (int k = 0; k < 3; k++) {
            ext[k] = rta::draw_stamp_ext(r.se[k]);
            stride[k] = rta::draw_stamp_stride(r.se[k]);
            CHECK(ext[k] == E[kPerm[orient >> 3][k]], "orient %u axis %d: E' %d", orient, k, ext[k]);
            CHECK(r.origin[k] == m.origin[k] && r.hi[k] == model_hi(ext[k], m.scale, m.origin[k]), "orient %u axis %d: corners", orient, k);
        }
        std::vector<uint8_t> seen((size_t)E[0] * E[1] * E[2], 0);
        int c[3];
        for (c[2] = 0; c[2] < ext[2]; c[2]++)
            for (c[1] = 0; c[1] < ext[1]; c[1]++)
                for (c[0] = 0; c[0] < ext[0]; c[0]++) {
                    int s[3];
                    model_source(E, orient, c, s);
                    const long want = ((long)s[2] * E[1] + s[1]) * E[0] + s[0];
                    const long got = (long)r.base + (long)stride[0] * c[0] + (long)stride[1] * c[1] + (long)stride[2] * c[2];
                    CHECK(got == want, "orient %u cell (%d, %d, %d): voxel %ld, the header says %ld", orient, c[0], c[1], c[2], got, want);
                    if (got >= 0 && got < (long)seen.size()) seen[(size_t)got]++;
                    g_voxels++;
                }
        for (uint8_t v : seen) CHECK(v == 1, "orient %u: every voxel is shown once", orient);
    }
}

// ---- verdicts ---------------------------------------------------------------------------------------------------------------
void check_verdict(const rta::StampStore& st, const RtDrawStamp& m, const char* what) {
    const rta::StampEntry* e = st.find(m.stamp);
    const bool want = model_valid(m, e ? e->ext : nullptr);
    const RtDrawStamp two[2] = {record(st.slots[0].id, 0.0f, 0.0f, 0.0f, 1.0f, 0), m};
    const uint32_t got = rta::draw_stamps_validate(st, two, 2);
    CHECK(got == (want ? 2u : 1u), "%s: the header says %s", what, want ? "valid" : "invalid");
    g_records++;
    g_rejected += !want;
}

void run_verdicts(rta::StampStore& st, Rng& rng) {
    const uint32_t id = st.slots[0].id;                  // the first stamp made: extent 3 x 5 x 7
    const float inf = INFINITY, nan = NAN;
    const float below_min = std::nextafterf(1.0f / 256.0f, 0.0f), above_max = std::nextafterf(64.0f, 100.0f), past = std::nextafterf(kBig, 1e9f);
    RtDrawStamp m = record(id, 1.0f, 2.0f, 3.0f, 0.5f, 0);
    check_verdict(st, m, "a plain record");
    check_verdict(st, record(0u, 0, 0, 0, 1, 0), "id 0");
    check_verdict(st, record(id + (1u << 10), 0, 0, 0, 1, 0), "another serial");
    check_verdict(st, record(id ^ 5u, 0, 0, 0, 1, 0), "another slot");
    check_verdict(st, record(id, 0, 0, 0, 1, 47), "orient 47");
    check_verdict(st, record(id, 0, 0, 0, 1, 48), "orient 48");
    check_verdict(st, record(id, 0, 0, 0, 1, 255), "orient 255");
    for (int b = 0; b < 3; b++) { RtDrawStamp r = m; r.reserved0[b] = 1; check_verdict(st, r, "a reserved byte"); }
    { RtDrawStamp r = m; r.reserved = 0x80000000u; check_verdict(st, r, "the reserved word"); }
    for (float s : {1.0f / 256.0f, 64.0f, below_min, above_max, 0.0f, -1.0f, inf, -inf, nan, 1e-40f}) check_verdict(st, record(id, 0, 0, 0, s, 0), "a scale");
    for (int k = 0; k < 3; k++)
        for (float v : {kBig, -kBig, past, -past, inf, -inf, nan, kBig - 1.5f, kBig - 2.0f, kBig - 3.5f, kBig - 4.0f}) {
            for (uint8_t orient : {(uint8_t)0, (uint8_t)(3 << 3), (uint8_t)(5 << 3 | 7)}) {
                RtDrawStamp r = record(id, 0.0f, 0.0f, 0.0f, 0.5f, orient);
                r.origin[k] = v;
                check_verdict(st, r, "a corner near 2^22");
            }
        }
    // random records round the limits
    for (int i = 0; i < 200000; i++) {
        const rta::StampEntry& e = st.slots[rng.below((uint32_t)st.slots.size())];
        RtDrawStamp r = record(rng.below(16) ? e.id : e.id + rng.below(3) * 1024u + rng.below(2), 0, 0, 0, 1, (uint8_t)rng.below(rng.below(8) ? 48 : 64));
        for (int k = 0; k < 3; k++) {
            const uint32_t how = rng.below(8);
            r.origin[k] = how == 0 ? (rng.below(2) ? kBig : -kBig) - (float)rng.below(4096) * 0.25f * (rng.below(2) ? 1.0f : -1.0f)
                          : how == 1 ? (rng.unit() - 0.5f) * 1.0e-20f
                                     : (rng.unit() - 0.5f) * 2.0f * kBig * (how == 2 ? 1.001f : 1.0f);
        }
        const uint32_t hows = rng.below(8);
        r.scale = hows == 0 ? 1.0f / 256.0f + (float)((int)rng.below(5) - 2) * 4.6566e-10f : hows == 1 ? 64.0f + (float)((int)rng.below(5) - 2) * 7.6e-6f
                                                                                                        : 1.0f / 256.0f + rng.unit() * 64.0f;
        if (!rng.below(64)) r.reserved = rng.next();
        if (!rng.below(64)) r.reserved0[rng.below(3)] = (uint8_t)rng.next();
        check_verdict(st, r, "a random record");
    }
}

}  // namespace

int main() {
    static_assert(sizeof(RtDrawStamp) == 32, "RtDrawStamp is 32 bytes");
    rta::StampStore st;
    run_packing();
    const int32_t exts[][3] = {{3, 5, 7}, {1, 1, 1}, {9, 9, 12}, {256, 1, 3}, {2, 256, 1}, {1, 2, 256}, {4, 4, 4}};
    for (const auto& E : exts) run_mapping(st, E);
    Rng rng{0x9E3779B97F4A7C15ull};
    run_verdicts(st, rng);
    CHECK(g_rejected > g_records / 20 && g_rejected < g_records - g_records / 20, "%ld of %ld records rejected", g_rejected, g_records);
    // a batch: the index of the first invalid record, and records in batch order
    {
        std::vector<RtDrawStamp> batch;
        for (int i = 0; i < 100; i++) batch.push_back(record(st.slots[(size_t)i % st.slots.size()].id, (float)i, 0.5f, -3.0f, 0.25f, (uint8_t)(i % 48), (uint32_t)i));
        CHECK(rta::draw_stamps_validate(st, batch.data(), 100) == 100u, "a valid batch");
        std::vector<rta::DrawStampRecord> recs(100);
        rta::draw_stamp_fill_records(st, batch.data(), 100, recs.data());
        for (int i = 0; i < 100; i++) CHECK(recs[(size_t)i].emission == (uint32_t)i && recs[(size_t)i].origin[0] == (float)i, "record %d in its place", i);
        batch[57].orient = 48;
        batch[80].scale = 0.0f;
        CHECK(rta::draw_stamps_validate(st, batch.data(), 100) == 57u, "the first invalid record");
        CHECK(rta::draw_stamps_validate(st, batch.data(), 57) == 57u, "the records before it");
        CHECK(rta::draw_stamps_validate(st, batch.data(), 0) == 0u, "an empty batch");
    }
    if (g_failures) {
        fprintf(stderr, "%d checks failed\n", g_failures);
        return 1;
    }
    printf("all cases match the model: %ld records (%ld rejected), %ld voxels over 48 orientations\n", g_records, g_rejected, g_voxels);
    return 0;
}
