// Stand-alone check of raytrace_amd/csrc/api/edit_shapes.hpp (the host half of rt_edit_shapes) against a brute-force model written
// from the ABI's words alone: a shape's verdict, its bounding box found by testing every texel of an axis in 64-bit arithmetic, the
// set of 64^3 chunks the boxes meet and the boxes that wait for the next frame.  Built and run by tests/test_edit_shapes_host.py,
// with the sanitizers where the compiler has them.  Exit status 0 = every case passed.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../raytrace_amd/csrc/api/edit_shapes.hpp"

namespace {

int g_failures = 0;
long g_shapes = 0, g_boxed = 0, g_rejected = 0;
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

RtShapeEdit box(int32_t x0, int32_t y0, int32_t z0, int32_t x1, int32_t y1, int32_t z1, uint8_t where = RT_WHERE_ALL) {
    RtShapeEdit s{};
    s.a[0] = x0; s.a[1] = y0; s.a[2] = z0; s.b[0] = x1; s.b[1] = y1; s.b[2] = z1;
    s.kind = RT_SHAPE_BOX; s.where = where; s.solid = 1; s.material = 0x1234u;
    return s;
}
RtShapeEdit sphere(int32_t ax, int32_t ay, int32_t az, int32_t b0, uint8_t where = RT_WHERE_ALL) {
    RtShapeEdit s{};
    s.a[0] = ax; s.a[1] = ay; s.a[2] = az; s.b[0] = b0;
    s.kind = RT_SHAPE_SPHERE; s.where = where; s.solid = 0; s.material = 0x77u;
    return s;
}

// ---- the model ------------------------------------------------------------------------------------------------------------
bool model_valid(const RtShapeEdit& s, int64_t R) {
    if (s.kind > 1 || s.where > 2 || s.reserved != 0) return false;
    for (int k = 0; k < 3; k++) {
        if ((int64_t)s.a[k] < -4 * R || (int64_t)s.a[k] > 4 * R) return false;
        if (s.kind == 0 && ((int64_t)s.b[k] < -4 * R || (int64_t)s.b[k] > 4 * R || s.a[k] > s.b[k])) return false;
    }
    if (s.kind == 1 && (s.b[0] < 0 || (int64_t)s.b[0] > ((int64_t)1 << 26) || s.b[1] != 0 || s.b[2] != 0)) return false;
    return true;
}
struct Box { int64_t lo[3], hi[3]; };
bool model_box(const RtShapeEdit& s, int64_t R, Box* out) {
    for (int k = 0; k < 3; k++) {
        int64_t lo = -1, hi = -1;
        for (int64_t x = 0; x < R; x++) {
            const int64_t d = 2 * x + 1 - (int64_t)s.a[k];
            const bool pass = s.kind == 0 ? ((int64_t)s.a[k] <= x && x <= (int64_t)s.b[k]) : d * d <= (int64_t)s.b[0];
            if (pass) { if (lo < 0) lo = x; hi = x; }
        }
        if (lo < 0) return false;
        out->lo[k] = lo; out->hi[k] = hi;
    }
    return true;
}

// A valid batch: plan, chunk list and pending boxes against the model.
void run_valid(rta::ShapeScratch& sc, const std::vector<RtShapeEdit>& shapes, int logr, const char* what) {
    const int64_t R = (int64_t)1 << logr, n = R / 64;
    const uint32_t count = (uint32_t)shapes.size();
    std::set<uint32_t> want;
    std::vector<Box> boxes;
    for (const RtShapeEdit& s : shapes) {
        CHECK(model_valid(s, R), "%s: the case holds a shape the model rejects", what);
        Box b;
        g_shapes++;
        if (!model_box(s, R, &b)) continue;
        g_boxed++;
        boxes.push_back(b);
        for (int64_t cz = b.lo[2] / 64; cz <= b.hi[2] / 64; cz++)
            for (int64_t cy = b.lo[1] / 64; cy <= b.hi[1] / 64; cy++)
                for (int64_t cx = b.lo[0] / 64; cx <= b.hi[0] / 64; cx++) want.insert((uint32_t)((cz * n + cy) * n + cx));
    }
    const uint32_t r = rta::shapes_validate(shapes.data(), count, logr);
    CHECK(r == count, "%s logr %d: valid batch rejected at %u", what, logr, r);
    if (r != count) return;
    const rta::ShapePlan plan = rta::shapes_touched(sc, shapes.data(), count, logr);
    CHECK(plan.touched == want.size(), "%s logr %d: touched %u, model %zu", what, logr, plan.touched, want.size());
    CHECK(plan.boxes == boxes.size(), "%s logr %d: %u boxes, model %zu", what, logr, plan.boxes, boxes.size());
    CHECK(plan.off_shapes == ((size_t)plan.touched * 4u + 15u) / 16u * 16u, "%s: off_shapes %zu", what, plan.off_shapes);
    CHECK(plan.need == plan.off_shapes + 32u * (size_t)count, "%s: need %zu", what, plan.need);
    if (plan.touched != want.size() || plan.boxes != boxes.size()) return;
    // exactly as many words and boxes as the plan announces, as heap blocks of their own so that the sanitizer sees a write past them
    std::vector<uint32_t> chunks(plan.touched);
    const uint32_t nc = rta::shapes_fill_chunks(sc, chunks.data());
    CHECK(nc == plan.touched, "%s: %u chunk ids written, %u announced", what, nc, plan.touched);
    uint32_t t = 0;
    for (uint32_t c : want) { CHECK(chunks[t] == c, "%s logr %d: chunk[%u] = %u, model %u", what, logr, t, chunks[t], c); t++; }
    std::vector<rta::EditBox> got(plan.boxes);
    const uint32_t nb = rta::shape_pending_boxes(shapes.data(), count, logr, got.data());
    CHECK(nb == plan.boxes, "%s: %u boxes written, %u announced", what, nb, plan.boxes);
    for (uint32_t i = 0; i < nb && i < boxes.size(); i++)
        for (int k = 0; k < 3; k++)
            CHECK(got[i].lo[k] == boxes[i].lo[k] && got[i].hi[k] == boxes[i].hi[k], "%s logr %d: box %u axis %d is %u..%u, model %lld..%lld", what, logr,
                  i, k, got[i].lo[k], got[i].hi[k], (long long)boxes[i].lo[k], (long long)boxes[i].hi[k]);
}

// One shape: the header's verdict and box against the model's, whatever the shape.
void run_one(const RtShapeEdit& s, int logr, const char* what) {
    const int64_t R = (int64_t)1 << logr;
    const bool ok = model_valid(s, R);
    CHECK(rta::shape_valid(s, (int32_t)R) == ok, "%s logr %d: verdict %d, model %d (a %d %d %d, b %d %d %d, kind %u where %u reserved %u)", what, logr,
          (int)!ok, (int)ok, s.a[0], s.a[1], s.a[2], s.b[0], s.b[1], s.b[2], s.kind, s.where, s.reserved);
    CHECK(rta::shapes_validate(&s, 1, logr) == (ok ? 1u : 0u), "%s: shapes_validate of one shape", what);
    if (!ok) { g_rejected++; return; }
    rta::ShapeScratch sc;
    run_valid(sc, {s}, logr, what);
}

RtShapeEdit random_shape(Rng& rng, int32_t R) {
    const uint32_t how = rng.below(8);
    if (rng.below(2)) {
        int32_t a[3], b[3];
        for (int k = 0; k < 3; k++) {
            a[k] = how < 5 ? rng.between(-R / 4, R + R / 4) : rng.between(-4 * R, 4 * R);
            b[k] = how < 5 ? a[k] + rng.between(0, how < 2 ? 3 : R / 2) : rng.between(a[k], 4 * R);
            if (b[k] > 4 * R) b[k] = 4 * R;
        }
        return box(a[0], a[1], a[2], b[0], b[1], b[2], (uint8_t)rng.below(3));
    }
    const int32_t d = how < 2 ? rng.between(0, 4) : how < 6 ? rng.between(0, R) : rng.between(0, 8192);   // 2 r
    const int32_t b0 = how == 3 ? rng.between(0, 1 << 26) : d * d - (how == 4 && d ? 1 : 0);              // (also one below a square)
    const int32_t w = how < 6 ? 2 * R + R / 2 : 4 * R;
    return sphere(rng.between(how < 6 ? -R / 2 : -4 * R, w), rng.between(how < 6 ? -R / 2 : -4 * R, w), rng.between(how < 6 ? -R / 2 : -4 * R, w), b0,
                  (uint8_t)rng.below(3));
}

void run_all(int logr) {
    const int32_t R = 1 << logr;
    Rng rng{0x9E3779B97F4A7C15ull + (uint64_t)logr};
    rta::ShapeScratch sc;   // one for the whole sequence, as the context keeps it

    // boundary shapes
    run_one(box(0, 0, 0, 0, 0, 0), logr, "one voxel at the origin");
    run_one(box(R - 1, R - 1, R - 1, R - 1, R - 1, R - 1), logr, "one voxel at the far corner");
    run_one(box(0, 0, 0, R - 1, R - 1, R - 1), logr, "the whole region");
    run_one(box(-4 * R, -4 * R, -4 * R, 4 * R, 4 * R, 4 * R), logr, "the widest box");
    run_one(box(64, 64, 64, 127, 127, 127), logr, "exactly one chunk");
    run_one(box(63, 63, 63, 64, 64, 64), logr, "2 x 2 x 2 on a chunk corner");
    run_one(box(R, 0, 0, R, 0, 0), logr, "one voxel past the region");
    run_one(box(-1, 0, 0, -1, R - 1, R - 1), logr, "a plane in front of the region");
    run_one(box(-5, -5, -5, 0, 0, 0), logr, "reaches the origin from outside");
    run_one(sphere(21, 21, 21, 49), logr, "radius 3.5 round (10, 10, 10)");
    run_one(sphere(129, 129, 129, 0), logr, "b0 = 0, odd centre: one voxel");
    run_one(sphere(128, 129, 129, 0), logr, "b0 = 0, even centre: none");
    run_one(sphere(128, 128, 128, 1), logr, "b0 = 1, even centre: a box of two texels per axis, nothing selected");
    run_one(sphere(128, 128, 128, 49), logr, "radius 3.5 on a chunk corner");
    run_one(sphere(-9, R, 2 * R + 9, 400), logr, "centred outside, clipped");
    run_one(sphere(-9, R, 2 * R + 9, 99), logr, "centred outside, one short of reaching in");
    run_one(sphere(-9, R, 2 * R + 9, 100), logr, "centred outside, touching one texel");
    run_one(sphere(4 * R, 4 * R, 4 * R, 1 << 26), logr, "the largest sphere, from the far limit");
    run_one(sphere(-4 * R, -4 * R, -4 * R, 1 << 26), logr, "the largest sphere, from the near limit");
    run_one(sphere(R, R, R, (1 << 26) - 1), logr, "one below the largest budget");
    // verdicts at every limit
    for (int k = 0; k < 3; k++)
        for (int32_t v : {-4 * R - 1, -4 * R, 4 * R, 4 * R + 1}) {
            RtShapeEdit s = box(0, 0, 0, 4 * R, 4 * R, 4 * R);
            s.a[k] = v;
            run_one(s, logr, "box a at a limit");
            s = box(-4 * R, -4 * R, -4 * R, 0, 0, 0);
            s.b[k] = v;
            run_one(s, logr, "box b at a limit");
            s = sphere(0, 0, 0, 16);
            s.a[k] = v;
            run_one(s, logr, "sphere a at a limit");
        }
    for (int k = 0; k < 3; k++) { RtShapeEdit s = box(5, 5, 5, 5, 5, 5); s.b[k] = 4; run_one(s, logr, "box with a > b"); }
    for (int32_t v : {-1, 0, 1 << 26, (1 << 26) + 1, INT32_MAX, INT32_MIN}) run_one(sphere(10, 10, 10, v), logr, "sphere b0 at a limit");
    { RtShapeEdit s = sphere(10, 10, 10, 9); s.b[1] = 1; run_one(s, logr, "sphere b1 != 0"); s.b[1] = 0; s.b[2] = -1; run_one(s, logr, "sphere b2 != 0"); }
    for (uint8_t v : {(uint8_t)0, (uint8_t)1, (uint8_t)2, (uint8_t)255}) { RtShapeEdit s = box(1, 1, 1, 2, 2, 2); s.kind = v; run_one(s, logr, "kind"); }
    for (uint8_t v : {(uint8_t)2, (uint8_t)3, (uint8_t)255}) { RtShapeEdit s = box(1, 1, 1, 2, 2, 2); s.where = v; run_one(s, logr, "where"); }
    { RtShapeEdit s = box(1, 1, 1, 2, 2, 2); s.reserved = 1; run_one(s, logr, "reserved"); s.reserved = 0; s.solid = 255; run_one(s, logr, "solid 255"); }

    // seeded random shapes one by one (verdict and box), then as batches with the scratch kept between them
    for (int i = 0; i < 600; i++) {
        RtShapeEdit s = random_shape(rng, R);
        if (rng.below(10) == 0) {   // spoil one field
            switch (rng.below(5)) {
                case 0: s.a[rng.below(3)] = rng.below(2) ? 4 * R + 1 + (int32_t)rng.below(100) : -4 * R - 1 - (int32_t)rng.below(100); break;
                case 1: s.b[rng.below(3)] = rng.below(2) ? 4 * R + 1 + (int32_t)rng.below(100) : -1 - (int32_t)rng.below(100); break;
                case 2: s.kind = (uint8_t)(2 + rng.below(254)); break;
                case 3: s.where = (uint8_t)(3 + rng.below(253)); break;
                default: s.reserved = (uint8_t)(1 + rng.below(255)); break;
            }
        }
        run_one(s, logr, "random shape");
    }
    for (uint32_t n : {1u, 2u, 17u, 300u, 4096u}) {
        std::vector<RtShapeEdit> v;
        while (v.size() < n) { const RtShapeEdit s = random_shape(rng, R); if (model_valid(s, R)) v.push_back(s); }
        run_valid(sc, v, logr, "random batch");
        // a batch with one bad shape reports its index
        const uint32_t at = rng.below(n);
        std::vector<RtShapeEdit> w = v;
        w[at].reserved = 7;
        CHECK(rta::shapes_validate(w.data(), n, logr) == at, "bad shape at %u of %u not reported", at, n);
    }
    run_valid(sc, {box(-9, -9, -9, -1, -1, -1), sphere(-100, 5, 5, 16)}, logr, "nothing inside: no chunk, no box");
    run_valid(sc, {}, logr, "an empty batch");
}

}  // namespace

int main() {
    for (int32_t v : {0, 1, 2, 3, 4, 48, 49, 50, (1 << 26) - 1, 1 << 26, 8191 * 8191, 8191 * 8191 - 1}) {
        const int32_t s = rta::shape_isqrt(v);
        CHECK((int64_t)s * s <= v && (int64_t)(s + 1) * (s + 1) > v, "isqrt(%d) = %d", v, s);
    }
    run_all(8);
    run_all(9);
    run_all(10);
    CHECK(g_boxed > 500 && g_shapes - g_boxed > 50 && g_rejected > 100, "the cases are one-sided: %ld shapes, %ld with a box, %ld rejected", g_shapes, g_boxed, g_rejected);
    if (g_failures) { fprintf(stderr, "%d checks failed\n", g_failures); return 1; }
    printf("edit shapes: all cases match the model (%ld shapes, %ld with a bounding box, %ld rejected)\n", g_shapes, g_boxed, g_rejected);
    return 0;
}
