// Stand-alone check of raytrace_amd/csrc/api/entity_query_check.hpp (the host half of rt_trace_entities / rt_trace_entities_async /
// rt_pick_entities that needs no context) against a model written from the ABI's words alone: a table of the plain arguments (the
// counts at and past 2^24 and 4096, NULL pointers against their counts), the pixel range at every edge of a frame, and the boxes'
// validity through shadows_check.hpp's one host definition, with the first invalid box at every position.  Built and run by
// tests/test_entity_query_abi.py, with the sanitizers where the compiler has them.  Exit status 0 = every case passed.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../raytrace_amd/csrc/api/entity_query_check.hpp"

namespace {

int g_failures = 0;
long g_cases = 0;
#define CHECK(cond, ...)                                                            \
    do {                                                                            \
        if (!(cond)) {                                                              \
            if (g_failures++ < 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } \
        }                                                                           \
    } while (0)

// "NULL rays / xy / u / lr / entity_hits with count > 0; a NULL entity array with its count above 0; count > 2^24; nboxes or nmodels
// above 4096"
bool model_args_ok(uint64_t count, bool in, bool more, bool hits, bool boxes, uint64_t nboxes, bool models, uint64_t nmodels) {
    if (count > 16777216ull || nboxes > 4096ull || nmodels > 4096ull) return false;
    if (count > 0 && !(in && more && hits)) return false;
    if (nboxes > 0 && !boxes) return false;
    if (nmodels > 0 && !models) return false;
    return true;
}

// "a pixel outside the frame"
bool model_pixel_inside(long x, long y, long w, long h) { return x >= 0 && y >= 0 && x < w && y < h; }

RtDrawBox good() {
    RtDrawBox b{};
    b.lo[0] = 1.5f; b.lo[1] = -128.0f; b.lo[2] = 100.0f;
    b.hi[0] = 2.5f; b.hi[1] = -127.0f; b.hi[2] = 101.75f;
    return b;
}

}  // namespace

int main() {
    static_assert(sizeof(RtEntityHit) == 48 && sizeof(RtRayHit) == 48 && sizeof(RtDrawBox) == 32 && sizeof(RtDrawStamp) == 32, "record sizes");
    static_assert(rta::kMaxEntityRays == (1u << 24) && rta::kMaxEntityBoxes == 4096 && rta::kMaxEntityModels == 4096, "limits of a call");
    static_assert(RT_ENTITY_NONE == 0 && RT_ENTITY_BOX == 1 && RT_ENTITY_MODEL == 2, "kinds");

    // ---- the plain arguments: the whole table ----
    const int something = 0;
    const std::vector<uint32_t> counts = {0u, 1u, 64u, (1u << 24) - 1u, 1u << 24, (1u << 24) + 1u, 1u << 26, 0xFFFFFFFFu};
    const std::vector<uint32_t> entities = {0u, 1u, 64u, 4095u, 4096u, 4097u, 0x7FFFFFFFu, 0xFFFFFFFFu};
    long ok = 0, bad = 0;
    for (int mask = 0; mask < 32; mask++) {
        const void* in = (mask & 1) ? &something : nullptr;
        const void* more = (mask & 2) ? &something : nullptr;
        const void* hits = (mask & 4) ? &something : nullptr;
        const void* boxes = (mask & 8) ? &something : nullptr;
        const void* models = (mask & 16) ? &something : nullptr;
        for (uint32_t count : counts)
            for (uint32_t nb : entities)
                for (uint32_t nm : entities) {
                    const bool want = model_args_ok(count, in, more, hits, boxes, nb, models, nm);
                    const char* got = rta::entity_query_args_error(count, in, more, hits, boxes, nb, models, nm);
                    (want ? ok : bad)++;
                    g_cases++;
                    CHECK((got == nullptr) == want, "count %u in %d more %d hits %d boxes %d x %u models %d x %u: model says %d, header says %s", count,
                          in != nullptr, more != nullptr, hits != nullptr, boxes != nullptr, nb, models != nullptr, nm, (int)want, got ? got : "fine");
                }
    }
    CHECK(ok > 100 && bad > 100, "both verdicts occur: %ld fine, %ld refused", ok, bad);
    CHECK(rta::entity_query_args_error(0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0) == nullptr, "an empty call needs no pointer");
    CHECK(rta::entity_query_args_error(5, &something, &something, &something, nullptr, 0, nullptr, 0) == nullptr, "no entities need no arrays");
    CHECK(rta::entity_query_args_error(0, nullptr, nullptr, nullptr, nullptr, 4097, nullptr, 0) != nullptr, "the limits hold for an empty call too");

    // ---- pixels against the frame ----
    const int32_t imin = std::numeric_limits<int32_t>::min(), imax = std::numeric_limits<int32_t>::max();
    for (int32_t w : {1, 2, 100, 4096})
        for (int32_t h : {1, 3, 60, 2160}) {
            const std::vector<int32_t> xs = {imin, -1, 0, 1, w - 1, w, w + 1, imax}, ys = {imin, -1, 0, 1, h - 1, h, h + 1, imax};
            for (int32_t x : xs)
                for (int32_t y : ys) {
                    const int32_t one[2] = {x, y};
                    const bool want = model_pixel_inside(x, y, w, h);
                    g_cases++;
                    CHECK((rta::first_pixel_outside(one, 1, w, h) == 1u) == want, "pixel %d %d of %d x %d: model says %d", x, y, w, h, (int)want);
                }
            // the first pixel outside at every position of a batch, and none
            for (uint32_t n : {0u, 1u, 2u, 65u}) {
                std::vector<int32_t> xy(2u * n + 2u, 0);
                for (uint32_t i = 0; i < n; i++) { xy[2u * i] = (int32_t)(i % (uint32_t)w); xy[2u * i + 1u] = (int32_t)(i % (uint32_t)h); }
                CHECK(rta::first_pixel_outside(xy.data(), n, w, h) == n, "a batch of %u pixels inside %d x %d", n, w, h);
                for (uint32_t at = 0; at < n; at++) {
                    std::vector<int32_t> b = xy;
                    b[2u * at + (at & 1u)] = (at & 2u) ? -1 : ((at & 1u) ? h : w);
                    if (at + 1u < n) b[2u * (n - 1u)] = -7;
                    g_cases++;
                    CHECK(rta::first_pixel_outside(b.data(), n, w, h) == at, "batch of %u, first pixel outside at %u", n, at);
                }
            }
        }
    CHECK(rta::first_pixel_outside(nullptr, 0, 100, 60) == 0u, "an empty batch reads nothing");

    // ---- the boxes: the synchronous calls refuse the first invalid one (rt_draw_boxes' valid box) ----
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (uint32_t n : {0u, 1u, 63u, 64u, 65u, 4096u}) {
        std::vector<RtDrawBox> batch(n, good());
        CHECK(rta::first_invalid_draw_box(batch.data(), n) == n, "a batch of %u valid boxes", n);
        for (uint32_t at = 0; at < n; at += (n > 70u ? 389u : 1u)) {
            std::vector<RtDrawBox> b = batch;
            switch (at % 4u) {
                case 0: b[at].hi[1] = b[at].lo[1]; break;
                case 1: b[at].lo[0] = nan; break;
                case 2: b[at].hi[2] = inf; break;
                default: b[at].lo[2] = -4194305.0f; break;
            }
            if (at + 1u < n) b[n - 1u].lo[2] = nan;
            g_cases++;
            CHECK(rta::first_invalid_draw_box(b.data(), n) == at, "batch of %u, first invalid at %u", n, at);
        }
    }

    if (g_failures) { fprintf(stderr, "%d failures in %ld cases\n", g_failures, g_cases); return 1; }
    printf("all cases match the model (%ld cases)\n", g_cases);
    return 0;
}
