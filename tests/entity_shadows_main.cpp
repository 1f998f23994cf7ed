// Stand-alone check of raytrace_amd/csrc/api/shadows_check.hpp (the host half of rt_shadow_entities that needs no context) against
// a model written from the ABI's words alone, in double precision with std::isfinite: the plain arguments (NULL pointers against
// their counts, the counts at and past 4096, `strength` at, just inside and just outside (0, 1], NaNs and infinities), the occluder
// box with every field at its bounds and with random bit patterns, batches whose first invalid box sits at every position, and the
// night test of a sun colour.  Built and run by tests/test_entity_shadow_abi.py, with the sanitizers where the compiler has them.
// Exit status 0 = every case passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../raytrace_amd/csrc/api/shadows_check.hpp"

namespace {

int g_failures = 0;
long g_cases = 0, g_valid = 0;
#define CHECK(cond, ...)                                                            \
    do {                                                                            \
        if (!(cond)) {                                                              \
            if (g_failures++ < 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } \
        }                                                                           \
    } while (0)

struct Rng {   // xorshift64*
    uint64_t s;
    uint32_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32); }
};

// "every float finite, |lo_k|, |hi_k| <= 2^22 and lo_k < hi_k on every axis"
bool model_box_valid(const RtDrawBox& b) {
    for (int k = 0; k < 3; k++) {
        const double lo = b.lo[k], hi = b.hi[k];
        if (!std::isfinite(lo) || !std::isfinite(hi)) return false;
        if (lo > 4194304.0 || lo < -4194304.0 || hi > 4194304.0 || hi < -4194304.0) return false;
        if (!(lo < hi)) return false;
    }
    return true;
}

// "a NULL u; a NULL array with its count above 0; a count above 4096; strength not finite or outside (0, 1]"
bool model_args_ok(const void* u, const void* boxes, uint32_t nboxes, const void* models, uint32_t nmodels, float strength) {
    if (!u) return false;
    if ((nboxes > 0 && !boxes) || (nmodels > 0 && !models)) return false;
    if (nboxes > 4096 || nmodels > 4096) return false;
    const double s = strength;
    return std::isfinite(s) && s > 0.0 && s <= 1.0;
}

RtDrawBox good() {
    RtDrawBox b{};
    b.lo[0] = 1.5f; b.lo[1] = -128.0f; b.lo[2] = 100.0f;
    b.hi[0] = 2.5f; b.hi[1] = -127.0f; b.hi[2] = 101.75f;
    b.material = 0x12345u; b.emission = 0xFF000000u;
    return b;
}

void check_box(const RtDrawBox& b) {
    g_cases++;
    const bool want = model_box_valid(b);
    g_valid += want;
    CHECK(rta::draw_box_valid(b) == want, "lo %g %g %g hi %g %g %g: model says %d", b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2], (int)want);
}

float* field(RtDrawBox& b, int f) { return f < 3 ? &b.lo[f] : &b.hi[f - 3]; }

}  // namespace

int main() {
    static_assert(sizeof(RtDrawBox) == 32, "RtDrawBox is 32 bytes");
    static_assert(rta::kMaxEntityBoxes == 4096 && rta::kMaxEntityModels == 4096, "occluders per call");
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float denorm = std::numeric_limits<float>::denorm_min(), big = std::numeric_limits<float>::max();

    // ---- the plain arguments ----
    const int something = 0;
    const std::vector<float> strengths = {1.0f, 0.5f, denorm, std::nextafter(1.0f, 0.0f), std::nextafter(1.0f, 2.0f), 0.0f, -0.0f, -denorm, -1.0f,
                                          2.0f, big, -big, inf, -inf, nan, -nan};
    const std::vector<uint32_t> counts = {0u, 1u, 64u, 4095u, 4096u, 4097u, 0x7FFFFFFFu, 0xFFFFFFFFu};
    long args_ok = 0, args_bad = 0;
    for (const void* u : {(const void*)&something, (const void*)nullptr})
        for (const void* boxes : {(const void*)&something, (const void*)nullptr})
            for (const void* models : {(const void*)&something, (const void*)nullptr})
                for (uint32_t nb : counts)
                    for (uint32_t nm : counts)
                        for (float s : strengths) {
                            const bool want = model_args_ok(u, boxes, nb, models, nm, s);
                            const char* got = rta::shadow_args_error(u, boxes, nb, models, nm, s);
                            (want ? args_ok : args_bad)++;
                            g_cases++;
                            CHECK((got == nullptr) == want, "u %d boxes %d x %u models %d x %u strength %g: model says %d, header says %s", u != nullptr,
                                  boxes != nullptr, nb, models != nullptr, nm, s, (int)want, got ? got : "fine");
                        }
    CHECK(args_ok > 100 && args_bad > 100, "both verdicts occur: %ld fine, %ld refused", args_ok, args_bad);
    CHECK(rta::shadow_args_error(&something, nullptr, 0, nullptr, 0, 1.0f) == nullptr, "no occluders need no arrays");

    // ---- one box ----
    std::vector<float> probes = {0.0f, -0.0f, denorm, -denorm, 1.0f, -1.0f, 4194304.0f, -4194304.0f, std::nextafter(4194304.0f, inf),
                                 std::nextafter(-4194304.0f, -inf), std::nextafter(4194304.0f, 0.0f), std::nextafter(-4194304.0f, 0.0f), big, -big, inf,
                                 -inf, nan, -nan};
    check_box(good());
    CHECK(rta::draw_box_valid(good()), "the plain box is valid");
    for (int f = 0; f < 6; f++)
        for (float v : probes) {
            RtDrawBox b = good();
            *field(b, f) = v;
            check_box(b);
            // ... and its partner on the same axis at the far bound, so that lo < hi can hold at the limits
            *field(b, f < 3 ? f + 3 : f - 3) = f < 3 ? 4194304.0f : -4194304.0f;
            check_box(b);
        }
    for (int k = 0; k < 3; k++) {   // lo == hi, lo one ulp below hi, lo above hi
        RtDrawBox b = good();
        b.lo[k] = b.hi[k];
        check_box(b);
        b.lo[k] = std::nextafter(b.hi[k], -inf);
        check_box(b);
        b.lo[k] = std::nextafter(b.hi[k], inf);
        check_box(b);
    }
    {   // material and emission play no part
        RtDrawBox b = good();
        b.material = 0xFFFFFFFFu; b.emission = 0u;
        check_box(b);
        CHECK(rta::draw_box_valid(b), "material and emission are not looked at");
    }
    Rng rng{0x9E3779B97F4A7C15ull};
    for (int i = 0; i < 200000; i++) {   // random bit patterns in every float field: every class of float turns up
        RtDrawBox b = good();
        const int f = (int)(rng.next() % 6u);
        const uint32_t bits = rng.next();
        std::memcpy(field(b, f), &bits, 4);
        check_box(b);
    }

    // ---- batches: the first invalid box at every position, and none ----
    for (uint32_t n : {0u, 1u, 2u, 63u, 64u, 65u, 4096u}) {
        std::vector<RtDrawBox> batch(n, good());
        CHECK(rta::first_invalid_draw_box(batch.data(), n) == n, "a batch of %u valid boxes", n);
        for (uint32_t bad = 0; bad < n; bad += (n > 70u ? 389u : 1u)) {
            std::vector<RtDrawBox> b = batch;
            b[bad].hi[1] = b[bad].lo[1];
            if (bad + 1u < n) b[n - 1u].lo[2] = nan;
            CHECK(rta::first_invalid_draw_box(b.data(), n) == bad, "batch of %u, first invalid at %u", n, bad);
            g_cases++;
        }
    }
    CHECK(rta::first_invalid_draw_box(nullptr, 0) == 0, "an empty batch reads nothing");

    // ---- night ----
    {
        const float day[3] = {1.9294f, 1.5686f, 1.7648f}, below[3] = {-1.4824f, -0.4314f, -0.3372f}, zero[3] = {0.0f, -0.0f, 0.0f};
        const float one[3] = {0.0f, 0.0f, denorm}, nans[3] = {nan, 0.0f, 0.0f};
        CHECK(!rta::shadow_sun_is_dark(day) && !rta::shadow_sun_is_dark(below) && !rta::shadow_sun_is_dark(one) && !rta::shadow_sun_is_dark(nans),
              "a sun colour with a non-zero channel is not the night");
        CHECK(rta::shadow_sun_is_dark(zero), "(0, -0, 0) is the night");
        g_cases += 5;
    }

    CHECK(g_valid > 1000 && g_cases - g_valid > 1000, "both verdicts occur: %ld valid of %ld", g_valid, g_cases);
    if (g_failures) { fprintf(stderr, "%d failures in %ld cases\n", g_failures, g_cases); return 1; }
    printf("all cases match the model (%ld cases, %ld valid boxes)\n", g_cases, g_valid);
    return 0;
}
