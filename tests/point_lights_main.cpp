// Stand-alone check of raytrace_amd/csrc/api/lights_check.hpp (the host half of rt_add_lights) against a model written from the ABI's
// words alone, in double precision with std::isfinite: every field at, just inside and just outside each of its bounds, NaNs and
// infinities of both signs, every bit pattern class of a float in every field, and batches whose first invalid record sits at every
// position.  Built and run by tests/test_point_light_abi.py, with the sanitizers where the compiler has them.  Exit status 0 = every
// case passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../raytrace_amd/csrc/api/lights_check.hpp"

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

// "every float finite, |position_k| <= 2^22, 0 < radius <= 1024, 0 <= color_k <= 2^20, reserved == 0"
bool model_valid(const RtPointLight& l) {
    if (l.reserved != 0) return false;
    const double r = l.radius;
    if (!std::isfinite(r) || !(r > 0.0) || r > 1024.0) return false;
    for (int k = 0; k < 3; k++) {
        const double p = l.position[k], c = l.color[k];
        if (!std::isfinite(p) || !std::isfinite(c)) return false;
        if (p > 4194304.0 || p < -4194304.0) return false;
        if (c < 0.0 || c > 1048576.0) return false;
    }
    return true;
}

RtPointLight good() {
    RtPointLight l{};
    l.position[0] = 1.5f; l.position[1] = -128.0f; l.position[2] = 100.0f;
    l.radius = 8.0f;
    l.color[0] = 30.0f; l.color[1] = 20.0f; l.color[2] = 0.0f;
    return l;
}

void check_one(const RtPointLight& l) {
    g_cases++;
    const bool want = model_valid(l);
    g_valid += want;
    CHECK(rta::point_light_valid(l) == want, "position %g %g %g radius %g color %g %g %g reserved %u: model says %d", l.position[0], l.position[1],
          l.position[2], l.radius, l.color[0], l.color[1], l.color[2], l.reserved, (int)want);
}

float* field(RtPointLight& l, int f) { return f < 3 ? &l.position[f] : (f == 3 ? &l.radius : &l.color[f - 4]); }

}  // namespace

int main() {
    static_assert(sizeof(RtPointLight) == 32, "RtPointLight is 32 bytes");
    static_assert(rta::kMaxPointLights == 1024, "lights per call");
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float denorm = std::numeric_limits<float>::denorm_min(), big = std::numeric_limits<float>::max();
    std::vector<float> probes = {0.0f, -0.0f, denorm, -denorm, 1.0f, -1.0f, 1024.0f, std::nextafter(1024.0f, inf), std::nextafter(1024.0f, 0.0f),
                                 1048576.0f, std::nextafter(1048576.0f, inf), std::nextafter(1048576.0f, 0.0f), 4194304.0f, -4194304.0f,
                                 std::nextafter(4194304.0f, inf), std::nextafter(-4194304.0f, -inf), std::nextafter(4194304.0f, 0.0f), big, -big,
                                 inf, -inf, nan, -nan};
    check_one(good());
    CHECK(rta::point_light_valid(good()), "the plain light is valid");
    for (int f = 0; f < 7; f++)
        for (float v : probes) {
            RtPointLight l = good();
            *field(l, f) = v;
            check_one(l);
        }
    for (uint32_t r : {1u, 0x80000000u, 0xFFFFFFFFu}) {
        RtPointLight l = good();
        l.reserved = r;
        check_one(l);
    }
    // random bit patterns in every float field: every class of float turns up
    Rng rng{0x9E3779B97F4A7C15ull};
    for (int i = 0; i < 200000; i++) {
        RtPointLight l = good();
        const int f = (int)(rng.next() % 7u);
        const uint32_t bits = rng.next();
        std::memcpy(field(l, f), &bits, 4);
        if (rng.next() % 16u == 0u) l.reserved = rng.next() % 2u;
        check_one(l);
    }
    // batches: the first invalid record at every position, and none
    for (uint32_t n : {0u, 1u, 2u, 63u, 64u, 65u, 1024u}) {
        std::vector<RtPointLight> batch(n, good());
        CHECK(rta::first_invalid_point_light(batch.data(), n) == n, "a batch of %u valid lights", n);
        for (uint32_t bad = 0; bad < n; bad += (n > 70u ? 97u : 1u)) {
            std::vector<RtPointLight> b = batch;
            b[bad].radius = 0.0f;
            if (bad + 1u < n) b[n - 1u].color[1] = nan;
            CHECK(rta::first_invalid_point_light(b.data(), n) == bad, "batch of %u, first invalid at %u", n, bad);
            g_cases++;
        }
    }
    CHECK(rta::first_invalid_point_light(nullptr, 0) == 0, "an empty batch reads nothing");
    CHECK(g_valid > 1000 && g_cases - g_valid > 1000, "both verdicts occur: %ld valid of %ld", g_valid, g_cases);
    if (g_failures) { fprintf(stderr, "%d failures in %ld cases\n", g_failures, g_cases); return 1; }
    printf("all cases match the model (%ld cases, %ld valid)\n", g_cases, g_valid);
    return 0;
}
