// Stand-alone check of raytrace_amd/csrc/api/light_shadows_check.hpp (the host half of rt_add_lights_occluded that needs no context)
// against a model written from the ABI's words alone: the plain arguments (NULL pointers against their counts, the light count at and
// past 1024, the occluder counts at and past 4096) and the synchronous call's verdict on its records — lights before boxes, the first
// invalid record of each at every position, NaNs among them.  Built and run by tests/test_light_shadow_abi.py, with the sanitizers
// where the compiler has them.  Exit status 0 = every case passed.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../raytrace_amd/csrc/api/light_shadows_check.hpp"

namespace {

int g_failures = 0;
long g_cases = 0;
#define CHECK(cond, ...)                                                            \
    do {                                                                            \
        if (!(cond)) {                                                              \
            if (g_failures++ < 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } \
        }                                                                           \
    } while (0)

// "NULL u; a NULL lights with count > 0; count > 1024; a NULL array with its count above 0; a count above 4096"
bool model_args_ok(const void* u, const void* lights, uint32_t count, const void* boxes, uint32_t nboxes, const void* models, uint32_t nmodels) {
    if (!u) return false;
    if (count > 1024 || (count > 0 && !lights)) return false;
    if (nboxes > 4096 || nmodels > 4096) return false;
    return !((nboxes > 0 && !boxes) || (nmodels > 0 && !models));
}

RtPointLight good_light() {
    RtPointLight l{};
    l.position[0] = 1.5f; l.position[1] = -128.0f; l.position[2] = 100.0f; l.radius = 8.0f;
    l.color[0] = 16.0f; l.color[1] = 8.0f; l.color[2] = 0.0f;
    return l;
}

RtDrawBox good_box() {
    RtDrawBox b{};
    b.lo[0] = 1.5f; b.lo[1] = -128.0f; b.lo[2] = 100.0f;
    b.hi[0] = 2.5f; b.hi[1] = -127.0f; b.hi[2] = 101.75f;
    return b;
}

}  // namespace

int main() {
    static_assert(rta::kMaxPointLights == 1024 && rta::kMaxEntityBoxes == 4096 && rta::kMaxEntityModels == 4096, "records per call");
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();

    // ---- the plain arguments ----
    const int something = 0;
    const std::vector<uint32_t> light_counts = {0u, 1u, 64u, 1023u, 1024u, 1025u, 4096u, 0xFFFFFFFFu};
    const std::vector<uint32_t> counts = {0u, 1u, 65u, 4095u, 4096u, 4097u, 0xFFFFFFFFu};
    long ok = 0, bad = 0;
    for (const void* u : {(const void*)&something, (const void*)nullptr})
        for (const void* lights : {(const void*)&something, (const void*)nullptr})
            for (const void* boxes : {(const void*)&something, (const void*)nullptr})
                for (const void* models : {(const void*)&something, (const void*)nullptr})
                    for (uint32_t n : light_counts)
                        for (uint32_t nb : counts)
                            for (uint32_t nm : counts) {
                                const bool want = model_args_ok(u, lights, n, boxes, nb, models, nm);
                                const char* got = rta::light_shadow_args_error(u, lights, n, boxes, nb, models, nm);
                                (want ? ok : bad)++;
                                g_cases++;
                                CHECK((got == nullptr) == want, "u %d lights %d x %u boxes %d x %u models %d x %u: model says %d, header says %s", u != nullptr,
                                      lights != nullptr, n, boxes != nullptr, nb, models != nullptr, nm, (int)want, got ? got : "fine");
                            }
    CHECK(ok > 100 && bad > 100, "both verdicts occur: %ld fine, %ld refused", ok, bad);
    CHECK(rta::light_shadow_args_error(&something, nullptr, 0, nullptr, 0, nullptr, 0) == nullptr, "an empty call needs no arrays");
    CHECK(rta::light_shadow_args_error(&something, &something, 1, nullptr, 0, nullptr, 0) == nullptr, "no occluders need no arrays");

    // ---- the records of the synchronous call: lights first, then boxes; the first invalid one of each at every position ----
    for (uint32_t n : {0u, 1u, 2u, 64u, 65u, 1024u})
        for (uint32_t nb : {0u, 1u, 63u, 65u, 4096u}) {
            const std::vector<RtPointLight> lights(n, good_light());
            const std::vector<RtDrawBox> boxes(nb, good_box());
            uint32_t at = 77u;
            CHECK(rta::light_shadow_first_invalid(lights.data(), n, boxes.data(), nb, &at) == 0, "%u valid lights, %u valid boxes", n, nb);
            g_cases++;
            for (uint32_t i = 0; i < n; i += (n > 70u ? 341u : 1u)) {
                std::vector<RtPointLight> l = lights;
                l[i].radius = (i & 1u) ? nan : 0.0f;
                if (i + 1u < n) l[n - 1u].reserved = 1u;
                std::vector<RtDrawBox> b = boxes;
                if (nb) b[0].lo[0] = inf;   // an invalid box does not hide the invalid light in front of it
                CHECK(rta::light_shadow_first_invalid(l.data(), n, b.data(), nb, &at) == 1 && at == i, "%u lights, first invalid at %u: said %u", n, i, at);
                g_cases++;
            }
            for (uint32_t i = 0; i < nb; i += (nb > 70u ? 389u : 1u)) {
                std::vector<RtDrawBox> b = boxes;
                b[i].hi[1] = (i & 1u) ? nan : b[i].lo[1];
                if (i + 1u < nb) b[nb - 1u].lo[2] = nan;
                CHECK(rta::light_shadow_first_invalid(lights.data(), n, b.data(), nb, &at) == 2 && at == i, "%u boxes, first invalid at %u: said %u", nb, i, at);
                g_cases++;
            }
        }
    {
        uint32_t at = 5u;
        CHECK(rta::light_shadow_first_invalid(nullptr, 0, nullptr, 0, &at) == 0, "empty batches read nothing");
    }

    if (g_failures) { fprintf(stderr, "%d failures in %ld cases\n", g_failures, g_cases); return 1; }
    printf("all cases match the model (%ld cases)\n", g_cases);
    return 0;
}
