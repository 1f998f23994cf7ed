// emit_check.hpp — the host half of rt_emit_particles that needs no context: the verdict on one emitter, on the window and on the
// call's plain arguments, the cursor test of the synchronous call and the PLAN of a batch — per emitter with a bounding box the box
// of 4^3 bricks it covers and where that box's bricks begin among the call's items.  Plain C++ with no HIP include, so that
// tests/emit_particles_main.cpp runs this very code on the CPU.  The shape's validity and bounding box are rt_edit_shapes'
// (edit_shapes.hpp): nothing of them is restated here.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../../include/rt_abi.h"
#include "edit_shapes.hpp"

namespace rta __attribute__((visibility("hidden"))) {

constexpr uint32_t kMaxEmitters = 256;            // emitters per call
constexpr uint32_t kMaxEmitCapacity = 1u << 20;   // slots of the ring (one rt_step_particles call)
constexpr uint32_t kMaxEmitBricks = 1u << 18;     // bricks of the clipped bounding boxes of one call: a whole 256^3 region

// The emitter's shape as rt_edit_shapes reads it (where, solid, material and reserved 0).
inline RtShapeEdit emit_shape(const RtParticleEmit& e) {
    RtShapeEdit s{};
    for (int k = 0; k < 3; k++) { s.a[k] = e.a[k]; s.b[k] = e.b[k]; }
    s.kind = e.kind;
    return s;
}

// One emitter of a region of edge R.  Every comparison is false for a NaN.
inline bool emitter_valid(const RtParticleEmit& e, int32_t R) {
    if (!shape_valid(emit_shape(e), R)) return false;
    if (e.response > RT_PARTICLE_BOUNCE || e.reserved0[0] != 0u || e.reserved0[1] != 0u || e.reserved[0] != 0u || e.reserved[1] != 0u) return false;
    if (e.density < 1u || e.density > 256u) return false;
    if (!(e.half >= 0.00390625f && e.half <= 0.5f)) return false;
    if (!(e.speed >= 0.0f && e.speed <= 4096.0f && e.spread >= 0.0f && e.spread <= 4096.0f)) return false;
    for (int k = 0; k < 3; k++)
        if (!(std::fabs(e.drift[k]) <= 4096.0f && std::fabs(e.origin[k]) <= 4194304.0f)) return false;
    if (!(e.life_min > 0.0f)) return false;   // (+inf passes: for ever)
    return e.life_span >= 0.0f && e.life_span <= 4096.0f;
}

// `count`, or the index of the first emitter that is not valid.
inline uint32_t first_invalid_emitter(const RtParticleEmit* emitters, uint32_t count, int logr) {
    for (uint32_t i = 0; i < count; i++)
        if (!emitter_valid(emitters[i], (int32_t)1 << logr)) return i;
    return count;
}

// |lr_k| <= 2^22 - R: every emitted corner then lies inside rt_sweep_boxes' |lo|, |hi| <= 2^22.
inline bool emit_window_valid(const int32_t lr[3], int logr) {
    const int64_t bound = ((int64_t)1 << 22) - ((int64_t)1 << logr);
    for (int k = 0; k < 3; k++)
        if ((int64_t)lr[k] < -bound || (int64_t)lr[k] > bound) return false;
    return true;
}

// What is wrong with the arguments that are tested before the context is looked at, or nullptr.
inline const char* emit_args_error(const void* emitters, uint32_t count, const void* lr, const void* states, uint32_t capacity, uint32_t max_emit,
                                   const void* cursor) {
    if (count > kMaxEmitters) return "more than 256 emitters in one call";
    if (count == 0u) return nullptr;
    if (!emitters || !lr || !states || !cursor) return "null pointer";
    if (capacity > kMaxEmitCapacity) return "capacity above 2^20";
    if (max_emit < 1u || max_emit > capacity) return "max_emit must be 1..capacity";
    return nullptr;
}

// The synchronous call's cursor: next inside the ring, reserved 0.
inline bool emit_cursor_valid(const RtEmitCursor& c, uint32_t capacity) { return c.next < capacity && c.reserved == 0u; }

// What the device reads per emitter that has a bounding box, 128 bytes: the emitter as the caller gave it, then the box of bricks
// its clipped bounding box covers — low brick, bricks per axis — and `first`: the index of the box's first brick among the call's
// items.  An item is one (emitter, brick); a box's bricks are numbered z-major, then y, then x.
struct EmitRecord {
    RtParticleEmit e;
    uint32_t blo[3], nbx;
    uint32_t nby, nbz, first, reserved;
};
static_assert(sizeof(EmitRecord) == 128, "the kernels read eight 16-byte words per record");

struct EmitPlan {
    std::vector<EmitRecord> recs;   // in emitter order
    uint64_t items = 0;             // bricks in all (the caller refuses more than kMaxEmitBricks)
};

// The plan of a (valid) batch.
inline EmitPlan emit_plan(const RtParticleEmit* emitters, uint32_t count, int logr) {
    EmitPlan p;
    for (uint32_t i = 0; i < count; i++) {
        EditBox b;
        if (!shape_bounding_box(emit_shape(emitters[i]), logr, &b)) continue;
        EmitRecord r{};
        r.e = emitters[i];
        uint32_t n[3];
        for (int k = 0; k < 3; k++) { r.blo[k] = (uint32_t)b.lo[k] >> 2; n[k] = ((uint32_t)b.hi[k] >> 2) - r.blo[k] + 1u; }
        r.nbx = n[0]; r.nby = n[1]; r.nbz = n[2];
        r.first = (uint32_t)(p.items > UINT32_MAX ? UINT32_MAX : p.items);
        p.items += (uint64_t)n[0] * n[1] * n[2];
        p.recs.push_back(r);
    }
    return p;
}

// Where the synchronous call's `n` particles, emitted in order from slot `next`, lie in the ring: at most two contiguous runs
// (slot, first particle, length).  Returns how many runs.
struct EmitRun { uint32_t slot, first, count; };
inline uint32_t emit_ring_runs(uint32_t next, uint32_t n, uint32_t capacity, EmitRun runs[2]) {
    if (n == 0u) return 0u;
    const uint32_t head = capacity - next < n ? capacity - next : n;
    runs[0] = EmitRun{next, 0u, head};
    if (head == n) return 1u;
    runs[1] = EmitRun{0u, head, n - head};
    return 2u;
}

}  // namespace rta
