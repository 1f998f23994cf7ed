// draw_stamps.hpp — the host half of the voxel-model entities (rt_draw_stamps, rt_draw_stamps_async): which RtDrawStamp records are
// valid, a placed model's high corner and the 64-byte device record per model.  Plain C++ with no HIP include, so that
// tests/draw_stamps_main.cpp runs this very code on the CPU.  The store of stamps and the orientation mapping are edit_stamps.hpp's
// (include/rt_abi.h, RtDrawStamp).
#pragma once

#include <cstdint>

#include "../../../include/rt_abi.h"
#include "../../../include/rt_math.h"
#include "edit_stamps.hpp"

namespace rta __attribute__((visibility("hidden"))) {

constexpr uint32_t kMaxDrawStamps = 4096;         // models per call
constexpr float kDrawStampMaxCoord = 4194304.0f;  // 2^22
constexpr float kDrawStampMinScale = 1.0f / 256.0f, kDrawStampMaxScale = 64.0f;

// hi_k = rtm_fma(float(E'_k), scale, origin_k): plane E'_k of axis k, the bounding box's high face
inline float draw_stamp_hi(int32_t ext, float scale, float origin) { return rtm_fma((float)ext, scale, origin); }

// One record, its id resolved: `E` is the named stamp's extent.  Every comparison is false for a NaN, so a NaN fails.
inline bool draw_stamp_valid(const RtDrawStamp& m, const int32_t E[3]) {
    if (m.orient >= kStampOrients || m.reserved0[0] != 0u || m.reserved0[1] != 0u || m.reserved0[2] != 0u || m.reserved != 0u) return false;
    if (!(m.scale >= kDrawStampMinScale && m.scale <= kDrawStampMaxScale)) return false;
    const StampMap map = stamp_map(E, m.orient);
    for (int k = 0; k < 3; k++) {
        if (!(rtm_abs(m.origin[k]) <= kDrawStampMaxCoord)) return false;
        if (!(rtm_abs(draw_stamp_hi(map.ext[k], m.scale, m.origin[k])) <= kDrawStampMaxCoord)) return false;
    }
    return true;
}

// `count`, or the index of the first record that is not valid or names no live stamp.
inline uint32_t draw_stamps_validate(const StampStore& st, const RtDrawStamp* models, uint32_t count) {
    for (uint32_t i = 0; i < count; i++) {
        const StampEntry* e = st.find(models[i].stamp);
        if (!e || !draw_stamp_valid(models[i], e->ext)) return i;
    }
    return count;
}

// What the device reads per model (rt_draw_stamps.hip), 64 bytes.  Cell c (0 <= c_k < E'_k) of the placed model shows stamp voxel
// base + sum_k stride[k] * c[k].  se[k] holds stride[k] in its low 18 bits (two's complement; |stride| <= 2^16) and E'_k - 1 in the
// eight bits above them.
struct DrawStampRecord {
    uint64_t mats, state;
    int32_t base;
    uint32_t se[3];
    float origin[3], scale;
    float hi[3];
    uint32_t emission;
};
static_assert(sizeof(DrawStampRecord) == 64, "DrawStampRecord is four dword4");

inline uint32_t draw_stamp_pack(int32_t stride, int32_t ext) { return ((uint32_t)stride & 0x3FFFFu) | ((uint32_t)(ext - 1) << 18); }
inline int32_t draw_stamp_stride(uint32_t se) { return (int32_t)(se << 14) >> 14; }
inline int32_t draw_stamp_ext(uint32_t se) { return (int32_t)((se >> 18) & 0xFFu) + 1; }

// The device records of the (valid) batch, one per model in batch order.
inline void draw_stamp_fill_records(const StampStore& st, const RtDrawStamp* models, uint32_t count, DrawStampRecord* out) {
    for (uint32_t i = 0; i < count; i++) {
        const RtDrawStamp& m = models[i];
        const StampEntry* e = st.find(m.stamp);
        const StampMap map = stamp_map(e->ext, m.orient);
        DrawStampRecord r{};
        r.mats = e->mats;
        r.state = e->state;
        r.base = map.base;
        for (int k = 0; k < 3; k++) {
            r.se[k] = draw_stamp_pack(map.stride[k], map.ext[k]);
            r.origin[k] = m.origin[k];
            r.hi[k] = draw_stamp_hi(map.ext[k], m.scale, m.origin[k]);
        }
        r.scale = m.scale;
        r.emission = m.emission;
        out[i] = r;
    }
}

}  // namespace rta
