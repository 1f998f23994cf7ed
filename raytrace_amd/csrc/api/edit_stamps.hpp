// edit_stamps.hpp — the host half of the voxel stamps (rt_stamp_*, rt_edit_stamps): the store of live stamps, the orientation
// mapping, validation of a batch of placements, each one's placed extent and clipped bounding box, the marks of the 64^3 chunks the
// boxes meet, the boxes that wait for the next frame and the 64-byte device record per placement.  Plain C++ with no HIP include, so
// that tests/edit_stamps_main.cpp runs this very code on the CPU.  Everything is integer arithmetic (include/rt_abi.h, RtStampPlace).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../../include/rt_abi.h"
#include "edit_binning.hpp"
#include "edit_shapes.hpp"

namespace rta __attribute__((visibility("hidden"))) {

constexpr uint32_t kMaxStampPlaces = 4096;   // placements per call
constexpr uint32_t kMaxStamps = 1024;        // live stamps per context
constexpr int32_t kMaxStampExtent = 256;     // per axis
constexpr uint32_t kStampOrients = 48;

// ---- the store: ids are serial << 10 | slot with serial >= 1, so that an id is never 0 and a destroyed id stays unknown -------------
struct StampEntry {
    uint32_t id = 0;            // 0: the slot is free
    int32_t ext[3] = {0, 0, 0};
    uint64_t mats = 0, state = 0;   // device addresses: uint32_t[ez][ey][ex] and uint8_t[ez][ey][ex]
    bool used = false;          // a capture or placement that names it may still be running
    size_t voxels() const { return (size_t)ext[0] * (size_t)ext[1] * (size_t)ext[2]; }
};
struct StampStore {
    std::vector<StampEntry> slots;
    uint32_t live = 0, serial = 0;
    // the entry of a live id, or null
    StampEntry* find(uint32_t id) {
        const uint32_t s = id & (kMaxStamps - 1u);
        return id != 0u && s < slots.size() && slots[s].id == id ? &slots[s] : nullptr;
    }
    const StampEntry* find(uint32_t id) const { return const_cast<StampStore*>(this)->find(id); }
    // a new entry with an id of its own, or null when kMaxStamps are live
    StampEntry* add(const int32_t ext[3]) {
        if (live == kMaxStamps) return nullptr;
        uint32_t s = 0;
        while (s < slots.size() && slots[s].id != 0u) s++;
        if (s == slots.size()) slots.emplace_back();
        serial = serial >= (1u << 22) - 1u ? 1u : serial + 1u;
        StampEntry& e = slots[s];
        e = StampEntry{};
        e.id = (serial << 10) | s;
        for (int k = 0; k < 3; k++) e.ext[k] = ext[k];
        live++;
        return &e;
    }
    void remove(StampEntry* e) { *e = StampEntry{}; live--; }
};

inline bool stamp_extent_valid(const int32_t ext[3]) {
    for (int k = 0; k < 3; k++)
        if (ext[k] < 1 || ext[k] > kMaxStampExtent) return false;
    return true;
}

// ---- the orientation mapping (the kernel walks the strides this gives; the tests hold it against np.transpose / np.flip) ------------
// orient = p << 3 | f: world axis k of the placed box is stamp axis perm[k]; bit j of f flips stamp axis j.
constexpr uint8_t kStampPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

// ext = E', and index(d) = base + sum_k stride[k] * d[k] is the stamp voxel ([ez][ey][ex], x fastest) that placed-local cell d shows
struct StampMap { int32_t ext[3], stride[3], base; };
inline StampMap stamp_map(const int32_t E[3], uint32_t orient) {
    const uint8_t* perm = kStampPerm[orient >> 3];
    const uint32_t f = orient & 7u;
    const int32_t mult[3] = {1, E[0], E[0] * E[1]};
    StampMap m{};
    for (int k = 0; k < 3; k++) {
        const int a = perm[k];
        const bool flip = ((f >> a) & 1u) != 0u;
        m.ext[k] = E[a];
        m.stride[k] = flip ? -mult[a] : mult[a];
        if (flip) m.base += (E[a] - 1) * mult[a];
    }
    return m;
}
inline int32_t stamp_source_index(const StampMap& m, int32_t dx, int32_t dy, int32_t dz) {
    return m.base + m.stride[0] * dx + m.stride[1] * dy + m.stride[2] * dz;
}

// ---- a batch of placements --------------------------------------------------------------------------------------------------
// One placement in a region of edge R, its id apart: orient, where and reserved in range, at within [-4R, 4R].
inline bool place_valid(const RtStampPlace& p, int32_t R) {
    if (p.orient >= kStampOrients || p.where > RT_WHERE_AIR || p.reserved0[0] != 0u || p.reserved0[1] != 0u) return false;
    if (p.reserved[0] != 0u || p.reserved[1] != 0u || p.reserved[2] != 0u) return false;
    for (int k = 0; k < 3; k++)
        if (p.at[k] < -4 * R || p.at[k] > 4 * R) return false;
    return true;
}

// `count`, or the index of the first placement that is not valid or names no live stamp.
inline uint32_t places_validate(const StampStore& st, const RtStampPlace* places, uint32_t count, int logr) {
    const int32_t R = 1 << logr;
    for (uint32_t i = 0; i < count; i++)
        if (!place_valid(places[i], R) || !st.find(places[i].stamp)) return i;
    return count;
}

// The bounding box of a valid placement of a stamp of extent E: [at, at + E') clipped to [0, R)^3.  False when it is empty (`out` is
// then untouched).
inline bool place_bounding_box(const RtStampPlace& p, const int32_t E[3], int logr, EditBox* out) {
    const int32_t R = 1 << logr;
    const StampMap m = stamp_map(E, p.orient);
    int32_t lo[3], hi[3];
    for (int k = 0; k < 3; k++) {
        lo[k] = p.at[k] < 0 ? 0 : p.at[k];
        hi[k] = p.at[k] + m.ext[k] - 1 > R - 1 ? R - 1 : p.at[k] + m.ext[k] - 1;
        if (lo[k] > hi[k]) return false;
    }
    for (int k = 0; k < 3; k++) { out->lo[k] = (uint16_t)lo[k]; out->hi[k] = (uint16_t)hi[k]; }
    return true;
}

// what stamps_touched found, and the layout of the staging block: touched chunk ids at 0, one StampRecord per placement at
// off_recs; `need` bytes in all
struct StampPlan {
    uint32_t touched = 0;   // chunks that meet the bounding box of at least one placement
    uint32_t boxes = 0;     // placements with a bounding box
    size_t off_recs = 0, need = 0;
};

// What the device reads per placement (rt_edit.hip, StampStage), 64 bytes: the stamp's arrays, the bounding box in world texels
// (inclusive; lo > hi on every chunk's test when there is none), and the mapping folded with `at`: the stamp voxel that world texel w
// of the box shows is base + sum_k stride[k] * w[k].
struct StampRecord {
    uint64_t mats, state;
    int32_t lo[3], hi[3];
    int32_t stride[3];
    int32_t base;
    uint32_t where, reserved;
};
static_assert(sizeof(StampRecord) == 64, "StampRecord is four dword4");

// Marks every chunk that meets a bounding box of the (valid) batch; sc is rt_edit_shapes' scratch (shapes_fill_chunks lists them).
inline StampPlan stamps_touched(ShapeScratch& sc, const StampStore& st, const RtStampPlace* places, uint32_t count, int logr) {
    const int nl = logr - 6;
    sc.mark.assign((size_t)1 << (3 * nl), 0u);
    StampPlan p;
    for (uint32_t i = 0; i < count; i++) {
        EditBox b;
        if (!place_bounding_box(places[i], st.find(places[i].stamp)->ext, logr, &b)) continue;
        p.boxes++;
        for (uint32_t cz = b.lo[2] >> 6; cz <= (uint32_t)(b.hi[2] >> 6); cz++)
            for (uint32_t cy = b.lo[1] >> 6; cy <= (uint32_t)(b.hi[1] >> 6); cy++)
                for (uint32_t cx = b.lo[0] >> 6; cx <= (uint32_t)(b.hi[0] >> 6); cx++) {
                    uint8_t& m = sc.mark[(((size_t)cz << nl | cy) << nl) | cx];
                    p.touched += m == 0u;
                    m = 1u;
                }
    }
    p.off_recs = align16((size_t)p.touched * 4u);
    p.need = p.off_recs + (size_t)count * sizeof(StampRecord);
    return p;
}

// The device records of the (valid) batch, one per placement in batch order.
inline void stamp_fill_records(const StampStore& st, const RtStampPlace* places, uint32_t count, int logr, StampRecord* out) {
    const int32_t R = 1 << logr;
    for (uint32_t i = 0; i < count; i++) {
        const RtStampPlace& p = places[i];
        const StampEntry* e = st.find(p.stamp);
        const StampMap m = stamp_map(e->ext, p.orient);
        StampRecord r{};
        r.mats = e->mats;
        r.state = e->state;
        EditBox b;
        const bool has = place_bounding_box(p, e->ext, logr, &b);
        for (int k = 0; k < 3; k++) {
            r.lo[k] = has ? (int32_t)b.lo[k] : R;
            r.hi[k] = has ? (int32_t)b.hi[k] : -1;
            r.stride[k] = m.stride[k];
        }
        r.base = m.base - m.stride[0] * p.at[0] - m.stride[1] * p.at[1] - m.stride[2] * p.at[2];   // (|.| < 3 * 2^16 * 4 R <= 2^30)
        r.where = p.where;
        out[i] = r;
    }
}

// The boxes that wait for the next frame (RtConfig.edit_radius > 0): one per placement with a bounding box, that box, in batch
// order.  out[] holds at least StampPlan::boxes of them; returns how many were written.
inline uint32_t stamp_pending_boxes(const StampStore& st, const RtStampPlace* places, uint32_t count, int logr, EditBox* out) {
    uint32_t t = 0;
    for (uint32_t i = 0; i < count; i++)
        if (place_bounding_box(places[i], st.find(places[i].stamp)->ext, logr, out + t)) t++;
    return t;
}

}  // namespace rta
