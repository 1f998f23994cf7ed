// edit_shapes.hpp — the host half of rt_edit_shapes: validate a batch of shapes, clip each one's bounding box to the region, mark the
// 64^3 chunks the boxes meet and list the boxes that wait for the next frame.  Plain C++ with no HIP include, so that
// tests/edit_shapes_main.cpp runs this very code on the CPU.  Everything is integer arithmetic (include/rt_abi.h, RtShapeEdit).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../../include/rt_abi.h"
#include "edit_binning.hpp"

namespace rta __attribute__((visibility("hidden"))) {

constexpr uint32_t kMaxShapes = 4096;          // shapes per call
constexpr int32_t kMaxSphereBudget = 1 << 26;  // RtShapeEdit.b[0] of a sphere: (2 r)^2, so r <= 4096

// floor(sqrt(v)) for 0 <= v <= 2^26, bit by bit (the device's rule, rt_edit.hip)
inline int32_t shape_isqrt(int32_t v) {
    int32_t s = 0;
    for (int32_t bit = 1 << 13; bit; bit >>= 1) {
        const int32_t t = s | bit;
        if (t * t <= v) s = t;
    }
    return s;
}

// One shape of a region of edge R: kind, where and reserved in range, coordinates within [-4R, 4R], a box with a <= b, a sphere
// with b[0] in [0, 2^26] and b[1] = b[2] = 0.
inline bool shape_valid(const RtShapeEdit& s, int32_t R) {
    if (s.kind > RT_SHAPE_SPHERE || s.where > RT_WHERE_AIR || s.reserved != 0u) return false;
    for (int k = 0; k < 3; k++)
        if (s.a[k] < -4 * R || s.a[k] > 4 * R) return false;
    if (s.kind == RT_SHAPE_BOX) {
        for (int k = 0; k < 3; k++)
            if (s.b[k] < -4 * R || s.b[k] > 4 * R || s.a[k] > s.b[k]) return false;
        return true;
    }
    return s.b[0] >= 0 && s.b[0] <= kMaxSphereBudget && s.b[1] == 0 && s.b[2] == 0;
}

// `count`, or the index of the first shape that is not valid.
inline uint32_t shapes_validate(const RtShapeEdit* shapes, uint32_t count, int logr) {
    const int32_t R = 1 << logr;
    for (uint32_t i = 0; i < count; i++)
        if (!shape_valid(shapes[i], R)) return i;
    return count;
}

// The bounding box of a valid shape: per axis the texels of [0, R) that pass that axis's own test — a box's range, a sphere's
// (2 x + 1 - a)^2 <= b[0], i.e. a - s <= 2 x + 1 <= a + s with s = floor(sqrt(b[0])).  False when an axis has none (`out` is then
// untouched).
inline bool shape_bounding_box(const RtShapeEdit& s, int logr, EditBox* out) {
    const int32_t R = 1 << logr;
    int32_t lo[3], hi[3];
    const int32_t r = s.kind == RT_SHAPE_SPHERE ? shape_isqrt(s.b[0]) : 0;
    for (int k = 0; k < 3; k++) {
        if (s.kind == RT_SHAPE_BOX) { lo[k] = s.a[k]; hi[k] = s.b[k]; }
        else { lo[k] = (s.a[k] - r) >> 1; hi[k] = (s.a[k] + r - 1) >> 1; }   // ceil((a - r - 1) / 2), floor((a + r - 1) / 2)
        if (lo[k] < 0) lo[k] = 0;
        if (hi[k] > R - 1) hi[k] = R - 1;
        if (lo[k] > hi[k]) return false;
    }
    for (int k = 0; k < 3; k++) { out->lo[k] = (uint16_t)lo[k]; out->hi[k] = (uint16_t)hi[k]; }
    return true;
}

// scratch kept between calls (the context owns one): a mark per chunk
struct ShapeScratch { std::vector<uint8_t> mark; };

// what shapes_touched found, and the layout of the staging block: touched chunk ids at 0, the shape records (32 bytes each, as
// the caller gave them) at off_shapes; `need` bytes in all
struct ShapePlan {
    uint32_t touched = 0;   // chunks that meet the bounding box of at least one shape
    uint32_t boxes = 0;     // shapes with a bounding box
    size_t off_shapes = 0, need = 0;
};

// Marks every chunk that meets a bounding box of the (valid) batch.
inline ShapePlan shapes_touched(ShapeScratch& sc, const RtShapeEdit* shapes, uint32_t count, int logr) {
    const int nl = logr - 6;
    const uint32_t nchunks = 1u << (3 * nl);
    sc.mark.assign(nchunks, 0u);
    ShapePlan p;
    for (uint32_t i = 0; i < count; i++) {
        EditBox b;
        if (!shape_bounding_box(shapes[i], logr, &b)) continue;
        p.boxes++;
        for (uint32_t cz = b.lo[2] >> 6; cz <= (uint32_t)(b.hi[2] >> 6); cz++)
            for (uint32_t cy = b.lo[1] >> 6; cy <= (uint32_t)(b.hi[1] >> 6); cy++)
                for (uint32_t cx = b.lo[0] >> 6; cx <= (uint32_t)(b.hi[0] >> 6); cx++) {
                    uint8_t& m = sc.mark[(((size_t)cz << nl | cy) << nl) | cx];
                    p.touched += m == 0u;
                    m = 1u;
                }
    }
    p.off_shapes = align16((size_t)p.touched * 4u);
    p.need = p.off_shapes + (size_t)count * sizeof(RtShapeEdit);
    return p;
}

// The chunk ids shapes_touched marked, ascending: h_chunks holds at least `touched` words; returns how many were written.
inline uint32_t shapes_fill_chunks(const ShapeScratch& sc, uint32_t* h_chunks) {
    uint32_t t = 0;
    for (size_t c = 0; c < sc.mark.size(); c++)
        if (sc.mark[c]) h_chunks[t++] = (uint32_t)c;
    return t;
}

// The boxes that wait for the next frame (RtConfig.edit_radius > 0): one per shape with a bounding box, that box, in shape order.
// out[] holds at least ShapePlan::boxes of them; returns how many were written.
inline uint32_t shape_pending_boxes(const RtShapeEdit* shapes, uint32_t count, int logr, EditBox* out) {
    uint32_t t = 0;
    for (uint32_t i = 0; i < count; i++)
        if (shape_bounding_box(shapes[i], logr, out + t)) t++;
    return t;
}

}  // namespace rta
