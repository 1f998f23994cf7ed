// edit_binning.hpp — the host half of rt_edit_voxels: validate a batch of edits and bin it by chunk.  Plain C++ with no HIP include,
// so that tests/edit_binning_main.cpp runs this very code on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../../include/rt_abi.h"

namespace rta __attribute__((visibility("hidden"))) {

inline size_t align16(size_t n) { return (n + 15u) & ~(size_t)15u; }

// scratch kept between calls (the context owns one)
struct EditBinning {
    std::vector<uint32_t> chunk, order, start, stamp;
    uint32_t gen = 0;   // stamp generation: a voxel's slot holds the generation of the chunk run that kept it
};

// what edit_bin found: the touched chunks, and the layout of the staging block — touched chunk ids at 0, their touched + 1 record
// offsets at off_offs, the records (8 bytes each, at most one per edit) at off_recs; `need` bytes in all
struct EditBins {
    uint32_t touched = 0;
    size_t off_offs = 0, off_recs = 0, need = 0;
};

// Validates every edit, then one stable counting pass by chunk: b.order holds the edit indices grouped by chunk in batch order,
// b.start[c] the END of chunk c's range.  Returns `count`, or the index of the first edit with a coordinate outside the region or
// reserved != 0 (`out` is then untouched).
inline uint32_t edit_bin(EditBinning& b, const RtVoxelEdit* edits, uint32_t count, int logr, EditBins* out) {
    const uint32_t R = 1u << logr;
    const int nl = logr - 6;
    const uint32_t nchunks = 1u << (3 * nl);
    std::vector<uint32_t>& chunk = b.chunk;
    std::vector<uint32_t>& start = b.start;
    chunk.resize(count);
    start.assign((size_t)nchunks + 1u, 0u);
    for (uint32_t i = 0; i < count; i++) {
        const RtVoxelEdit& e = edits[i];
        if (e.x >= R || e.y >= R || e.z >= R || e.reserved != 0u) return i;
        const uint32_t c = ((uint32_t)(e.z >> 6) << (2 * nl)) | ((uint32_t)(e.y >> 6) << nl) | (uint32_t)(e.x >> 6);
        chunk[i] = c;
        start[c + 1u]++;
    }
    uint32_t touched = 0;
    for (uint32_t c = 0; c < nchunks; c++) { touched += start[c + 1u] != 0u; start[c + 1u] += start[c]; }
    std::vector<uint32_t>& order = b.order;   // edit indices grouped by chunk, batch order within a chunk
    order.resize(count);
    for (uint32_t i = 0; i < count; i++) order[start[chunk[i]]++] = i;   // afterwards start[c] = end of chunk c's range
    out->touched = touched;
    out->off_offs = align16((size_t)touched * 4u);
    out->off_recs = out->off_offs + align16(((size_t)touched + 1u) * 4u);
    out->need = out->off_recs + (size_t)count * 8u;
    return count;
}

// The texel box (min / max per axis, inclusive) of one chunk's edits.
struct EditBox { uint16_t lo[3], hi[3]; };

// One box per touched chunk of the batch edit_bin binned last, in chunk order: the texel min / max over EVERY record of the chunk
// (duplicates and records that change nothing included).  out[] holds at least `touched` boxes; returns how many were written.
inline uint32_t edit_chunk_boxes(const EditBinning& b, const RtVoxelEdit* edits, int logr, EditBox* out) {
    const uint32_t nchunks = 1u << (3 * (logr - 6));
    const std::vector<uint32_t>&start = b.start, &order = b.order;
    uint32_t t = 0;
    for (uint32_t c = 0; c < nchunks; c++) {
        const uint32_t lo = c ? start[c - 1u] : 0u, hi = start[c];
        if (lo == hi) continue;
        EditBox& x = out[t++];
        for (int k = 0; k < 3; k++) { x.lo[k] = 0xFFFFu; x.hi[k] = 0u; }
        for (uint32_t j = lo; j < hi; j++) {
            const RtVoxelEdit& ed = edits[order[j]];
            const uint16_t p[3] = {ed.x, ed.y, ed.z};
            for (int k = 0; k < 3; k++) { x.lo[k] = std::min(x.lo[k], p[k]); x.hi[k] = std::max(x.hi[k], p[k]); }
        }
    }
    return t;
}

// Staging of the batch edit_bin binned last: touched chunk ids, their edit ranges, and per chunk one record per edited voxel — its
// last edit in the batch (the range is walked backwards; b.stamp marks the voxels a chunk's run has kept).  Returns the records.
inline uint32_t edit_fill(EditBinning& b, const RtVoxelEdit* edits, int logr, uint32_t* h_chunks, uint32_t* h_offs, uint32_t* h_recs) {
    const uint32_t nchunks = 1u << (3 * (logr - 6));
    const std::vector<uint32_t>&start = b.start, &order = b.order;
    std::vector<uint32_t>& stamp = b.stamp;
    if (stamp.size() != (size_t)RT_CHUNK_SIZE * RT_CHUNK_SIZE * RT_CHUNK_SIZE) stamp.assign((size_t)RT_CHUNK_SIZE * RT_CHUNK_SIZE * RT_CHUNK_SIZE, 0u);
    uint32_t t = 0, nrec = 0;
    for (uint32_t c = 0; c < nchunks; c++) {
        const uint32_t lo = c ? start[c - 1u] : 0u, hi = start[c];
        if (lo == hi) continue;
        if (++b.gen == 0u) { std::fill(stamp.begin(), stamp.end(), 0u); b.gen = 1u; }
        const uint32_t gen = b.gen;
        h_chunks[t] = c;
        h_offs[t++] = nrec;
        for (uint32_t j = hi; j-- > lo;) {
            const RtVoxelEdit& ed = edits[order[j]];
            const uint32_t local = ((uint32_t)(ed.z & 63u) << 12) | ((uint32_t)(ed.y & 63u) << 6) | (uint32_t)(ed.x & 63u);
            if (stamp[local] == gen) continue;
            stamp[local] = gen;
            h_recs[2u * nrec] = local | (ed.solid ? 1u << 18 : 0u);
            h_recs[2u * nrec + 1u] = ed.material;
            nrec++;
        }
    }
    h_offs[t] = nrec;
    return nrec;
}

}  // namespace rta
