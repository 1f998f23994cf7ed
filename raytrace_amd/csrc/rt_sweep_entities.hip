// rt_sweep_entities.hip — gfx950 kernel of rt_sweep_entities / rt_sweep_entities_async: a box swept through the resident region AND
// the entities a host draws — RtDrawBox boxes and RtDrawStamp voxel models — so that what is drawn is also solid
// (include/rt_abi.h "Entity sweeps"; restated, without a cull and cell by cell, in tests/sweep_entities_ref.py).
//
//   k_sweep_entities : 256 threads, one lane per sweep, no LDS, no atomics; the plan of k_entity_query.
//     Phase 1: the lane sweeps the world with sweep_box (rt_sweep_box.hpp, the one definition k_sweep calls) and stores the
//              RtSweepHit where the caller wants it: W.
//     Phase 2: a lane whose record lies outside the domain can report nothing and is done.  Every other lane's hull — its box and
//              the box displaced by the motion, grown by a margin — bounds every obstacle that can embed or block it; the wave
//              reduces the hulls of its live lanes.  Per batch of 64 records lane l loads record base + l — the boxes first, then the
//              models' 64-byte DrawStampRecords — and tests the record's box against the wave's bounds; per keeper the record's
//              words are broadcast and each live lane runs the exact obstacle rule: once for a box, once per SOLID cell of the part
//              of a model its own hull reaches.
//     Phase 3: a lane that reports a block finds the cell ranges of the world sweep at its horizon t_e (the trailing and leading
//              planes crossed before t_e: no voxel is fetched, W found them free) and clamps the returned box with them.
//
// The cull may only drop a record for which the exact rule reports nothing for every live lane of the wave, and the cell ranges of
// a model only cells for which it reports nothing for this lane (DESIGN.md "Entity sweeps" carries the argument for the margin).
// The cells of a model are visited in ascending (z, y, x) order, which is the contract's tie order; what depends on one axis only —
// the planes, the overlap at the start, the two times — is computed in that axis' loop.
#include <hip/hip_runtime.h>

#include "rt_sweep_box.hpp"
#include "rt_tile_pass.hpp"

namespace rtd {

namespace {

constexpr uint32_t kSweepEntitiesWg = 256;
// the hull's margin per axis: 2^-20 of |lo| + |hi| + |motion| (the rule's own error against real arithmetic is below 2^-22 of
// them), and 1e-30 absolute where the product went denormal
constexpr float kHullRel = 1.0f / 1048576.0f;
constexpr float kHullAbs = 1.0e-30f;
constexpr int kHorizonMaxPlanes = 128;   // above the 73 planes a face crosses before t = 1 (|motion| <= 64, extent <= 8)

// What one axis of one obstacle [olo, ohi] means to the sweep (rt_abi.h "One obstacle box").
struct AxisTerm {
    bool start;     // overlaps at the start: lo < ohi && olo < hi
    float te, tx;   // a moving axis: when the leading face meets the obstacle's near face, when the trailing face leaves its far face
};
__device__ __forceinline__ AxisTerm axis_term(float olo, float ohi, float lo, float hi, float m) {
    AxisTerm a;
    a.start = lo < ohi && olo < hi;
    const float near = m > 0.0f ? olo - hi : ohi - lo, far = m > 0.0f ? ohi - lo : olo - hi;
    a.te = near / m;
    a.tx = far / m;
    return a;
}

// The obstacle rule from its three axis terms: 0 = nothing, 1 = blocks at *t on *axis, 2 = embeds.
__device__ __forceinline__ int obstacle_rule(const AxisTerm& x, const AxisTerm& y, const AxisTerm& z, const float (&m)[3], float* t, uint32_t* axis) {
    if (x.start && y.start && z.start) return 2;
    const bool mx = m[0] != 0.0f, my = m[1] != 0.0f, mz = m[2] != 0.0f;
    if ((!mx && !x.start) || (!my && !y.start) || (!mz && !z.start)) return 0;
    // the moving axis with the largest te, the highest axis on equal values
    bool any = false;
    float te = 0.0f;
    uint32_t a = 3u;
    if (mx) { te = x.te; a = 0u; any = true; }
    if (my && (!any || y.te >= te)) { te = y.te; a = 1u; any = true; }
    if (mz && (!any || z.te >= te)) { te = z.te; a = 2u; any = true; }
    if (!any) return 0;
    if (!(te >= 0.0f && te < 1.0f)) return 0;
    if ((mx && !(te < x.tx)) || (my && !(te < y.tx)) || (mz && !(te < z.tx))) return 0;
    *t = te; *axis = a;
    return 1;
}

// The cells of one model axis the hull [hlo, hhi] can reach: the lowest i with plane(i + 1) >= hlo and the highest with
// plane(i) <= hhi, found from an estimate and fixed up against the planes themselves, which never decrease in i.  Empty: *i1 < *i0.
__device__ __forceinline__ void cell_range(float origin, float scale, int ext, float hlo, float hhi, int* i0, int* i1) {
    const float top = (float)(ext - 1);
    float q = rtm_floor((hlo - origin) / scale);
    int a = (int)(!(q > 0.0f) ? 0.0f : (q > top ? top : q));
    while (a > 0 && rtm_fma((float)a, scale, origin) >= hlo) a--;
    while (a < ext && rtm_fma((float)(a + 1), scale, origin) < hlo) a++;
    q = rtm_floor((hhi - origin) / scale);
    int b = (int)(!(q > 0.0f) ? 0.0f : (q > top ? top : q));
    while (b < ext - 1 && rtm_fma((float)(b + 1), scale, origin) <= hhi) b++;
    while (b >= 0 && rtm_fma((float)b, scale, origin) > hhi) b--;
    *i0 = a; *i1 = b;
}

// What a lane carries through phase 2.
struct Best {
    float t, face;                  // a block: its time and the obstacle's near face on the blocked axis
    uint32_t rec, axis, voxel, cell;   // rec: boxes 0 .., models nboxes ..; kNoRecord = nothing yet
    bool embedded;
};

template <int LOGR>
__global__ __launch_bounds__(kSweepEntitiesWg) void k_sweep_entities(Scene sc, SweepEntitiesArgs a) {
    const uint32_t i = blockIdx.x * kSweepEntitiesWg + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool mine = i < a.count;   // (a lane past the last sweep stays for the wave's broadcasts and stores nothing)

    // ---- phase 1: the world, as k_sweep sweeps it ----
    float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f}, m[3] = {0.0f, 0.0f, 0.0f};
    uint32_t skip_box = 0u, skip_model = 0u;
    SweepResult W;
    W.kind = RT_SWEEP_INVALID; W.t = 0.0f;
    if (mine) {
        const uint4 r0 = a.sweeps[3u * (size_t)i], r1 = a.sweeps[3u * (size_t)i + 1u], r2 = a.sweeps[3u * (size_t)i + 2u];
        lo[0] = __uint_as_float(r0.x); lo[1] = __uint_as_float(r0.y); lo[2] = __uint_as_float(r0.z);
        hi[0] = __uint_as_float(r1.x); hi[1] = __uint_as_float(r1.y); hi[2] = __uint_as_float(r1.z);
        m[0] = __uint_as_float(r2.x); m[1] = __uint_as_float(r2.y); m[2] = __uint_as_float(r2.z);
        skip_box = r0.w; skip_model = r1.w;
        sweep_box<LOGR>(sc.mine, a.lr, lo, hi, m, W);
        if (a.world_hits) {   // k_sweep's record
            uint32_t material = 0u, tx = 0xFFFFFFFFu, ty = 0xFFFFFFFFu, tz = 0xFFFFFFFFu;
            if (W.found) {
                constexpr int LB = LOGR - 2;
                const uint32_t vox = W.vox;
                material = sc.mat[vox];
                const uint32_t brick = vox >> 6, bm = (1u << LB) - 1u;
                tx = ((brick & bm) << 2) | (vox & 3u);
                ty = (((brick >> LB) & bm) << 2) | ((vox >> 2) & 3u);
                tz = ((brick >> (2 * LB)) << 2) | ((vox >> 4) & 3u);
            }
            uint4* out = a.world_hits + 4u * (size_t)i;
            out[0] = make_uint4(__float_as_uint(W.t), W.kind, W.normal, material);
            out[1] = make_uint4(tx, ty, tz, W.axis);
            out[2] = make_uint4(__float_as_uint(W.lo[0]), __float_as_uint(W.lo[1]), __float_as_uint(W.lo[2]), 0u);
            out[3] = make_uint4(__float_as_uint(W.hi[0]), __float_as_uint(W.hi[1]), __float_as_uint(W.hi[2]), 0u);
        }
    }

    // ---- phase 2: the lane's hull and the wave's bounds ----
    const bool live = mine && W.kind != (uint32_t)RT_SWEEP_INVALID;
    float hlo[3], hhi[3], wlo[3], whi[3];
    for (int k = 0; k < 3; k++) {
        const float mg = (rtm_abs(lo[k]) + rtm_abs(hi[k]) + rtm_abs(m[k])) * kHullRel + kHullAbs;
        hlo[k] = rtm_min(lo[k], lo[k] + m[k]) - mg;
        hhi[k] = rtm_max(hi[k], hi[k] + m[k]) + mg;
        float lo_k = live ? hlo[k] : INFINITY, hi_k = live ? hhi[k] : -INFINITY;
        for (int s = 32; s > 0; s >>= 1) {
            lo_k = fminf(lo_k, __shfl_xor(lo_k, s, 64));
            hi_k = fmaxf(hi_k, __shfl_xor(hi_k, s, 64));
        }
        wlo[k] = lo_k; whi[k] = hi_k;
    }

    Best best;
    best.t = INFINITY; best.face = 0.0f; best.rec = kNoRecord; best.axis = 3u; best.voxel = 0xFFFFFFFFu; best.cell = 0u; best.embedded = false;
    // ---- the boxes ----
    for (uint32_t base = 0; base < a.nboxes; base += 64u) {
        const uint32_t rec = base + lane;
        uint4 w0 = make_uint4(0u, 0u, 0u, 0u), w1 = w0;
        bool keep = false;
        if (rec < a.nboxes) {
            w0 = a.boxes[2u * (size_t)rec];
            w1 = a.boxes[2u * (size_t)rec + 1u];
            float olo[3], ohi[3];
            rec_xyz(w0, olo); rec_xyz(w1, ohi);
            keep = box_valid(olo, ohi);
            for (int k = 0; k < 3; k++) if (ohi[k] < wlo[k] || olo[k] > whi[k]) keep = false;
        }
        unsigned long long cand = __ballot(keep);
        while (cand) {
            const int j = __builtin_ctzll(cand);
            cand &= cand - 1ull;
            float olo[3], ohi[3];
            rec_xyz(w0, j, olo); rec_xyz(w1, j, ohi);
            const uint32_t idx = base + (uint32_t)j;
            if (!live || best.embedded || idx + 1u == skip_box) continue;
            float t;
            uint32_t axis;
            const int r = obstacle_rule(axis_term(olo[0], ohi[0], lo[0], hi[0], m[0]), axis_term(olo[1], ohi[1], lo[1], hi[1], m[1]),
                                        axis_term(olo[2], ohi[2], lo[2], hi[2], m[2]), m, &t, &axis);
            if (r == 2) { best.embedded = true; best.rec = idx; }
            else if (r == 1 && t < best.t) {
                best.t = t; best.rec = idx; best.axis = axis;
                const bool up = (axis == 0u ? m[0] : (axis == 1u ? m[1] : m[2])) > 0.0f;
                best.face = axis == 0u ? (up ? olo[0] : ohi[0]) : (axis == 1u ? (up ? olo[1] : ohi[1]) : (up ? olo[2] : ohi[2]));
            }
        }
    }
    // ---- the models ----
    for (uint32_t first = 0; first < a.nmodels; first += 64u) {
        const uint32_t rec = first + lane;
        uint4 w0 = make_uint4(0u, 0u, 0u, 0u), w1 = w0, w2 = w0, w3 = w0;
        bool keep = false;
        if (rec < a.nmodels) {
            w0 = a.recs[4u * (size_t)rec];
            w1 = a.recs[4u * (size_t)rec + 1u];
            w2 = a.recs[4u * (size_t)rec + 2u];
            w3 = a.recs[4u * (size_t)rec + 3u];
            float olo[3], ohi[3];
            rec_xyz(w2, olo); rec_xyz(w3, ohi);
            keep = true;
            for (int k = 0; k < 3; k++) if (ohi[k] < wlo[k] || olo[k] > whi[k]) keep = false;
        }
        unsigned long long cand = __ballot(keep);
        while (cand) {
            const int j = __builtin_ctzll(cand);
            cand &= cand - 1ull;
            float org[3], top[3];
            rec_xyz(w2, j, org); rec_xyz(w3, j, top);
            const ModelRec mr = model_rec(w0, w1, w2, j);
            const uint32_t idx = first + (uint32_t)j;
            if (!live || best.embedded || idx + 1u == skip_model) continue;
            // the lane's own hull against the model's box, planes 0 and E': the wave kept the record for some other lane
            if (top[0] < hlo[0] || org[0] > hhi[0] || top[1] < hlo[1] || org[1] > hhi[1] || top[2] < hlo[2] || org[2] > hhi[2]) continue;
            int c0[3], c1[3];
            for (int k = 0; k < 3; k++) cell_range(org[k], mr.scale, mr.ext[k], hlo[k], hhi[k], &c0[k], &c1[k]);
            if (c1[0] < c0[0] || c1[1] < c0[1] || c1[2] < c0[2]) continue;
            // within the model: the smallest t, then the lowest axis, then ascending (z, y, x); the first embedding cell ends it
            float mt = INFINITY, mface = 0.0f;
            uint32_t maxis = 3u, mvoxel = 0u, mcell = 0u;
            bool membedded = false;
            for (int cz = c0[2]; cz <= c1[2] && !membedded; cz++) {
                const float pz0 = rtm_fma((float)cz, mr.scale, org[2]), pz1 = rtm_fma((float)(cz + 1), mr.scale, org[2]);
                const AxisTerm tz = axis_term(pz0, pz1, lo[2], hi[2], m[2]);
                if (pz0 == pz1 || (m[2] == 0.0f && !tz.start)) continue;
                for (int cy = c0[1]; cy <= c1[1] && !membedded; cy++) {
                    const float py0 = rtm_fma((float)cy, mr.scale, org[1]), py1 = rtm_fma((float)(cy + 1), mr.scale, org[1]);
                    const AxisTerm ty = axis_term(py0, py1, lo[1], hi[1], m[1]);
                    if (py0 == py1 || (m[1] == 0.0f && !ty.start)) continue;
                    const int row = mr.base + mr.stride[1] * cy + mr.stride[2] * cz;
                    for (int cx = c0[0]; cx <= c1[0]; cx++) {
                        const int voxel = row + mr.stride[0] * cx;
                        if (mr.state[voxel] != RT_STAMP_SOLID) continue;
                        const float px0 = rtm_fma((float)cx, mr.scale, org[0]), px1 = rtm_fma((float)(cx + 1), mr.scale, org[0]);
                        if (px0 == px1) continue;
                        const AxisTerm tx = axis_term(px0, px1, lo[0], hi[0], m[0]);
                        float t;
                        uint32_t axis;
                        const int r = obstacle_rule(tx, ty, tz, m, &t, &axis);
                        if (r == 0) continue;
                        const uint32_t cell = (uint32_t)cx | ((uint32_t)cy << 8) | ((uint32_t)cz << 16);   // (0 <= c_k < 256)
                        if (r == 2) { membedded = true; mvoxel = (uint32_t)voxel; mcell = cell; break; }
                        if (t < mt || (t == mt && axis < maxis)) {
                            mt = t; maxis = axis; mvoxel = (uint32_t)voxel; mcell = cell;
                            const bool up = (axis == 0u ? m[0] : (axis == 1u ? m[1] : m[2])) > 0.0f;
                            mface = axis == 0u ? (up ? px0 : px1) : (axis == 1u ? (up ? py0 : py1) : (up ? pz0 : pz1));
                        }
                    }
                }
            }
            if (membedded) { best.embedded = true; best.rec = a.nboxes + idx; best.voxel = mvoxel; best.cell = mcell; }
            else if (maxis != 3u && mt < best.t) {
                best.t = mt; best.rec = a.nboxes + idx; best.axis = maxis; best.face = mface; best.voxel = mvoxel; best.cell = mcell;
            }
        }
    }

    if (!mine) return;
    // ---- what is reported: every byte of the record is written ----
    const bool embedded = live && best.embedded;
    const bool blocked = live && !embedded && best.rec != kNoRecord && (W.kind == (uint32_t)RT_SWEEP_FREE || W.kind == (uint32_t)RT_SWEEP_BLOCKED) &&
                         best.t < W.t;   // strict: the world wins ties
    uint4 h0 = make_uint4(__float_as_uint(live ? 1.0f : 0.0f), live ? (uint32_t)RT_SWEEP_FREE : (uint32_t)RT_SWEEP_INVALID, 6u, 0u);
    uint4 h1 = make_uint4((uint32_t)RT_ENTITY_NONE, 0xFFFFFFFFu, 3u, 0xFFFFFFFFu);
    uint4 h2 = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u);
    float rl[3] = {W.lo[0], W.lo[1], W.lo[2]}, rh[3] = {W.hi[0], W.hi[1], W.hi[2]};   // (an INVALID W returns the input bits)
    if (embedded || blocked) {
        uint32_t material;
        if (best.rec < a.nboxes) {
            material = a.boxes[2u * (size_t)best.rec].w;
            h1 = make_uint4((uint32_t)RT_ENTITY_BOX, best.rec, blocked ? best.axis : 3u, 0xFFFFFFFFu);
        } else {
            const uint32_t mi = best.rec - a.nboxes;
            const uint4 r0 = a.recs[4u * (size_t)mi];
            const uint32_t* mats = reinterpret_cast<const uint32_t*>((uint64_t)r0.x | ((uint64_t)r0.y << 32));
            material = mats[best.voxel];
            h1 = make_uint4((uint32_t)RT_ENTITY_MODEL, mi, blocked ? best.axis : 3u, best.voxel);
            h2 = make_uint4(best.cell & 0xFFu, (best.cell >> 8) & 0xFFu, (best.cell >> 16) & 0xFFu, 0u);
        }
        if (embedded) {
            h0 = make_uint4(__float_as_uint(0.0f), (uint32_t)RT_SWEEP_EMBEDDED, 6u, material);
            for (int k = 0; k < 3; k++) { rl[k] = lo[k]; rh[k] = hi[k]; }
        } else {
            // ---- phase 3: the world sweep's cell ranges at the horizon t_e, then rt_sweep_boxes' returned box at t_e ----
            const float te = best.t;
            bool up_a = false;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                rl[k] = lo[k]; rh[k] = hi[k];
                if (m[k] != 0.0f) {   // (an axis that does not move returns its input, bit for bit)
                    int clo = (int)__builtin_floorf(lo[k]), chi = (int)__builtin_ceilf(hi[k]) - 1;
                    const bool up = m[k] > 0.0f;
                    // trailing planes set the range's near end, leading planes add their layer at its far end
                    int gT = up ? clo + 1 : chi, gL = up ? chi + 1 : clo;
                    const float faceT = up ? lo[k] : hi[k], faceL = up ? hi[k] : lo[k];
                    for (int n = 0; n < kHorizonMaxPlanes && sweep_time(gT, faceT, m[k]) < te; n++) {
                        if (up) clo = gT; else chi = gT - 1;
                        gT += up ? 1 : -1;
                    }
                    for (int n = 0; n < kHorizonMaxPlanes && sweep_time(gL, faceL, m[k]) < te; n++) {
                        if (up) chi = gL; else clo = gL - 1;
                        gL += up ? 1 : -1;
                    }
                    rl[k] = clamp_lo(lo[k] + m[k] * te, clo);
                    rh[k] = clamp_hi(hi[k] + m[k] * te, chi + 1);
                    if (best.axis == (uint32_t)k) {
                        const float size = hi[k] - lo[k];
                        up_a = up;
                        if (up) {
                            rh[k] = best.face;
                            rl[k] = clamp_lo(best.face - size, clo);
                        } else {
                            rl[k] = best.face;
                            rh[k] = clamp_hi(best.face + size, chi + 1);
                        }
                    }
                }
            }
            h0 = make_uint4(__float_as_uint(te), (uint32_t)RT_SWEEP_BLOCKED, 2u * best.axis + (up_a ? 1u : 0u), material);
        }
    }
    uint4* out = a.entity_hits + 5u * (size_t)i;
    out[0] = h0; out[1] = h1; out[2] = h2;
    out[3] = make_uint4(__float_as_uint(rl[0]), __float_as_uint(rl[1]), __float_as_uint(rl[2]), 0u);
    out[4] = make_uint4(__float_as_uint(rh[0]), __float_as_uint(rh[1]), __float_as_uint(rh[2]), 0u);
}

}  // namespace

hipError_t launch_sweep_entities(const Scene& sc, int logr, const SweepEntitiesArgs& a, hipStream_t st) {
    if (logr < 8 || logr > 10) return hipErrorInvalidValue;
    if (a.count == 0u) return hipSuccess;
    const dim3 grid((a.count + kSweepEntitiesWg - 1u) / kSweepEntitiesWg), block(kSweepEntitiesWg);
    if (logr == 8) hipLaunchKernelGGL((k_sweep_entities<8>), grid, block, 0, st, sc, a);
    else if (logr == 9) hipLaunchKernelGGL((k_sweep_entities<9>), grid, block, 0, st, sc, a);
    else hipLaunchKernelGGL((k_sweep_entities<10>), grid, block, 0, st, sc, a);
    return hipGetLastError();
}

}  // namespace rtd
