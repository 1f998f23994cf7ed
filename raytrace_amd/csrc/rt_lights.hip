// rt_lights.hip — gfx950 kernels of rt_add_lights / rt_add_lights_async: point lights added to the two lighting planes of the frame
// drawn last, each through one hard shadow ray per (pixel, light) (include/rt_abi.h "Point lights"; the rules are restated, without a
// cull, in tests/point_light_ref.py) — and of rt_add_lights_occluded / rt_add_lights_occluded_async, the same with the drawn entities
// as occluders (k_add_lights_occluded, further down, with a head of its own).
//
//   k_add_lights : a tile pass (rt_tile_pass.hpp).  A lane rebuilds the surface point P' of its pixel from the depth and normal planes
//                  (surface_point); a tile without a surface pixel ends.  The wave reduces the per-axis bounds of its lanes' P'
//                  (tile_point_bounds).  Per batch of 64 lights lane l loads light base + l (two 16-byte loads), tests its validity and
//                  its sphere against the tile's bounds (light_may_reach_tile); for each candidate every lane runs the exact test with
//                  scalar light operands.  Lanes that pass step the shadow ray with the shared DDA of rt_dda.hpp (DIRECT: minefield
//                  bytes straight from the swizzled array, as k_query) and test between two steps whether the ray has reached the
//                  light.  No LDS, no atomics.
//
// What the two kernels do with one (pixel, light) pair — the exact test, the world's shadow ray, the weight, the add to the two
// lighting planes — exists once, as file-local helpers; the kernels stay two, k_add_lights at its own register count.
//
// All arithmetic that decides a pixel is fp32 with one rounding per operation (-ffp-contract=off).  The cull drops a light only where
// the exact test skips it at every pixel of the tile; it needs no margin (DESIGN.md "Point lights"): it repeats the exact test's own
// operations on operands that are no larger in magnitude, and every one of those operations is monotone.
#include <hip/hip_runtime.h>

#include "rt_dda.hpp"
#include "rt_tile_pass.hpp"

namespace rtd {

namespace {

constexpr float kLightMaxRadius = 1024.0f;
constexpr float kLightMaxColor = 1048576.0f;   // 2^20

// The contract's valid light (every comparison is false for a NaN).
__device__ __forceinline__ bool light_valid(uint4 w0, uint4 w1) {
    float p[3], c[3];
    rec_xyz(w0, p); rec_xyz(w1, c);
    const float radius = __uint_as_float(w0.w);
    bool ok = radius > 0.0f && radius <= kLightMaxRadius && w1.w == 0u;
    for (int k = 0; k < 3; k++) ok = ok && rtm_abs(p[k]) <= kPassMaxCoord && c[k] >= 0.0f && c[k] <= kLightMaxColor;
    return ok;
}

// Conservative: false only when the exact test skips the light at every pixel of the tile.  [lo, hi] bounds the finite P' of the tile's
// surface pixels (a pixel whose P' is not finite has dist2 = inf or NaN and is skipped by every light).  For such a pixel
// v_k = fl(pos_k - P'_k) and, rounding being monotone, v_k >= fl(pos_k - hi_k) and -v_k >= fl(lo_k - pos_k): |v_k| >= g_k, exactly.
// dist2 = fma(v_z, v_z, fma(v_y, v_y, fl(v_x v_x))) is monotone in each |v_k| (every partial sum is >= 0), so dist2 >= gap2 when gap2
// is the same expression of g — and r2 is the exact test's own fl(radius * radius).  The comparison is false for a NaN: it keeps the
// light.
__device__ __forceinline__ bool light_may_reach_tile(const float pos[3], float radius, const float lo[3], const float hi[3]) {
    rtm_vec3 g;
    g.x = rtm_max(rtm_max(pos[0] - hi[0], lo[0] - pos[0]), 0.0f);
    g.y = rtm_max(rtm_max(pos[1] - hi[1], lo[1] - pos[1]), 0.0f);
    g.z = rtm_max(rtm_max(pos[2] - hi[2], lo[2] - pos[2]), 0.0f);
    const float gap2 = rtm_dot3(g, g), r2 = radius * radius;
    return !(gap2 >= r2);
}

// ---- one (pixel, light) pair, as both kernels below treat it -------------------------------------------------------------------------
// The exact test of a pixel (its P', whether it shows a surface, its normal's axis and sign) against a light: v from P' to the light,
// its squared length, the squared radius and c, v's component along the normal.
struct LightPair {
    float v[3], dist2, r2, c;
    bool passes;
};
__device__ __forceinline__ LightPair light_pair(const float pos[3], float radius, const float P[3], bool surface, uint32_t axis, bool even) {
    LightPair p;
    for (int k = 0; k < 3; k++) p.v[k] = pos[k] - P[k];
    p.dist2 = rtm_dot3({p.v[0], p.v[1], p.v[2]}, {p.v[0], p.v[1], p.v[2]});
    p.r2 = radius * radius;
    const float va = axis == 0u ? p.v[0] : (axis == 1u ? p.v[1] : p.v[2]);
    p.c = even ? va : -va;
    p.passes = surface && p.dist2 > 0.0f && p.dist2 < p.r2 && p.c > 0.0f;
    return p;
}

// The world's shadow ray: trace_ray from P' (first texel vox0, ok0: wrap_texel's verdict) along d, the normalised v, ended as
// visible once it is as far from P' as the light.  Does the light's contribution arrive?
template <int LOGR, bool LRZ>
__device__ __forceinline__ bool light_reaches(const Scene& sc, const Frame& f, const float P[3], vec3 d, float dist2, bool ok0, uint32_t vox0) {
    constexpr float half = (float)((1 << LOGR) / 2);
    RaySlot2 r;
    r.lx = 1.0f / rtm_abs(d.x); r.ly = 1.0f / rtm_abs(d.y); r.lz = 1.0f / rtm_abs(d.z);
    unsigned long long unused = 0;
    dda_arm<LOGR, LRZ, false, true, false>(r, d.x, d.y, d.z, P[0], P[1], P[2], ok0, vox0, 0u, f, half, nullptr, sc, unused, nullptr);
    bool reached = false;
    while (r.tracing) {
        const float ex = r.px - P[0], ey = r.py - P[1], ez = r.pz - P[2];
        if (rtm_dot3({ex, ey, ez}, {ex, ey, ez}) >= dist2) { reached = true; break; }
        dda_advance<LOGR, LRZ, false, false, false>(r, (uint32_t)sc.mine[r.vox], f, half, unused, nullptr);
    }
    return reached || r2_kind(r) == PX_AIR;
}

// The weight of a pair whose light arrives (len = sqrt(dist2)): the cosine at the surface times the squared falloff to the radius.
__device__ __forceinline__ float light_weight(const LightPair& p, float len) {
    const float cosine = p.c / len;
    const float x = 1.0f - p.dist2 / p.r2;
    return (cosine * (x * x)) / (1.0f + p.dist2);
}

// A pixel's summed light goes into its two lighting planes.
__device__ __forceinline__ void add_to_lighting(const Planes& pl, size_t pix, const float add[3]) {
    const float s[3] = {add[0] / 16.0f, add[1] / 16.0f, add[2] / 16.0f};
    float4* lf = reinterpret_cast<float4*>(pl.lighting_f32) + pix;
    float4 lv = *lf;
    lv.x += s[0]; lv.y += s[1]; lv.z += s[2];
    *lf = lv;
    ushort4* lq = reinterpret_cast<ushort4*>(pl.lighting_rgba16) + pix;
    ushort4 q = *lq;
    q.x = (uint16_t)rtm_unorm((float)q.x / 65535.0f + s[0], 65535.0f);
    q.y = (uint16_t)rtm_unorm((float)q.y / 65535.0f + s[1], 65535.0f);
    q.z = (uint16_t)rtm_unorm((float)q.z / 65535.0f + s[2], 65535.0f);
    *lq = q;
}

template <int LOGR, bool LRZ>
__global__ __launch_bounds__(kTileWg) void k_add_lights(Scene sc, Frame f, Planes pl, LightsArgs a) {
    constexpr int R = 1 << LOGR, LB = LOGR - 2;
    const TileLane tl(f.width, f.height);
    if (!tl.live) return;

    const uint32_t normal = tl.inside ? (uint32_t)pl.normal_r8[tl.pix] : 255u;
    const float depth = tl.inside ? pl.depth_f32[tl.pix] : 65535.0f;
    const bool surface = normal < 6u && depth < 65535.0f;   // (false for a NaN depth)
    if (__ballot(surface) == 0ull) return;

    // ---- the surface point P' of this lane's pixel and the tile's bounds of it, the same in every lane ----
    float P[3], lo[3], hi[3];
    surface_point(f, tl.px, tl.py, depth, normal, P);
    tile_point_bounds(surface, P, lo, hi);
    const uint32_t axis = (normal >> 1) & 3u;
    const bool even = (normal & 1u) == 0u;

    // the first texel of every shadow ray of this pixel (trace_ray's fetch at its origin)
    int ix, iy, iz;
    const bool ok0 = wrap_texel(v3(P[0], P[1], P[2]), (float)R, &ix, &iy, &iz);
    const uint32_t vox0 = swizzled_index(ix, iy, iz, LB);

    float add[3] = {0.0f, 0.0f, 0.0f};
    bool lit = false;
    for (uint32_t base = 0; base < a.count; base += 64u) {
        const uint32_t mine = base + tl.lane;
        uint4 w0 = make_uint4(0u, 0u, 0u, 0u), w1 = w0;
        bool keep = false;
        if (mine < a.count) {
            w0 = a.lights[2u * (size_t)mine];
            w1 = a.lights[2u * (size_t)mine + 1u];
            float pos[3];
            rec_xyz(w0, pos);
            keep = light_valid(w0, w1) && light_may_reach_tile(pos, __uint_as_float(w0.w), lo, hi);
        }
        unsigned long long cand = __ballot(keep);
        while (cand) {
            const int j = __builtin_ctzll(cand);
            cand &= cand - 1ull;
            float pos[3], col[3];
            rec_xyz(w0, j, pos); rec_xyz(w1, j, col);
            const float radius = __uint_as_float(bcast(w0.w, j));
            const LightPair p = light_pair(pos, radius, P, surface, axis, even);
            if (!p.passes) continue;
            if (!light_reaches<LOGR, LRZ>(sc, f, P, vnormalize(v3(p.v[0], p.v[1], p.v[2])), p.dist2, ok0, vox0)) continue;
            const float w = light_weight(p, rtm_sqrt(p.dist2));
            for (int k = 0; k < 3; k++) add[k] = add[k] + col[k] * w;
            lit = true;
        }
    }

    if (lit) add_to_lighting(pl, tl.pix, add);
}

// ---- rt_add_lights_occluded: the same pass with the drawn entities between the surface and the light --------------------------------
// (include/rt_abi.h "Point-light shadows of entities"; restated without a cull in tests/light_shadow_ref.py)
//
//   k_add_lights_occluded : k_add_lights with one more verdict per (pixel, light) pair that passed the pair test — does a box or a
//                           model block the segment from P' to the light.  Lights cross occluders per tile, so the occluders are
//                           culled once per tile and not once per (tile, light):
//                             1. a cull-only sweep over the lights, 64 at a time, finds the tile's candidate lights and the hull of the
//                                tile's P' bounds and those lights' positions: every segment of the tile lies in it;
//                             2. boxes and model bounding boxes are tested, 64 at a time, against the hull (occluder_may_touch_hull);
//                                the survivors' indices are compacted into a wave-private list in LDS (the only use of LDS: lane l
//                                then reads entry l) and their records loaded once, lane l record list[l].  More than 64 survivors of
//                                a kind: the tile scans every record per candidate light instead (`overflow`);
//                             3. k_add_lights' light loop, per candidate;
//                             4. per pair that passed, the listed occluders with scalar record operands (slab_core, the model walk);
//                                the world's ray only for the pairs no entity blocks.
//                           No barrier (the list is its wave's alone), no atomics, no scratch.

constexpr uint32_t kListCap = 64;   // listed occluders of a kind per tile: what one lane each can hold

__device__ __forceinline__ float wave_min(float v) {   // (fminf drops a NaN)
    for (int s = 32; s > 0; s >>= 1) v = fminf(v, __shfl_xor(v, s, 64));
    return v;
}

// how many set bits of `mask` lie below this lane's
__device__ __forceinline__ uint32_t bits_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Conservative: false only when the exact test fails for every (pixel, light) pair of the tile whose P' and light position lie in
// the hull [hlo, hhi].  DESIGN.md "Point-light shadows of entities" carries the argument: with the box wholly above the hull on axis
// k by the margin, a pair with d_k == 0 fails `lo_k < o_k` exactly, one with d_k < 0 has t_out <= 0 exactly (a positive difference
// times a negative reciprocal), and one with d_k > 0 has, in real numbers, (lo_k - o_k) / d_k >= len (1 + 2^-16) — the exact test's
// rounded t_in and len lie within 2^-21 of those, so t_in >= len.  The absolute margin covers a d_k that went denormal.  A NaN makes
// both comparisons false: it keeps the occluder.
__device__ __forceinline__ bool occluder_may_touch_hull(const float lo[3], const float hi[3], const float hlo[3], const float hhi[3]) {
    for (int k = 0; k < 3; k++) {
        const float m = (hhi[k] - hlo[k]) * kCullRel + kCullAbs;
        if (lo[k] > hhi[k] + m || hi[k] < hlo[k] - m) return false;
    }
    return true;
}

// What a lane carries of its pair's segment: o = P', the normalised direction, its reciprocals and the segment's length.
struct Segment {
    float o[3], d[3], inv[3], len;
    bool nonzero[3];
};

// Does one of the boxes whose records the lanes of `cand` hold (w0, w1) block this lane's segment?  Every lane must call it; `open`
// says whether this lane's pair is still unblocked.  Returns the new `open`.
__device__ __forceinline__ bool boxes_leave_open(uint4 w0, uint4 w1, unsigned long long cand, const Segment& sg, bool open) {
    while (cand && __ballot(open) != 0ull) {
        const int j = __builtin_ctzll(cand);
        cand &= cand - 1ull;
        float lo[3], hi[3];
        rec_xyz(w0, j, lo); rec_xyz(w1, j, hi);
        float t_in, t_out;
        uint32_t axis;
        const bool crosses = slab_core(lo, hi, sg.o, sg.nonzero, sg.inv, &t_in, &t_out, &axis);
        if (crosses && t_out > 0.0f && t_in < t_out && t_in < sg.len) open = false;
    }
    return open;
}

// The same for the models whose records (w0..w3) the lanes of `cand` hold: the bounding box by the box rule, then the walk of the
// model's cells: walk_model<true, false> (rt_model_walk.hpp) with the stop at the light, kept as a loop of this file because the
// kernel built on the shared one measured slower than it was, twice (DESIGN.md "One model walk").  The arithmetic is that header's,
// and a change to it there is made here too.
__device__ __forceinline__ bool models_leave_open(uint4 w0, uint4 w1, uint4 w2, uint4 w3, unsigned long long cand, const Segment& sg, bool open) {
    while (cand && __ballot(open) != 0ull) {
        const int j = __builtin_ctzll(cand);
        cand &= cand - 1ull;
        float lo[3], hi[3];
        rec_xyz(w2, j, lo); rec_xyz(w3, j, hi);
        const ModelRec m = model_rec(w0, w1, w2, j);
        float t_in, t_out;
        uint32_t axis;
        const bool crosses = slab_core(lo, hi, sg.o, sg.nonzero, sg.inv, &t_in, &t_out, &axis);
        if (open && crosses && t_out > 0.0f && t_in < t_out && t_in < sg.len) {
            const float scale = m.scale;
            // the first cell: entered from outside (t_in > 0) or started inside; clamped as a float, so every index lies in the model
            const bool outside = t_in > 0.0f;
            int c[3];
            for (int k = 0; k < 3; k++) {
                const float p = (!outside || sg.d[k] == 0.0f) ? sg.o[k] : rtm_fma(sg.d[k], t_in, sg.o[k]);
                const float q = rtm_floor((p - lo[k]) / scale), qmax = (float)(m.ext[k] - 1);
                const int ck = (int)(!(q > 0.0f) ? 0.0f : (q > qmax ? qmax : q));
                c[k] = (outside && (uint32_t)k == axis) ? (sg.d[k] > 0.0f ? 0 : m.ext[k] - 1) : ck;
            }
            int cx = c[0], cy = c[1], cz = c[2];
            const int ex = m.ext[0], ey = m.ext[1], ez = m.ext[2], stx = m.stride[0], sty = m.stride[1], stz = m.stride[2];
            const bool px = sg.d[0] > 0.0f, py = sg.d[1] > 0.0f, pz = sg.d[2] > 0.0f;
            const bool gx = sg.nonzero[0], gy = sg.nonzero[1], gz = sg.nonzero[2];
            const float ox = sg.o[0], oy = sg.o[1], oz = sg.o[2], ivx = sg.inv[0], ivy = sg.inv[1], ivz = sg.inv[2], len = sg.len;
            int voxel = m.base + stx * cx + sty * cy + stz * cz;
            bool found = false;
            for (int n = ex + ey + ez; n > 0; n--) {   // (every step moves one coordinate the ray's way: at most E'x + E'y + E'z)
                if (m.state[voxel] == RT_STAMP_SOLID) { found = true; break; }
                bool have = false;
                float tmin = 0.0f;
                uint32_t ax = 0u;
                if (gx) { tmin = (rtm_fma((float)(cx + (px ? 1 : 0)), scale, lo[0]) - ox) * ivx; have = true; }
                if (gy) {
                    const float tk = (rtm_fma((float)(cy + (py ? 1 : 0)), scale, lo[1]) - oy) * ivy;
                    if (!have || tk < tmin) { tmin = tk; ax = 1u; have = true; }
                }
                if (gz) {
                    const float tk = (rtm_fma((float)(cz + (pz ? 1 : 0)), scale, lo[2]) - oz) * ivz;
                    if (!have || tk < tmin) { tmin = tk; ax = 2u; have = true; }
                }
                if (!have || !(tmin < len)) break;   // the light lies in this cell, or before its far plane
                bool out;
                if (ax == 0u) { const int dc = px ? 1 : -1; cx += dc; voxel += dc * stx; out = cx < 0 || cx >= ex; }
                else if (ax == 1u) { const int dc = py ? 1 : -1; cy += dc; voxel += dc * sty; out = cy < 0 || cy >= ey; }
                else { const int dc = pz ? 1 : -1; cz += dc; voxel += dc * stz; out = cz < 0 || cz >= ez; }
                if (out) break;
            }
            if (found) open = false;
        }
    }
    return open;
}

template <int LOGR, bool LRZ>
__global__ __launch_bounds__(kTileWg) void k_add_lights_occluded(Scene sc, Frame f, Planes pl, LightShadowArgs a) {
    constexpr int R = 1 << LOGR, LB = LOGR - 2;
    __shared__ uint32_t s_list[kTileWg / 64u][2][kListCap];
    const TileLane tl(f.width, f.height);
    if (!tl.live) return;
    const uint32_t lane = tl.lane;

    const uint32_t normal = tl.inside ? (uint32_t)pl.normal_r8[tl.pix] : 255u;
    const float depth = tl.inside ? pl.depth_f32[tl.pix] : 65535.0f;
    const bool surface = normal < 6u && depth < 65535.0f;   // (false for a NaN depth)
    if (__ballot(surface) == 0ull) return;

    // ---- the surface point P' of this lane's pixel and the tile's bounds of it; a surface pixel whose P' is not finite switches the
    // occluders' cull off for its tile (it passes no pair test itself, but the bounds no longer speak for every lane) ----
    float P[3], lo[3], hi[3];
    surface_point(f, tl.px, tl.py, depth, normal, P);
    const bool bounded = tile_point_bounds(surface, P, lo, hi);
    const bool cull = __ballot(surface && !bounded) == 0ull;
    const uint32_t axis = (normal >> 1) & 3u;
    const bool even = (normal & 1u) == 0u;

    // ---- 1. the candidate lights of the tile and the hull of its segments ----
    float hlo[3] = {lo[0], lo[1], lo[2]}, hhi[3] = {hi[0], hi[1], hi[2]};
    bool any_light = false;
    for (uint32_t base = 0; base < a.count; base += 64u) {
        const uint32_t mine = base + lane;
        float pos[3] = {0.0f, 0.0f, 0.0f};
        bool keep = false;
        if (mine < a.count) {
            const uint4 w0 = a.lights[2u * (size_t)mine], w1 = a.lights[2u * (size_t)mine + 1u];
            rec_xyz(w0, pos);
            keep = light_valid(w0, w1) && light_may_reach_tile(pos, __uint_as_float(w0.w), lo, hi);
        }
        if (__ballot(keep) == 0ull) continue;
        any_light = true;
        for (int k = 0; k < 3; k++) {
            hlo[k] = fminf(hlo[k], wave_min(keep ? pos[k] : INFINITY));
            hhi[k] = fmaxf(hhi[k], wave_max(keep ? pos[k] : -INFINITY));
        }
    }
    if (!any_light) return;

    // ---- 2. the occluders that may touch the hull: indices compacted through the wave's list, records loaded once ----
    uint32_t* const list_b = s_list[threadIdx.x >> 6][0];
    uint32_t* const list_m = s_list[threadIdx.x >> 6][1];
    uint32_t nb = 0u, nm = 0u;
    for (uint32_t base = 0; base < a.nboxes && nb <= kListCap; base += 64u) {
        const uint32_t mine = base + lane;
        bool keep = false;
        if (mine < a.nboxes) {
            float blo[3], bhi[3];
            rec_xyz(a.boxes[2u * (size_t)mine], blo); rec_xyz(a.boxes[2u * (size_t)mine + 1u], bhi);
            keep = box_valid(blo, bhi) && (!cull || occluder_may_touch_hull(blo, bhi, hlo, hhi));
        }
        const unsigned long long mask = __ballot(keep);
        const uint32_t at = nb + bits_below(mask);
        if (keep && at < kListCap) list_b[at] = mine;
        nb += (uint32_t)__builtin_popcountll(mask);
    }
    for (uint32_t base = 0; base < a.nmodels && nb <= kListCap && nm <= kListCap; base += 64u) {
        const uint32_t mine = base + lane;
        bool keep = false;
        if (mine < a.nmodels) {
            float blo[3], bhi[3];
            rec_xyz(a.recs[4u * (size_t)mine + 2u], blo); rec_xyz(a.recs[4u * (size_t)mine + 3u], bhi);
            keep = !cull || occluder_may_touch_hull(blo, bhi, hlo, hhi);
        }
        const unsigned long long mask = __ballot(keep);
        const uint32_t at = nm + bits_below(mask);
        if (keep && at < kListCap) list_m[at] = mine;
        nm += (uint32_t)__builtin_popcountll(mask);
    }
    const bool overflow = nb > kListCap || nm > kListCap;
    // the list is read by other lanes than wrote it: the wave's LDS operations complete in order, and the fence keeps the compiler
    // from moving the reads up
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    uint4 b0 = make_uint4(0u, 0u, 0u, 0u), b1 = b0, m0 = b0, m1 = b0, m2 = b0, m3 = b0;
    unsigned long long listed_b = 0ull, listed_m = 0ull;
    if (!overflow) {
        if (lane < nb) {   // (an entry was written from an index below nboxes; the minimum makes that plain)
            const uint32_t i = min(list_b[lane], a.nboxes - 1u);
            b0 = a.boxes[2u * (size_t)i]; b1 = a.boxes[2u * (size_t)i + 1u];
        }
        if (lane < nm) {
            const uint32_t i = min(list_m[lane], a.nmodels - 1u);
            m0 = a.recs[4u * (size_t)i]; m1 = a.recs[4u * (size_t)i + 1u]; m2 = a.recs[4u * (size_t)i + 2u]; m3 = a.recs[4u * (size_t)i + 3u];
        }
        listed_b = __ballot(lane < nb);
        listed_m = __ballot(lane < nm);
    }

    // the first texel of every shadow ray of this pixel (trace_ray's fetch at its origin)
    int ix, iy, iz;
    const bool ok0 = wrap_texel(v3(P[0], P[1], P[2]), (float)R, &ix, &iy, &iz);
    const uint32_t vox0 = swizzled_index(ix, iy, iz, LB);

    // ---- 3. k_add_lights' loop ----
    float add[3] = {0.0f, 0.0f, 0.0f};
    bool lit = false;
    for (uint32_t base = 0; base < a.count; base += 64u) {
        const uint32_t mine = base + lane;
        uint4 w0 = make_uint4(0u, 0u, 0u, 0u), w1 = w0;
        bool keep = false;
        if (mine < a.count) {
            w0 = a.lights[2u * (size_t)mine];
            w1 = a.lights[2u * (size_t)mine + 1u];
            float pos[3];
            rec_xyz(w0, pos);
            keep = light_valid(w0, w1) && light_may_reach_tile(pos, __uint_as_float(w0.w), lo, hi);
        }
        unsigned long long cand = __ballot(keep);
        while (cand) {
            const int j = __builtin_ctzll(cand);
            cand &= cand - 1ull;
            float pos[3], col[3];
            rec_xyz(w0, j, pos); rec_xyz(w1, j, col);
            const float radius = __uint_as_float(bcast(w0.w, j));
            const LightPair p = light_pair(pos, radius, P, surface, axis, even);
            bool open = p.passes;
            if (__ballot(open) == 0ull) continue;
            const vec3 d = vnormalize(v3(p.v[0], p.v[1], p.v[2]));
            const float len = rtm_sqrt(p.dist2);

            // ---- 4. the entities between P' and the light (every lane walks through here: the records are broadcast) ----
            Segment sg;
            sg.o[0] = P[0]; sg.o[1] = P[1]; sg.o[2] = P[2];
            sg.d[0] = d.x; sg.d[1] = d.y; sg.d[2] = d.z;
            for (int k = 0; k < 3; k++) { sg.inv[k] = 1.0f / sg.d[k]; sg.nonzero[k] = sg.d[k] != 0.0f; }
            sg.len = len;
            if (!overflow) {
                open = boxes_leave_open(b0, b1, listed_b, sg, open);
                open = models_leave_open(m0, m1, m2, m3, listed_m, sg, open);
            } else {
                for (uint32_t first = 0; first < a.nboxes && __ballot(open) != 0ull; first += 64u) {
                    const uint32_t at = first + lane;
                    uint4 x0 = make_uint4(0u, 0u, 0u, 0u), x1 = x0;
                    bool take = false;
                    if (at < a.nboxes) {
                        x0 = a.boxes[2u * (size_t)at]; x1 = a.boxes[2u * (size_t)at + 1u];
                        float blo[3], bhi[3];
                        rec_xyz(x0, blo); rec_xyz(x1, bhi);
                        take = box_valid(blo, bhi) && (!cull || occluder_may_touch_hull(blo, bhi, hlo, hhi));
                    }
                    open = boxes_leave_open(x0, x1, __ballot(take), sg, open);
                }
                for (uint32_t first = 0; first < a.nmodels && __ballot(open) != 0ull; first += 64u) {
                    const uint32_t at = first + lane;
                    uint4 x0 = make_uint4(0u, 0u, 0u, 0u), x1 = x0, x2 = x0, x3 = x0;
                    bool take = false;
                    if (at < a.nmodels) {
                        x0 = a.recs[4u * (size_t)at]; x1 = a.recs[4u * (size_t)at + 1u]; x2 = a.recs[4u * (size_t)at + 2u]; x3 = a.recs[4u * (size_t)at + 3u];
                        float blo[3], bhi[3];
                        rec_xyz(x2, blo); rec_xyz(x3, bhi);
                        take = !cull || occluder_may_touch_hull(blo, bhi, hlo, hhi);
                    }
                    open = models_leave_open(x0, x1, x2, x3, __ballot(take), sg, open);
                }
            }
            if (open && light_reaches<LOGR, LRZ>(sc, f, P, d, p.dist2, ok0, vox0)) {   // the world's shadow ray
                const float w = light_weight(p, len);
                for (int k = 0; k < 3; k++) add[k] = add[k] + col[k] * w;
                lit = true;
            }
        }
    }

    if (lit) add_to_lighting(pl, tl.pix, add);
}

}  // namespace

hipError_t launch_add_lights_occluded(const Scene& sc, const Frame& f, const Planes& pl, const LightShadowArgs& a, hipStream_t st) {
    if (f.logr < 8 || f.logr > 10) return hipErrorInvalidValue;
    if (a.count == 0u || f.width <= 0 || f.height <= 0) return hipSuccess;
    const dim3 grid = TileLane::grid(f.width, f.height), block(kTileWg);
    launch_for_region(f, [&](auto L, auto Z) { hipLaunchKernelGGL((k_add_lights_occluded<decltype(L)::value, decltype(Z)::value>), grid, block, 0, st, sc, f, pl, a); });
    return hipGetLastError();
}

hipError_t launch_add_lights(const Scene& sc, const Frame& f, const Planes& pl, const LightsArgs& a, hipStream_t st) {
    if (f.logr < 8 || f.logr > 10) return hipErrorInvalidValue;
    if (a.count == 0u || f.width <= 0 || f.height <= 0) return hipSuccess;
    const dim3 grid = TileLane::grid(f.width, f.height), block(kTileWg);
    launch_for_region(f, [&](auto L, auto Z) { hipLaunchKernelGGL((k_add_lights<decltype(L)::value, decltype(Z)::value>), grid, block, 0, st, sc, f, pl, a); });
    return hipGetLastError();
}

}  // namespace rtd
