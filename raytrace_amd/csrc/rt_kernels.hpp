// rt_kernels.hpp — argument blocks and host-callable launchers of every kernel file (rt_*.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "rt_device.hpp"

namespace rtd {

// The launch of a kernel template over <LOGR, LRZ> for a frame's region: launch(L, Z) with decltype(L)::value = f.logr (8, 9 or 10;
// the caller has checked the range) and decltype(Z)::value = (f.lr_zero != 0).
template <typename Launch>
void launch_for_region(const Frame& f, Launch&& launch) {
    auto with = [&](auto L) {
        if (f.lr_zero != 0) launch(L, std::true_type{});
        else launch(L, std::false_type{});
    };
    if (f.logr == 8) with(std::integral_constant<int, 8>{});
    else if (f.logr == 9) with(std::integral_constant<int, 9>{});
    else with(std::integral_constant<int, 10>{});
}

// SoA ray queue + per-path hit/state arrays, all in HBM (sizes in elements; cap = paths per batch).
//   queue : origin qo*[cap] shared by the pair, directions qd*[2*cap] (shadow at slot, diffuse at cap+slot), qid[cap] = path
//   hits  : hx,hy,hz,hinfo[cap] (diffuse / primary result per path), sunres[cap] (shadow ray reached the sky)
struct TraceArgs {
    const float *qox, *qoy, *qoz, *qdx, *qdy, *qdz;
    const uint32_t* qid;
    const uint32_t* qcount;     // number of queued pairs (written by the previous shade stage)
    uint32_t* cursor;           // global ray cursor, zero before launch
    uint32_t qcap;
    uint32_t nprimary;          // MODE 0: number of paths in the batch
    uint32_t npix_pad;          // MODE 0: paths per sample (local pixels padded to whole tiles)
    uint32_t refill_threshold;  // idle lanes per wave that trigger retire + refill (1..64)
    float *hx, *hy, *hz;
    uint32_t* hinfo;            // material[20:0] | face id << 24 | limit << 30 | air << 31
    uint8_t* sunres;
    DevCounters* counters;
};

struct ShadeArgs {
    float *qox, *qoy, *qoz, *qdx, *qdy, *qdz;
    uint32_t* qid;
    uint32_t* qcount_next;      // pairs appended by this stage (zero before launch)
    uint32_t qcap;
    uint32_t npaths;            // paths in this batch
    uint32_t npaths_cap;        // allocation stride of the per-level albedo stack
    uint32_t npix_pad;
    uint32_t sample0;           // index of the batch's first sample within the frame
    const float *hx, *hy, *hz;
    const uint32_t* hinfo;
    const uint8_t* sunres;
    float *pdx, *pdy, *pdz;     // diffuse direction of the level in flight (sample_sky argument on a sky exit)
    uint8_t* pnormal;
    uint8_t* pstate;            // 1 = path still has rays in flight
    uint32_t* sunbits;          // bit j-1: shadow ray of level j reached the sky
    uint32_t* stack;            // [(depth-1)][npaths_cap] packed material of surface j+1
    float *plx, *ply, *plz;     // finished light of the path
    DevCounters* counters;
};

// k_primary / k_primary2 (rt_persist.hip): primary prepass.  Arrays are indexed by worklist slot (acc: by local pixel).
struct PrimaryArgs {
    float4* phit;               // per queued pixel, ONE 16-byte record: primary hit position (with the 0.001 face offset) and, as bits of .w,
                                // face id << 28 | gl_WorkGroupID.y * 8 << 14 | gl_WorkGroupID.x * 8 (the noise_offset terms, raytrace.comp:304)
    uint32_t* worklist;         // local pixel ids that need shadow/diffuse rays
    uint32_t* wl_count;         // zero before launch
    uint32_t* tile_cursor;      // k_primary2: next tile to hand out (a workgroup takes 16 at a time); zero before launch
    uint32_t* zero_words;       // k_primary2: words the prepass clears for later launches instead of a memset of their own: the slot's other
    uint32_t zero_count;        // worklist counter and tile cursor (the slot's next prepass) ...
    uint32_t* zero_words2;      // ... and the path cursors of the lane this frame's first path launch runs on; either may be null
    uint32_t zero_count2;
    float4* acc;                // (unused by the prepass since it stores the lighting of the pixels it finishes itself)
    DevCounters* counters;
};
// k_persist (rt_persist.hip): persistent path kernel.  Work item r = sample_in_batch * nwork + w.
// light of one path, summed per pixel in sample order by k_accumulate_paths (12 bytes: the records are the path kernels' whole
// write traffic)
struct PathLight { float x, y, z; };
struct PersistArgs {
    uint32_t* cursor;           // [8][32] next path of each XCD group's share, one word per 128-byte line (zero before launch)
    const uint32_t* worklist;   // CACHE: pixels queued by the prepass
    const uint32_t* wl_count;   // CACHE: number of queued pixels (nwork)
    uint32_t npix_pad;          // CACHE=false: nwork = all local pixels (padded to whole 8x8 tiles)
    uint32_t sample0, nsamples; // samples of this batch: sample0 .. sample0+nsamples-1
    uint32_t threshold;         // parked lanes per wave that trigger a transition pass (1..64)
    uint32_t rmin;              // (was k_seq's re-arm threshold; unused)
    uint32_t chunk;             // paths per cursor atomic; 0 = the default (128)
    uint32_t nthreads;          // grid size in threads (stride of the albedo stack)
    uint32_t direct;            // 1: the frame has ONE sample, so a path's light is its pixel's: the kernel stores the lighting planes
                                // itself (0 + light, / spp / 16: what k_accumulate_paths would do) and writes no light record
    uint32_t pl_stream;         // k_paths: 1 = the light records go out as streaming (`nt`) stores — set when a launch's records are too many
                                // to be worth keeping in L2 / the Infinity Cache until k_accumulate_paths reads them
    uint32_t* stack;            // [2][(depth-1)][nthreads] packed material of surface j+1 (only touched when depth >= 2; k_persist uses half)
    const float4* phit;         // CACHE: the primary prepass' record per worklist slot (PrimaryArgs::phit): one load per new path
    const float4* sun_lut;      // [2*65536] per-frame shadow-ray table: direction, 1/|direction|
    const float4* dif_lut;      // [4*6*65536] diffuse-ray table, one 64-byte line per (face, noise byte pair): dir, normalized dir, 1/|dir|, per-frame sky(dir)
    PathLight* pl;              // [nsamples * nwork] light of each path (one 12-byte store per path)
    DevCounters* counters;
};
// k_frame (rt_frame.hip): the whole frame in one launch — primary rays, every sample's paths, the planes — for frames with little work
struct FrameArgs {
    uint32_t threshold;         // parked lanes per wave that trigger a transition pass (1..64; 0 = the default)
    uint32_t tiles_per_group;   // tiles of a (four-wave) workgroup; 0 = chosen by launch_frame from the frame's size and spp (RT_FRAME_TILES overrides)
    uint32_t pair_a;            // set by launch_frame: phase A walks two tiles at a time, one per ray slot (RT_FRAME_PAIR_A=0: one)
    const float4* sun_lut;      // as PersistArgs
    const float4* dif_lut;
    PathLight* pl;              // spp > 1: [pixel's out_index * spp + sample] light of each path, summed in sample order by the pixel's workgroup
    DevCounters* counters;
    unsigned long long* dbg_waves;   // counting build, diagnostics: four words per tile (null: none)
};
bool launch_frame_ok(const Frame& f);   // does k_frame cover this frame (depth <= 8)?
hipError_t launch_frame(const Scene& sc, const Frame& f, const Planes& pl, FrameArgs a, bool count, int num_cus, hipStream_t st);
hipError_t launch_accumulate_paths(const Frame& f, const Planes& planes, const PathLight* pl, const uint32_t* worklist,
                                   const uint32_t* wl_count, uint32_t npix_pad, uint32_t nsamples, bool first_batch, bool last_batch,
                                   bool cache, bool stream, float4* acc, float4* accum, bool accum_continue, int accum_div,
                                   uint32_t* zero_words, uint32_t zero_count, hipStream_t st);
// (accum: RT_FLAG_ACCUMULATE's running sums by out_index, null without; zero_words: the lane's path cursors, cleared for its next
// path launch, or null; see k_accumulate_paths)
// RT_FLAG_ACCUMULATE: accum[out] = (accum_continue ? accum[out] : 0) + reps x (16 x lighting_f32[out], a one-sample light, exactly),
// and the two lighting planes become that sum / n / 16 — for every pixel (one-sample frames, after the frame's launches) or only
// for the pixels a one-sample prepass finished (finished_only: sky pixels, or all of them at depth 0)
hipError_t launch_accumulate_frame(const Frame& f, const Planes& planes, float4* accum, uint32_t npix_pad, bool accum_continue, int n,
                                   int reps, bool finished_only, hipStream_t st);
hipError_t launch_sphere_lut(float4* lut, hipStream_t st);
hipError_t launch_dif_lut(const float4* sphere, float4* lut, hipStream_t st);
hipError_t launch_sun_lut(const Frame& f, float4* lut, hipStream_t st);
hipError_t launch_sky_lut(const Frame& f, float4* dif_lut, hipStream_t st);
hipError_t launch_primary(const Scene& sc, const Frame& f, const Planes& pl, const PrimaryArgs& a, bool count,
                          int version /* 1 = k_primary, 2 = k_primary2 */, int nworkgroups, hipStream_t st);
hipError_t launch_persist(const Scene& sc, const Frame& f, const Planes& pl, const PersistArgs& a, bool count, bool cache,
                          int version /* 1 = k_persist */, int nworkgroups, hipStream_t st);

// k_paths (rt_paths.hip): cached-primary frames with lr = 0 and region 256 only
bool launch_paths_direct_ok(const Frame& f);   // does k_paths honour PersistArgs::direct for this frame?
hipError_t launch_paths(const Scene& sc, const Frame& f, const Planes& pl, const PersistArgs& a, bool count, int nworkgroups,
                        hipStream_t st);

// rt_world.hip: the brick-swizzled region and its nibble maps.  A MapBoxes is the words of both maps that a change of the region
// touches: a box of coarse words in (x word, cube y, cube z) and a box of brick words in (x word, brick y, brick z), first + count.
struct MapBoxes { uint3 cw0, cwn, bw0, bwn; };
MapBoxes map_boxes_region(int logr);                              // every word
MapBoxes map_boxes_slab(int logr, int axis, int texel_offset);    // a 16-thick slab's
hipError_t launch_build_maps(const uint8_t* mine_sw, uint32_t* coarse, uint32_t* brick /* R > 256: the per-brick map, else null */,
                             int logr, const MapBoxes& boxes, hipStream_t st);
hipError_t launch_flatten(const uint8_t* mine_lin, const uint32_t* mat_lin, uint8_t* mine_sw, uint32_t* mat_sw,
                          uint32_t* coarse, uint32_t* brick, uint32_t* bad_flag, int logr, hipStream_t st);
hipError_t launch_flatten_slab(const uint8_t* mine_slab, const uint32_t* mat_slab, uint8_t* mine_sw, uint32_t* mat_sw, uint32_t* coarse,
                               uint32_t* brick, int logr, int axis, int offset, hipStream_t st);
hipError_t launch_check_maps(const uint8_t* mine_sw, const uint32_t* coarse, const uint32_t* brick, int logr,
                             unsigned long long* mismatches, hipStream_t st);   // rt_selftest(RT_SELFTEST_SCENE_MAPS)
hipError_t launch_read_box(const uint8_t* mine_sw, const uint32_t* mat_sw, int logr, int x0, int y0, int z0, int ex, int ey, int nz,
                           uint32_t* mat_out, uint8_t* mine_out, hipStream_t st);
// rt_edit.hip: rt_edit_voxels (chunk list, per-chunk edit ranges offs[0..n] and records as k_rebuild_chunks describes)
hipError_t launch_rebuild_chunks(uint8_t* mine_sw, uint32_t* mat_sw, const uint32_t* chunks, const uint32_t* offs, const uint2* recs,
                                 uint32_t nchunks, int logr, hipStream_t st);
// rt_edit_shapes: `shapes` = nshapes RtShapeEdit records (32 bytes each) as the caller gave them, validated on the host
hipError_t launch_shape_chunks(uint8_t* mine_sw, uint32_t* mat_sw, const uint32_t* chunks, const void* shapes, uint32_t nshapes,
                               uint32_t nchunks, int logr, hipStream_t st);
// rt_edit_stamps: `recs` = nrecs 64-byte placement records (api/edit_stamps.hpp, StampRecord), resolved and validated on the host
hipError_t launch_stamp_chunks(uint8_t* mine_sw, uint32_t* mat_sw, const uint32_t* chunks, const void* recs, uint32_t nrecs,
                               uint32_t nchunks, int logr, hipStream_t st);
// rt_stamp_capture: the region's box (x0, y0, z0) + [0, ex) x [0, ey) x [0, ez) into a stamp's arrays (x fastest; at most 2^24 voxels)
hipError_t launch_stamp_capture(const uint8_t* mine_sw, const uint32_t* mat_sw, int logr, int x0, int y0, int z0, int ex, int ey, int ez,
                                bool skip_air, uint32_t* mats_out, uint8_t* state_out, hipStream_t st);
// rt_stamp_create: clears the material words of the n voxels' ABSENT ones
hipError_t launch_stamp_clean(uint32_t* mats, const uint8_t* state, uint32_t n, hipStream_t st);
hipError_t launch_rebuild_chunk_maps(const uint8_t* mine_sw, uint32_t* coarse, uint32_t* brick, const uint32_t* chunks, uint32_t nchunks,
                                     int logr, hipStream_t st);
// rt_terrain.hip: rt_generate_world (axis = -1: the window [lo, lo + R) on every axis) and rt_generate_slice (axis 0..2: 16 voxels
// from lo[axis] along it); heights: int32 scratch for (R/64 + 1)^2 chunk columns of 64^2
hipError_t launch_terrain(uint8_t* mine_sw, uint32_t* mat_sw, uint32_t* coarse, uint32_t* brick, int32_t* heights, int logr,
                          uint64_t seed, const int64_t lo[3], int axis, hipStream_t st);
hipError_t launch_mega(const Scene& sc, const Frame& f, const Planes& pl, DevCounters* cn, bool count, hipStream_t st);
hipError_t launch_trace(const Scene& sc, const Frame& f, const TraceArgs& a, bool primary, bool count, int nworkgroups, hipStream_t st);
hipError_t launch_shade0(const Scene& sc, const Frame& f, const ShadeArgs& a, const Planes& pl, bool count, hipStream_t st);
hipError_t launch_shadeN(const Scene& sc, const Frame& f, const ShadeArgs& a, int level, bool count, hipStream_t st);
hipError_t launch_accumulate(const float* plx, const float* ply, const float* plz, float4* acc, uint32_t npix_pad,
                             uint32_t nsamples, bool first_batch, hipStream_t st);
hipError_t launch_resolve(const Frame& f, const float4* acc, const Planes& pl, uint32_t npix_pad, hipStream_t st);
hipError_t launch_untile_strided(const void* gathered, size_t rank_stride, void* frame, int world, int capacity, int tiles_x,
                                 int tiles_y, int width, int height, int bpp, hipStream_t st);
hipError_t launch_untile(const void* gathered, void* frame, int world, int capacity, int tiles_x, int tiles_y, int width,
                         int height, int bpp, hipStream_t st);

// rt_query.hip: ray queries against the resident region (rt_trace_rays, rt_pick_pixels)
struct QueryArgs {
    const float4* rays;   // RtRay[count] (two float4 each), or
    const int2* xy;       // non-null: pixel (x, y) of the frame's camera per query (primary_ray)
    uint4* hits;          // RtRayHit[count] (three uint4 each)
    uint32_t count;
};
hipError_t launch_query(const Scene& sc, const Frame& f, const QueryArgs& a, hipStream_t st);

// rt_probe.hip: light probes (rt_probe_light).  One launch covers `count` whole probes of `samples` paths each, at most kProbeMaxPaths
// paths; Frame supplies sunangle / sunlight, seed, lr, the region and `depth` (1..RT_MAX_DEPTH).
constexpr uint64_t kProbeMaxPaths = 1ull << 26;
struct ProbeArgs {
    const uint4* probes;  // RtLightProbe[count] (two uint4 each)
    uint4* out;           // RtProbeLight[count]
    float4* scratch;      // [count * samples] path records (light rgb, sun1.air bit) when !probe_sums_in_lds(samples); else unused
    uint32_t count, samples;
};
bool probe_sums_in_lds(uint32_t samples);   // a workgroup holds whole probes and adds their samples itself: no scratch, one launch
// pair: a lane steps the shadow and the diffuse ray of a level together (the shipped form); false: one after the other
hipError_t launch_probe(const Scene& sc, const Frame& f, const ProbeArgs& a, bool pair, hipStream_t st);

// rt_sweep.hip: box sweeps (rt_sweep_boxes).  One lane per sweep; `lr` is the window's centre in world voxels (RtUniforms.lr).
struct SweepArgs {
    const uint4* sweeps;  // RtBoxSweep[count] (three uint4 each)
    uint4* hits;          // RtSweepHit[count] (four uint4 each)
    uint32_t count;
    int32_t lr[3];
};
hipError_t launch_sweep(const Scene& sc, int logr, const SweepArgs& a, hipStream_t st);

// rt_step_particles.hip: one simulation tick of particles against the region (rt_step_particles).  One lane per particle, which
// reads its record whole before it writes: `out` may be `in`; no other overlap.  The parameters are RtParticleStep's, checked on the
// host (api/particle_step_check.hpp).
struct StepParticlesArgs {
    const uint4* in;      // RtParticleState[count] (four uint4 each)
    uint4* out;           // RtParticleState[count]
    uint4* draw;          // RtParticle[count] (two uint4 each), or null
    uint32_t count;       // at most kMaxParticles
    uint32_t sweeps;      // sub-sweeps per tick, 1..4
    int32_t lr[3];
    float dt, accel[3], damping, restitution, friction, rest_speed;
};
hipError_t launch_step_particles(const Scene& sc, int logr, const StepParticlesArgs& a, hipStream_t st);

// rt_emit.hip: debris from the occupied voxels of shapes into a ring of particle states (rt_emit_particles).  An ITEM is one
// (emitter, 4^3 brick) of the host's plan (api/emit_check.hpp, EmitRecord: eight uint4 per emitter that has a bounding box); one wave
// per item.  Three launches: count, scan (with the cursor update), write.
constexpr uint32_t kMaxEmitRecords = 256;      // emitters per call
constexpr uint32_t kMaxEmitItems = 1u << 18;   // items per call
struct EmitParticlesArgs {
    const uint4* recs;     // EmitRecord[nrecs], `first` ascending from 0
    uint4* states;         // the ring: RtParticleState[capacity] (four uint4 each)
    uint4* cursor;         // RtEmitCursor
    uint32_t* scratch;     // emit_scratch_words(items) words, 16-byte aligned
    uint32_t nrecs, items; // 1..kMaxEmitRecords, 1..kMaxEmitItems: the sum of the records' nbx * nby * nbz
    uint32_t capacity, max_emit;
    int32_t lr[3];
};
// The scratch of a call, in 4-byte words: [0] the ring slot of particle 0, [1] n, [2..3] unused, then per item its 64-bit mask of
// selected voxels, then per item the number of its first selected voxel.
inline size_t emit_scratch_words(uint32_t items) { return 4u + 3u * (size_t)items; }
hipError_t launch_emit_particles(const Scene& sc, int logr, const EmitParticlesArgs& a, hipStream_t st);

// rt_deposit.hip: resting particles into voxels of the region (rt_deposit_particles).  Two launches — claim (a lane per particle)
// and chunks (a workgroup per chunk of the clipped box, the chunk rebuild of rt_edit_voxels) — over a scratch the caller has filled
// with 0xFF bytes: one claim word per texel of the box (x fastest in box coordinates), then one flag word per chunk of the box
// (z-major: the order of the ascending chunk list), then a spare RtDepositCount for a call without counts.
constexpr uint64_t kMaxDepositTexels = 1ull << 24;   // texels of the clipped box
struct DepositArgs {
    uint4* states;         // RtParticleState[count] (four uint4 each): flags are updated in place
    uint4* draw;           // RtParticle[count] (two uint4 each) or nullptr
    uint32_t* counts;      // RtDepositCount (never nullptr: the scratch's spare where the caller gave none)
    uint32_t* claims;      // the scratch: texels words ...
    uint32_t* flags;       // ... and chunk words behind them
    uint32_t count;        // 1..kMaxParticles
    float max_speed;
    int32_t lr[3];
    int32_t lo[3], hi[3];  // the clipped box, texels, inclusive
};
inline size_t deposit_scratch_words(uint64_t texels, uint32_t nchunks) { return (size_t)texels + nchunks + 4u; }
// `chunks`: the ids of the box's nchunks chunks, ascending
hipError_t launch_deposit_particles(uint8_t* mine_sw, uint32_t* mat_sw, const uint32_t* chunks, uint32_t nchunks, int logr, const DepositArgs& a,
                                    hipStream_t st);

// rt_settle.hip: loose voxels of a box of texels fall along an axis (rt_settle_voxels).  Two launches — columns (a lane per column of
// the clipped box) and chunks (a workgroup per chunk of the box, the chunk rebuild of rt_edit_voxels) — over a scratch the caller has
// filled with 0xFF bytes: one flag word per chunk of the box (z-major: the order of the ascending chunk list), then a spare
// RtSettleCount for a call without counts.
struct SettleArgs {
    uint32_t* flags;       // the scratch: chunk words
    uint32_t* counts;      // RtSettleCount (never nullptr: the scratch's spare where the caller gave none)
    int32_t lo[3], hi[3];  // the clipped box, texels, inclusive
    uint32_t max_fall, air_material, loose_mask, loose_value;
    uint32_t axis, toward; // 0..2; 0 = towards lower texel coordinates
};
inline size_t settle_scratch_words(uint32_t nchunks) { return (size_t)nchunks + 4u; }
// `chunks`: the ids of the box's nchunks chunks, ascending
hipError_t launch_settle_voxels(uint8_t* mine_sw, uint32_t* mat_sw, const uint32_t* chunks, uint32_t nchunks, int logr, const SettleArgs& a,
                                hipStream_t st);

// rt_detach.hip: the unsupported voxels of a box of texels are found, carved and captured into a stamp (rt_detach_voxels).  A seed
// launch, max_passes reach launches and an apply launch, each a workgroup per chunk of the box (z-major over the box's chunks: the
// order of the ascending chunk list), then with RT_DETACH_CARVE the chunk rebuild of rt_edit_voxels behind a flag word's early exit.
// The scratch needs no fill: the seed launch writes every word a later launch reads.  Its layout, in words: the head — word p
// (1..256) says whether pass p changed anything, words kDetachSpareResult.. are a spare RtDetachResult —, a flag per chunk (to a
// multiple of four), then per chunk 64 x 64 rows of 64 bits along x (row z * 64 + y) three times: occupancy masked to the box, reach
// buffer 0, reach buffer 1.  Pass p reads buffer (p - 1) & 1 and writes buffer p & 1.
constexpr uint32_t kDetachMaxPasses = 256;
constexpr size_t kDetachChunkWords = 64u * 64u * 2u, kDetachHeadWords = 288u, kDetachSpareResult = 272u;
struct DetachArgs {
    uint32_t* scratch;     // detach_scratch_words(nchunks) words
    uint32_t* result;      // RtDetachResult (never nullptr: the scratch's spare where the caller gave none)
    uint32_t* stamp_mats;  // the new stamp's arrays over the clipped box, or nullptr without RT_DETACH_CAPTURE
    uint8_t* stamp_state;
    int32_t lo[3], hi[3];  // the clipped box, texels, inclusive
    uint32_t flags, air_material, anchor_mask, anchor_value, max_passes, anchor_faces;
};
__host__ __device__ inline size_t detach_flag_words(uint32_t nchunks) { return ((size_t)nchunks + 3u) & ~(size_t)3u; }
inline size_t detach_scratch_words(uint32_t nchunks) { return kDetachHeadWords + detach_flag_words(nchunks) + 3u * kDetachChunkWords * (size_t)nchunks; }
// `chunks`: the ids of the box's nchunks chunks, ascending (read only with RT_DETACH_CARVE)
hipError_t launch_detach_voxels(uint8_t* mine_sw, uint32_t* mat_sw, const uint32_t* chunks, uint32_t nchunks, int logr, const DetachArgs& a,
                                hipStream_t st);

// rt_flow.hip: a level-based fluid spreads, falls and dries inside a box of texels (rt_flow_voxels).  A seed launch (a lane per cell:
// the cell's state from its minefield byte and material word; the head of the scratch), `launches` tick launches of at most `group`
// ticks each — a workgroup per tile of 32 x 16 x 16 cells with a halo of `group` cells runs them in LDS, ping-ponging the two state
// arrays —, an apply launch (a lane per cell: the final byte and word against the world, the counts, the chunk flags, one more tick
// from the global states for `active`), then the chunk rebuild of rt_edit_voxels behind a flag word's early exit.  The scratch needs
// no fill.  Its layout, in words: the head — word j says whether tick launch j changed a cell, words kFlowSpareCount.. are a spare
// RtFlowCount, words kFlowChunkFlags.. a flag per chunk of the box (z-major: the order of the ascending chunk list) —, then the two
// state arrays, a byte per cell, [z][y][x] over the clipped box with rows padded to a multiple of four cells.  Tick launch j reads
// array j & 1 and writes array (j + 1) & 1.  A state: 0 empty, 1..13 flowing with that strength, 14 source, 15 fixed.
constexpr uint32_t kFlowMaxTicks = 256, kFlowMaxLevel = 13, kFlowMaxChunks = 125;
constexpr int32_t kFlowMaxExtent = 256;
constexpr size_t kFlowHeadWords = 512u, kFlowSpareCount = 256u, kFlowChunkFlags = 272u;
constexpr uint32_t kFlowSource = 14u, kFlowFixed = 15u;
struct FlowArgs {
    uint32_t* scratch;     // flow_scratch_words(lo, hi) words
    uint32_t* counts;      // RtFlowCount (never nullptr: the scratch's spare where the caller gave none)
    int32_t lo[3], hi[3];  // the clipped box, texels, inclusive
    uint32_t ticks, air_material, fluid_mask, fluid_value, fluid_word;
    uint32_t level_shift, max_level;
};
__host__ __device__ inline uint32_t flow_row_cells(int ex) { return ((uint32_t)ex + 3u) & ~3u; }
__host__ __device__ inline size_t flow_state_words(const int32_t lo[3], const int32_t hi[3]) {
    return (size_t)(flow_row_cells(hi[0] - lo[0] + 1) / 4u) * (size_t)(hi[1] - lo[1] + 1) * (size_t)(hi[2] - lo[2] + 1);
}
inline size_t flow_scratch_words(const int32_t lo[3], const int32_t hi[3]) { return kFlowHeadWords + 2u * flow_state_words(lo, hi); }
// `chunks`: the ids of the box's nchunks chunks, ascending; `group`: 1, 2, 4 or 8 ticks per launch
hipError_t launch_flow_voxels(uint8_t* mine_sw, uint32_t* mat_sw, const uint32_t* chunks, uint32_t nchunks, int logr, const FlowArgs& a,
                              uint32_t group, hipStream_t st);

// rt_nav.hip: navigation fields (rt_nav_build, rt_nav_sample).  A build is level-synchronous breadth-first search on bitmaps, backwards
// from the goals over the predecessor relation: a seed launch (the box's unoccupied bits, the field's fill, the head cleared), a
// launch that derives and counts the standable cells, a lane per goal, `launches` level launches of `levels` levels each — a
// workgroup per tile of 16 x 16 columns over the box's whole z extent, with a halo of `levels` columns, runs them in LDS — and a
// launch that gives every reached cell its move code.  The scratch needs no fill.  Its layout, in words: the head — word j says
// whether level launch j has a frontier to start from, word kNavTruncWord whether a cell lies at max_dist + 1, words
// kNavSpareResult.. are a spare RtNavResult —, then five bitmaps of nav_bitmap_words each, rows of bits along x per (y, z) in 16-bit
// pieces: unoccupied, unreached standable cells (two buffers), frontier (two buffers).  Level launch j reads buffers j & 1 and
// writes buffers (j + 1) & 1.
constexpr size_t kNavHeadWords = 4112u, kNavTruncWord = 4100u, kNavSpareResult = 4104u;
constexpr uint32_t kNavMaxDist = 4096u, kNavMaxGoals = 4096u, kNavMaxAgents = 1u << 20;
struct NavArgs {
    uint32_t* scratch;     // nav_scratch_words(ext) words
    uint16_t* dist;        // [ez][ey][ex]
    uint8_t* move;         // [ez][ey][ex]
    uint32_t* result;      // RtNavResult (never nullptr: the scratch's spare where the caller gave none)
    const int4* goals;     // RtNavGoal[goal_count]
    int32_t lo[3], ext[3];
    uint32_t max_dist, goal_count;
    int32_t height, max_climb, max_drop, goal_snap;
};
__host__ __device__ inline uint32_t nav_row_halves(int ex) { return ((((uint32_t)ex + 15u) >> 4) + 1u) & ~1u; }
__host__ __device__ inline size_t nav_bitmap_words(const int32_t ext[3]) { return (size_t)ext[1] * (size_t)ext[2] * (size_t)(nav_row_halves(ext[0]) / 2u); }
inline size_t nav_scratch_words(const int32_t ext[3]) { return kNavHeadWords + 5u * nav_bitmap_words(ext); }
// `levels`: 1, 4 or 8
hipError_t launch_nav_build(const uint8_t* mine_sw, int logr, const NavArgs& a, uint32_t levels, hipStream_t st);
struct NavSampleArgs {
    const uint16_t* dist;
    const uint8_t* move;
    const uint4* agents;   // RtNavAgent[count]
    uint4* steps;          // RtNavStep[count] (two uint4 each)
    uint32_t count;
    int32_t lo[3], ext[3];
};
hipError_t launch_nav_sample(const NavSampleArgs& a, hipStream_t st);

// rt_boxes.hip: entity boxes composited into a whole frame's row-major planes by depth (rt_draw_boxes).  One launch for the batch;
// a wave owns an 8x8 pixel tile.
struct DrawBoxesArgs {
    const uint4* boxes;   // RtDrawBox[count] (two uint4 each)
    const float4* lights; // RtProbeLight[6 * count]: record 6 b + n lights face n of box b (.xyz read)
    uint32_t count;
    int width, height;
    float origin[3], forward[3], up[3], right[3];   // the camera of the frame the planes hold (primary_ray without the slide)
};
hipError_t launch_draw_boxes(const Planes& pl, const DrawBoxesArgs& a, hipStream_t st);

// rt_draw_stamps.hip: voxel-model entities (stamps placed at float positions) composited likewise (rt_draw_stamps).  One launch for
// the batch; a wave owns an 8x8 pixel tile.
struct DrawStampsArgs {
    const uint4* recs;    // DrawStampRecord[count] (api/draw_stamps.hpp; four uint4 each), resolved and validated on the host
    const float4* lights; // RtProbeLight[6 * count]: record 6 i + n lights bounding-box face n of model i (.xyz read)
    uint32_t count;
    int width, height;
    float origin[3], forward[3], up[3], right[3];   // as DrawBoxesArgs
};
hipError_t launch_draw_stamps(const Planes& pl, const DrawStampsArgs& a, hipStream_t st);

// rt_particles.hip: up to 2^20 small cubes composited likewise (rt_draw_particles): every pixel ends as launch_draw_boxes would leave
// it for the cubes' boxes, but a tile reads only the particles binned to it.  Four launches behind one memset: bin (a thread per
// particle finds the rectangle of tiles it may touch and counts itself into them, or joins the wide list), offsets (a thread per
// tile claims its segment of the pair buffer), fill (a thread per particle again), draw (a wave per tile).
constexpr uint32_t kMaxParticles = 1u << 20;       // particles per call, and light records per call
constexpr uint32_t kParticleBinTiles = 16;         // W: a particle whose rectangle holds more tiles is listed by 8x8-tile blocks; more blocks: wide
struct ParticleArgs {
    const uint4* particles;  // RtParticle[count] (two uint4 each)
    const float4* lights;    // RtProbeLight[nlights] (.xyz read)
    uint32_t* scratch;       // particle_scratch_words(count, width, height) words
    uint32_t count, nlights;
    int width, height;
    float origin[3], forward[3], up[3], right[3];   // as DrawBoxesArgs
};
// The scratch of a call, in 4-byte words: [0] the wide list's length, [1] the pairs handed out, then per list — one per 8x8 tile, then
// one per block of 8x8 tiles — its pair count and its cursor into the pair buffer, then per particle its rectangle word and its place
// in the wide list, then the kParticleBinTiles * count pairs — which cannot overflow: a binned particle adds at most
// kParticleBinTiles of them, to tiles' lists or to blocks'.
__host__ __device__ inline size_t particle_lists(int width, int height) {
    const size_t tx = ((size_t)width + 7u) / 8u, ty = ((size_t)height + 7u) / 8u;
    return tx * ty + ((tx + 7u) / 8u) * ((ty + 7u) / 8u);
}
inline size_t particle_scratch_words(uint32_t count, int width, int height) {
    return 2u + 2u * particle_lists(width, height) + (size_t)(2u + kParticleBinTiles) * count;
}
hipError_t launch_draw_particles(const Planes& pl, const ParticleArgs& a, hipStream_t st);

// rt_lights.hip: point lights added to the lighting planes of a whole frame's row-major planes (rt_add_lights).  One launch for the
// batch; a wave owns an 8x8 pixel tile.  Frame supplies the camera of the frame the planes hold (origin, forward, up, right: the ray
// of rt_draw_boxes), lr and the region.
struct LightsArgs {
    const uint4* lights;  // RtPointLight[count] (two uint4 each)
    uint32_t count;
};
hipError_t launch_add_lights(const Scene& sc, const Frame& f, const Planes& pl, const LightsArgs& a, hipStream_t st);

// rt_shadows.hip: the sun's direct term taken out of the lighting planes of a whole frame's row-major planes where an entity shades
// the pixel (rt_shadow_entities).  One launch for boxes and models together; a wave owns an 8x8 pixel tile.  Frame supplies the camera
// of the frame the planes hold, lr, the region and sunangle / sunlight.
struct ShadowArgs {
    const uint4* boxes;   // RtDrawBox[nboxes] (two uint4 each; lo and hi are read)
    const uint4* recs;    // DrawStampRecord[nmodels] (api/draw_stamps.hpp; four uint4 each), resolved and validated on the host
    uint32_t nboxes, nmodels;
    float strength;       // (0, 1]
};
hipError_t launch_shadow_entities(const Scene& sc, const Frame& f, const Planes& pl, const ShadowArgs& a, hipStream_t st);

// rt_lights.hip: launch_add_lights with the drawn entities as occluders of each (pixel, light) segment (rt_add_lights_occluded).  One
// launch; a wave owns an 8x8 pixel tile and culls the occluders once against the hull of its segments.
struct LightShadowArgs {
    const uint4* lights;  // RtPointLight[count] (two uint4 each)
    const uint4* boxes;   // RtDrawBox[nboxes] (two uint4 each; lo and hi are read); an invalid box is skipped
    const uint4* recs;    // DrawStampRecord[nmodels] (api/draw_stamps.hpp; four uint4 each), resolved and validated on the host
    uint32_t count, nboxes, nmodels;
};
hipError_t launch_add_lights_occluded(const Scene& sc, const Frame& f, const Planes& pl, const LightShadowArgs& a, hipStream_t st);

// rt_entity_query.hip: ray and pixel queries against drawn entities (rt_trace_entities, rt_pick_entities).  One launch, one lane per
// ray: the world's hit as rt_query.hip finds it, then the nearest box or model under the draws' rules, depth-tested against it.
struct EntityQueryArgs {
    const float4* rays;   // RtRay[count] (two float4 each), or
    const int2* xy;       // non-null: pixel (x, y) of the frame's camera per query
    uint4* world_hits;    // RtRayHit[count] (three uint4 each), or null
    uint4* entity_hits;   // RtEntityHit[count] (three uint4 each)
    const uint4* boxes;   // RtDrawBox[nboxes] (two uint4 each); an invalid box is skipped
    const uint4* recs;    // DrawStampRecord[nmodels] (api/draw_stamps.hpp; four uint4 each), resolved and validated on the host
    uint32_t count, nboxes, nmodels;
};
hipError_t launch_entity_query(const Scene& sc, const Frame& f, const EntityQueryArgs& a, hipStream_t st);

// rt_sweep_entities.hip: box sweeps against the region and the drawn entities (rt_sweep_entities).  One launch, one lane per sweep:
// the world's hit as rt_sweep.hip finds it, then the first box or model cell that embeds or blocks the sweep before the world does.
struct SweepEntitiesArgs {
    const uint4* sweeps;  // RtBoxSweep[count] (three uint4 each); reserved0 / reserved1 name the box / model the sweep ignores, plus 1
    uint4* world_hits;    // RtSweepHit[count] (four uint4 each), or null
    uint4* entity_hits;   // RtEntitySweepHit[count] (five uint4 each)
    const uint4* boxes;   // RtDrawBox[nboxes] (two uint4 each); an invalid box is skipped
    const uint4* recs;    // DrawStampRecord[nmodels] (api/draw_stamps.hpp; four uint4 each), resolved and validated on the host
    uint32_t count, nboxes, nmodels;
    int32_t lr[3];
};
hipError_t launch_sweep_entities(const Scene& sc, int logr, const SweepEntitiesArgs& a, hipStream_t st);

// rt_temporal.hip: RT_FLAG_REPROJECT's pass over a one-sample whole-frame (it replaces launch_accumulate_frame there)
// (TEMPORAL_MOVED_BOXES: a moved frame after rt_edit_voxels on a context with RtConfig.edit_radius > 0 — pixels near an edited box
// or in its sun shadow restart, the others go on as in TEMPORAL_MOVED)
// (TEMPORAL_MOVED_SLABS: a moved frame after rt_upload_slice / rt_generate_slice on a context with RtConfig.stream_history — the
// test of TEMPORAL_MOVED_BOXES against the frame's edit boxes, 0..kTemporalMaxBoxes of them, and then against the boxes
// k_place_slab_boxes left in device memory)
enum { TEMPORAL_RESTART = 0, TEMPORAL_STILL = 1, TEMPORAL_MOVED = 2, TEMPORAL_MOVED_BOXES = 3, TEMPORAL_MOVED_SLABS = 4 };
constexpr uint32_t kTemporalMaxBoxes = 16;
struct TemporalBox { float lo[3], hi[3]; };   // world coordinates, [first voxel, last voxel + 1] per axis
// rt_slab.hip: RtConfig.stream_history.  A pending slab owns one of kSlabSlots mask slots: two sets (what the slab held just before
// it was written, what it holds just after), each three rows of kSlabMaskWords words — bit t of row a is set when an occupied voxel
// (minefield byte 0) of the slab has coordinate t on axis a.  k_place_slab_boxes turns the pending slots into world boxes.
constexpr uint32_t kSlabSlots = 4, kSlabMaskWords = 32, kSlabSetWords = 3 * kSlabMaskWords, kSlabSlotWords = 2 * kSlabSetWords;
constexpr uint32_t kSlabMaxBoxes = 2 * kSlabSlots;
struct SlabBoxes { uint32_t count, pad[3]; TemporalBox box[kSlabMaxBoxes]; };
// ORs the occupancy of the 16-thick slab at texel `offset` of `axis` into masks[kSlabSetWords] (cleared by the caller)
hipError_t launch_slab_occupancy(const uint8_t* mine_sw, int logr, int axis, int offset, uint32_t* masks, hipStream_t st);
// slots 0..nslots-1 of masks (kSlabSlotWords each), in order: the old set placed with lr_prev, the new one with lr_cur; w(t) =
// lr - R/2 + (t - lr) mod R per set bit, the box [min w, max w + 1] per axis; a set without a bit gives no box
hipError_t launch_place_slab_boxes(const uint32_t* masks, uint32_t nslots, const int32_t lr_prev[3], const int32_t lr_cur[3], int logr,
                                   SlabBoxes* out, hipStream_t st);
struct TemporalArgs {
    const float4* prev_sum;   // the history set the previous frame's pass wrote: sums by row-major pixel ...
    const uint2* prev_rec;    // ... and (depth_f32 bits, count | normal << 27)
    float4* next_sum;         // the set this pass writes
    uint2* next_rec;
    float origin[3], forward[3], right[3], up[3];   // the previous frame's camera (TEMPORAL_MOVED)
    uint32_t cap;             // most samples a history carries across a camera change (1..65535)
    // TEMPORAL_MOVED_BOXES only (appended: the other modes read what they read before, at the offsets they had)
    uint32_t nbox;            // edited boxes in use (1..kTemporalMaxBoxes)
    TemporalBox box[kTemporalMaxBoxes];
    float r2;                 // (float)(edit_radius^2)
    float sun[3], inv_sun[3]; // Frame::sunangle and 1.0f / it, divided on the host
    // TEMPORAL_MOVED_SLABS only (appended likewise)
    const SlabBoxes* slab;    // what k_place_slab_boxes wrote in front of this launch, in stream order
};
hipError_t launch_temporal_frame(const Frame& f, const Planes& planes, const TemporalArgs& a, int mode, hipStream_t st);

// rt_post.hip: the reference's post passes
hipError_t launch_denoise_prepare(const void* lighting, const void* depth, const void* normal, int W, int H, void* work,
                                  hipStream_t st);
hipError_t launch_denoise(const void* work_in, int W, int H, int size, bool swapped, bool last, void* work_out, void* lighting,
                          hipStream_t st);
// the history-aware dispatches (rt_denoise_history, rt_denoise_planes_counted): `counts` is the history record of RT_FLAG_REPROJECT
// (TemporalArgs::next_rec) or a row-major u32 plane; settle 0 = nobody settles, else 1..127
hipError_t launch_denoise_prepare_counted(const void* lighting, const void* depth, const void* normal, const void* counts,
                                          bool counts_are_records, int W, int H, void* work, hipStream_t st);
hipError_t launch_denoise_counted(const void* work_in, int W, int H, int size, bool swapped, bool last, bool weight, uint32_t settle,
                                  void* work_out, void* lighting, hipStream_t st);
hipError_t launch_selftest_dn_div(unsigned long long* mismatches_dev, hipStream_t st);
hipError_t launch_finalize(const void* albedo, const void* emission, const void* fog, const void* lighting, const void* depth,
                           const uint32_t* noise, int W, int H, void* out_bgra8, hipStream_t st);

}  // namespace rtd
