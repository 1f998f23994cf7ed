/*
 * rt_abi.h — C ABI of the MI355X-native ray-trace hot path (librt_amd.so).
 *
 * This is the drop-in boundary for the per-pixel path of someguynamedjosh/raytrace:
 * what the reference does in shaders/glsl/raytrace.comp behind `render::Pipeline`
 * is done here by hand-written gfx950 HIP kernels behind plain `extern "C"` entry
 * points (plain pointers and sizes only; no C++/torch types cross this line).
 * A Rust host binds these with an `extern "C"` block.
 *
 * Every entry point cites the reference interface it replaces (paths relative to
 * the reference repository root).
 *
 * Conventions
 *   - All functions returning int return RT_OK (0) or a negative RtStatus; they
 *     never throw or abort (the reference panics via .expect(): pipeline.rs:145,167).
 *   - Host pointers are borrowed for the duration of the call only; the context
 *     owns all device memory (reference: Vulkan objects owned by RenderData).
 *   - A context is used from one host thread at a time (reference: Rc<Core> is !Send,
 *     render/mod.rs:40).
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- constants restated from src/render/constants.rs:15-33 and raytrace.comp:37-58 ---- */
#define RT_CHUNK_SIZE        64      /* constants.rs:23  CHUNK_SIZE = 1 << MAX_CHUNK_LOD      */
#define RT_MAX_CHUNK_LOD     6       /* constants.rs:22                                       */
#define RT_ROOT_CHUNK_SIZE   4       /* constants.rs:26                                       */
#define RT_ROOT_BLOCK_SIZE   256     /* constants.rs:27; raytrace.comp:37 ROOT_BLOCK_WIDTH    */
#define RT_SLICE_SIZE        16      /* constants.rs:30                                       */
#define RT_SHADER_GROUP_SIZE 8       /* constants.rs:33; raytrace.comp:9 local_size 8x8       */
#define RT_PIXEL_SPREAD      16      /* raytrace.comp:54                                      */
#define RT_NOISE_SIZE        512     /* constants.rs:16-17; raytrace.comp:43                  */
#define RT_NOISE_BYTES       (512 * 512 * 4) /* constants.rs:19 BLUE_NOISE_SIZE               */
#define RT_LIGHTING_SCALE    16.0f   /* raytrace.comp:57                                      */
#define RT_TRACE_LIMIT       2048    /* raytrace.comp:109                                     */
#define RT_NORMAL_AIR        16      /* raytrace.comp:369 value stored for sky pixels         */
#define RT_DEPTH_AIR         0xFFFF  /* raytrace.comp:357                                     */
#define RT_MAX_DEPTH         16      /* build limit on the `depth` extension      */

typedef enum RtStatus {
    RT_OK = 0,
    RT_ERR_INVALID_ARG = -1,
    RT_ERR_NO_DEVICE = -2,      /* no HIP device / HIP runtime failure at create          */
    RT_ERR_HIP = -3,            /* a HIP call failed; see rt_last_error                   */
    RT_ERR_NOT_READY = -4,      /* draw before world/noise upload                         */
    RT_ERR_UNIMPLEMENTED = -5,
    RT_ERR_OOM = -6
} RtStatus;

/*
 * RtUniforms — byte-identical to `RaytraceUniformData` (src/render/pipeline/structs.rs:3-31)
 * and the GLSL std140 block `UniformData` (shaders/glsl/raytrace.comp:25-35). 192 bytes.
 * Live fields: sun_angle@0 seed@4 origin@16 forward@32 up@48 right@64 lr@160.
 * Dead in the shader (kept for layout): old_origin@80 old_transform_c0..2@96/112/128
 * region_offset@144 lso@176.
 */
typedef struct RtUniforms {
    float    sun_angle;           /*   0 */
    uint32_t seed;                /*   4 */
    uint32_t _padding0[2];        /*   8  (u64 in the reference)                       */
    float    origin[3];           /*  16 */
    uint32_t _padding1;
    float    forward[3];          /*  32 */
    uint32_t _padding2;
    float    up[3];               /*  48  pre-scaled by 0.4 on the host: pipeline.rs:198 */
    uint32_t _padding3;
    float    right[3];            /*  64  pre-scaled by 0.4 on the host: pipeline.rs:199 */
    uint32_t _padding4;
    float    old_origin[3];       /*  80  dead */
    uint32_t _padding5;
    float    old_transform_c0[3]; /*  96  dead */
    uint32_t _padding6;
    float    old_transform_c1[3]; /* 112  dead */
    uint32_t _padding7;
    float    old_transform_c2[3]; /* 128  dead */
    uint32_t _padding8;
    int32_t  region_offset[3];    /* 144  dead */
    uint32_t _padding9;
    int32_t  lr[3];               /* 160  `rotation` in structs.rs:27; `lr` in the shader */
    uint32_t _padding10;
    int32_t  lso[3];              /* 176  `space_offset`; dead */
    uint32_t _padding11;
} RtUniforms;

/* Which traversal implementation a context uses. */
typedef enum RtKernel {
    RT_KERNEL_DEFAULT = 0,    /* library picks per frame: frame (one-sample frames < 2.5 M pixels) / paths / persistent by work size */
    RT_KERNEL_MEGA = 1,       /* one thread per pixel, all rays inline, byte minefield from HBM (baseline)      */
    RT_KERNEL_WAVEFRONT = 2,  /* split stages: persistent traversal kernel fed by SoA ray/hit queues in HBM     */
    RT_KERNEL_PERSISTENT = 3, /* production kernel: persistent wave64 path kernel, a lane owns a path with its shadow
                                 and diffuse ray in two ray slots, state in registers, __ballot batched transitions,
                                 nibble map in LDS, per-XCD path cursors                                         */
    /* 4 was RT_KERNEL_PERSISTENT2 (two paths per lane, one slot each): retired in round 3, rejected by rt_create */
    RT_KERNEL_PATHS = 5,      /* a lane carries two paths with two ray slots each (four fetch chains in flight per lane) and
                                 the step loop is branch-free; frames it does not cover (no primary cache)
                                 run on RT_KERNEL_PERSISTENT                                                     */
    /* 6 was RT_KERNEL_SEQ (three paths per lane, one ray slot each): retired in round 4 (ABI 1.2), rejected by rt_create */
    RT_KERNEL_FRAME = 7,      /* (ABI 1.3) the whole frame in ONE launch: waves walk the primary rays of 8x8 tiles and then every
                                 sample's path of each of their workgroup's pixels (a pixel's samples added in order by its
                                 workgroup; no prepass, worklist or accumulate launch).  What RT_KERNEL_DEFAULT runs for frames
                                 with little work: the reference's own 1024 x 1024, 1 sample, depth 2 (one-sample frames below
                                 2.5 M pixels) and multi-sample frames below 1.5 M pixel-sample-levels.  Needs
                                 RT_FLAG_CACHE_PRIMARY (or one sample per pixel), depth <= 8 and the frame's light records in one
                                 launch's array; other frames of such a context run on RT_KERNEL_PATHS / RT_KERNEL_PERSISTENT  */
} RtKernel;

#define RT_FLAG_COUNTERS      0x1u  /* count rays/iterations/hits exactly (slower; for B_alg + parity)   */
#define RT_FLAG_CACHE_PRIMARY 0x2u  /* spp>1: trace the (seed-independent) primary ray once per pixel    */
#define RT_FLAG_TIMING        0x4u  /* bracket the traversal-kernel launches with HIP events (RtTiming.trace_ms)  */
#define RT_FLAG_TIMING_ALL    0xCu  /* ... and every other launch and the frame as well (shade_ms, frame_ms); includes RT_FLAG_TIMING */
#define RT_FLAG_TRUSTED_WORLD 0x10u /* rt_upload_slice: the host vouches that every minefield value is <= 30 (the reference
                                       writes 0..6); the slab is applied without the host-side scan of its bytes        */
#define RT_FLAG_FRAMES_IN_FLIGHT_2 0x20u /* (ABI 1.2) two frames in flight: consecutive rt_draw_frame calls render into two frame
                                       slots (two sets of output planes) on two streams, so that frame k + 1's kernels take the CUs
                                       frame k's draining path kernel leaves — the reference keeps one frame in flight behind its
                                       fence (pipeline.rs:162-172), and a host that waits (rt_sync) after every frame sees no
                                       difference.  What changes for a host that does not: rt_device_ptr / rt_gbuffer_ptr return
                                       the planes of the frame drawn LAST and alternate from frame to frame (the planes of frame k
                                       stay intact until frame k + 2 is drawn); rt_readback, rt_denoise, rt_finalize and
                                       rt_gather_gbuffer act on the frame drawn last and are ordered after it; rt_sync waits for
                                       every frame.  Persistent kernels (DEFAULT / PERSISTENT / PATHS) on the context's own stream
                                       only: ignored elsewhere and after rt_set_stream(non-NULL).                          */
#define RT_FLAG_ACCUMULATE 0x40u /* (ABI 1.3, additive) progressive accumulation while the camera holds still: the context keeps a
                                       per-pixel fp32 running sum of the lighting (npix_pad x 16 B of device memory, RtInfo.device_bytes,
                                       shared by the frame slots, untouched by rt_denoise / rt_finalize) and, on the host, the number
                                       of samples it holds.  A frame CONTINUES the accumulation when a frame was drawn before and its
                                       live uniforms other than seed (sun_angle, origin, forward, up, right, lr) are bitwise equal to
                                       that frame's, none of rt_upload_world / rt_upload_slice / rt_upload_noise / rt_reset_accumulation
                                       / rt_edit_voxels (count > 0) was called since, and samples + spp <= 2^24; otherwise it starts from zero and is bit-identical to
                                       the same frame without the flag.  The dead uniform fields are ignored and seed is not checked: a
                                       host that advances seed by spp per frame (mod RT_NOISE_BYTES; spp 1: the reference's own +1)
                                       gets after K frames of spp samples exactly the frame of K x spp samples from the first seed
                                       (RtConfig.spp: the ordered fp32 sum continues where the previous frame left it).  Then
                                       lighting_f32 / lighting_rgba16 = sum of all the samples / n / 16; the other planes and RtCounters
                                       are the frame's own.  One-sample frames run as before plus one bandwidth pass (k_accumulate_frame);
                                       frames of more samples do not run on RT_KERNEL_FRAME's k_frame (small ones lose its speed-up)
                                       but on the persistent kernels, whose prepass and accumulate launch continue the sum.
                                       RT_KERNEL_DEFAULT / FRAME / PATHS / PERSISTENT; rt_create rejects it on MEGA and WAVEFRONT
                                       (RT_ERR_UNIMPLEMENTED).  See rt_reset_accumulation / rt_get_accumulation.             */
#define RT_FLAG_REPROJECT 0x80u /* (ABI 1.3, additive) temporal reprojection: an RT_FLAG_ACCUMULATE context of one-sample whole frames
                                       keeps its lighting history when the camera moves.  Valid only together with RT_FLAG_ACCUMULATE
                                       (else RT_ERR_INVALID_ARG), with spp == 1 and tile_world == 1 (else RT_ERR_UNIMPLEMENTED).  The
                                       context owns two history sets used in turn (a frame's pass reads one and writes the other): per
                                       pixel the fp32 sum of its lights, the frame's depth_f32 and a word count | normal << 27 —
                                       npix_pad x 32 B more than RT_FLAG_ACCUMULATE alone (RtInfo.device_bytes) — and, on the host, the
                                       previous frame's camera.  rt_draw_frame classifies the frame:
                                         restart  no frame before, a world / noise change or rt_reset_accumulation since (the list of
                                                  RT_FLAG_ACCUMULATE, rt_generate_* included), sun_angle differs, or the count would
                                                  pass 2^24: every pixel sum = 0 + L, n = 1;
                                         still    every live uniform other than seed bitwise equal: sum = sum_prev + L, n = n_prev + 1
                                                  (a context that never moves is bit-identical to RT_FLAG_ACCUMULATE alone);
                                         moved    origin, forward, up, right or lr differ: per pixel, the hit point rebuilt from
                                                  depth_f32 is projected into the previous camera; the history of the nearest previous
                                                  pixel is taken when it has the same normal and lies on the same face plane (at most
                                                  0.25 apart along the normal's axis), scaled down to RtConfig.history_cap samples when
                                                  it holds more; every other pixel (sky, off screen, disoccluded) restarts.
                                       L = 16 x lighting_f32 of the frame just drawn; lighting_f32 / lighting_rgba16 = sum / n / 16 with
                                       the pixel's own n (rt_read_history); the other planes are the frame's own.  The arithmetic is
                                       fixed (DESIGN.md "Reprojection"; restated in tests/temporal_ref.py) and reproduced bit for bit.
                                       One launch per frame (k_temporal_frame) in place of k_accumulate_frame.
                                       RtConfig.edit_radius > 0 keeps the history across rt_edit_voxels: each call records one box per
                                       touched 64^3 chunk (the texel min / max of its records; at most 16 may wait, see
                                       rt_edit_boxes_pending) and the next frame drawn consumes them.  If that frame would be still or
                                       moved it is
                                         moved with boxes  the moved pass — also under an unchanged camera, where it projects into the
                                                  same camera — in which a pixel whose rebuilt hit point lies within edit_radius voxels
                                                  of an edited box, or from which the ray towards the sun meets a box grown by 1 voxel,
                                                  restarts (sum = 0 + L, n = 1) and every other pixel goes on as in a moved frame;
                                       a frame that restarts anyway, or whose set overflowed, restarts as before and drops the boxes.
                                       Boxes are texels until that frame's lr places them in the world (a box cut by the window's seam
                                       covers the whole window on that axis).  Bounce light beyond the radius and sky occlusion are
                                       not tested: they fade through history_cap.  DESIGN.md "Edits under a kept history".
                                       RtConfig.stream_history = 1 keeps the history across rt_upload_slice and rt_generate_slice as
                                       well: an accepted slab takes one of 4 pending slots (rt_slabs_pending), and the device records
                                       per axis which texels hold an occupied voxel (minefield byte 0) of the slab just before and
                                       just after it is written.  The next frame drawn consumes the slots like edit boxes: it places
                                       what left with the previous frame's lr and what arrived with its own — per set bit, so that the
                                       window's seam costs nothing — into at most 8 world boxes on the device (rt_read_slab_boxes) and
                                       runs the moved pass with the same near / sun-shadow test against the frame's edit boxes, then
                                       those.  A fifth slab empties the set and the next frame restarts.  One box per content is
                                       conservative for a slab whose terrain is tall in one corner.  DESIGN.md "Slabs under a kept
                                       history".                                                                                 */

/*
 * RtConfig — replaces the compile-time window constants (constants.rs:9-10) and adds the
 * build's extensions: spp, depth, and the multi-GPU tile split.
 *   spp = N   : N frames with seed, seed+1, ... (mod RT_NOISE_BYTES, pipeline.rs:201);
 *               lighting = (sum_i light_i) / N in fp32; other planes from the primary hit.
 *   depth = D : light recursion truncated at D levels; D=2 is exactly raytrace.comp:321-350.
 *   tile_rank/tile_world : this context renders only the 8x8-pixel tiles t with
 *               t % tile_world == tile_rank (t = row-major tile index); outputs are then
 *               tile-major (see rt_tile_count / rt_untile).  tile_world=1 => whole frame,
 *               row-major pixel layout, row 0 = bottom of the view (finalize.comp:60-63).
 */
typedef struct RtConfig {
    uint32_t struct_size;   /* sizeof(RtConfig), for forward compatibility */
    int32_t  width;
    int32_t  height;
    int32_t  region;        /* region edge R: 256 = the reference (ROOT_BLOCK_WIDTH); 512 and 1024 are extensions (C5) */
    int32_t  spp;           /* >= 1 */
    int32_t  depth;         /* 0..RT_MAX_DEPTH */
    int32_t  device;        /* HIP device ordinal */
    int32_t  tile_rank;
    int32_t  tile_world;
    int32_t  kernel;        /* RtKernel */
    uint32_t flags;         /* RT_FLAG_* */
    int32_t  history_cap;   /* (was reserved[0]) RT_FLAG_REPROJECT: the most samples a pixel's history carries across a camera
                               change; 0 = the default, 32; valid 1..65535 (else RT_ERR_INVALID_ARG).  Ignored without the flag. */
    int32_t  edit_radius;   /* (was reserved[0]) RT_FLAG_REPROJECT: 0 = rt_edit_voxels restarts the lighting history; 1..64 = it keeps
                               the history, and the next frame restarts only the pixels whose hit point lies within this many voxels
                               of an edited box or in the sun shadow of one; anything else RT_ERR_INVALID_ARG.  Ignored without
                               the flag. */
    int32_t  stream_history;/* (was reserved[0]) RT_FLAG_REPROJECT: 0 = rt_upload_slice and rt_generate_slice restart the lighting
                               history; 1 = they keep it, and the next frame restarts only the pixels near the occupied voxels that
                               left or arrived or in their sun shadow — the test of edit_radius, which must then be 1..64; anything
                               else RT_ERR_INVALID_ARG.  Ignored without the flag. */
    int32_t  reserved[2];
} RtConfig;

/* Output planes. Bindings cited from shaders/glsl/raytrace.comp:14-21; formats from
 * src/render/pipeline/render_data.rs:166-189. */
typedef enum RtBufferId {
    RT_BUF_LIGHTING_RGBA16 = 0, /* binding 5, R16G16B16A16_UNORM: vec4(light,1)/16            8 B/px */
    RT_BUF_DEPTH_R16UI     = 1, /* binding 8, R16_UINT: uint(|origin-pos|*32) or 0xFFFF       2 B/px */
    RT_BUF_NORMAL_R8UI     = 2, /* binding 7, R8_UINT: face id 0..5 or 16                     1 B/px */
    RT_BUF_ALBEDO_RGBA8    = 3, /* binding 2, RGBA8_UNORM                                     4 B/px */
    RT_BUF_EMISSION_RGBA8  = 4, /* binding 3, RGBA8_UNORM                                     4 B/px */
    RT_BUF_FOG_RGBA8       = 5, /* binding 4, RGBA8_UNORM: sky(dir, no sun)/2                 4 B/px */
    RT_BUF_LIGHTING_F32    = 6, /* the vec4 handed to imageStore before UNORM conversion      16 B/px */
    RT_BUF_FOG_F32         = 7, /* same for fog                                               16 B/px */
    RT_BUF_DEPTH_F32       = 8, /* |origin-pos|*32 before uint(); 65535.0 for sky             4 B/px */
    RT_BUF_FINAL_BGRA8     = 9, /* rt_finalize output = the swapchain image (finalize.comp:62): B8G8R8A8_UNORM
                                   (core_builder.rs:557-568), rows TOP-down (the shader flips Y)   4 B/px */
    RT_BUF_COUNT           = 10
} RtBufferId;

/* Exact integer counters (RT_FLAG_COUNTERS), accumulated since the last rt_reset_counters.
 * B_alg = minefield_fetches*1 + material_fetches*4 + noise_fetches*4 + pixels*23. */
typedef struct RtCounters {
    uint64_t rays;               /* trace_ray invocations (primary + shadow + diffuse)     */
    uint64_t rays_primary;
    uint64_t rays_shadow;
    uint64_t rays_diffuse;
    uint64_t iterations;         /* DDA loop iterations (raytrace.comp:113)                */
    uint64_t minefield_fetches;  /* = rays + iterations (raytrace.comp:106,137)            */
    uint64_t material_fetches;   /* = hits (raytrace.comp:150-154)                         */
    uint64_t noise_fetches;      /* noise_value + seed-base lookups (raytrace.comp:302-303,324,336) */
    uint64_t hits;
    uint64_t sky_exits;
    uint64_t limit_exits;        /* Q8: loop limit reached                                 */
    uint64_t border_fetches;     /* Q7: minefield fetch outside [0,256)^3 or NaN -> 0      */
    uint64_t pixels;             /* output pixels written (x frames)                       */
    uint64_t frames;
} RtCounters;

/* HIP-event timings, milliseconds, of a context created with a timing flag (all zero without: an event between two launches is
 * 4-5 us of GPU idle time).  RT_FLAG_TIMING: trace_ms / trace_launches.  RT_FLAG_TIMING_ALL: shade_ms / other_launches and
 * frame_ms (the last rt_draw_frame, first launch to last) too.  The per-launch sums cover every frame drawn since the previous
 * rt_get_timing call. */
typedef struct RtTiming {
    float    frame_ms;        /* whole frame on the context's stream                      */
    float    trace_ms;        /* sum of traversal-kernel launches                         */
    float    shade_ms;        /* sum of ray-gen / shade / resolve launches                */
    uint32_t trace_launches;
    uint32_t other_launches;
    uint64_t rays_traced;     /* rays pushed through the traversal kernel this frame      */
} RtTiming;

typedef struct RtContext RtContext;

/* What a context allocated (no reference counterpart: Vulkan reports this through the allocator's own statistics). */
typedef struct RtInfo {
    uint32_t struct_size;               /* = sizeof(RtInfo), set by the caller                                              */
    int32_t  num_cus;                   /* CUs the persistent kernels launch on (RT_RESERVE_CUS subtracted)                 */
    uint32_t samples_per_launch;        /* samples of every pixel one path-kernel launch covers (spp / this = launches)     */
    uint16_t launches_in_flight;        /* (ABI 1.2; was reserved = 0) path launches the context keeps in flight: 2 = its launches
                                           alternate between two streams (sample batches of a frame; frames too with
                                           RT_FLAG_FRAMES_IN_FLIGHT_2), 1 otherwise                                          */
    uint16_t frames_in_flight;          /* (ABI 1.2) frame slots: 2 with RT_FLAG_FRAMES_IN_FLIGHT_2                          */
    uint64_t light_record_budget_bytes; /* what the per-path light records were sized for, all launches in flight together:
                                           min(default, free / 10) or RT_PERSIST_LIGHT_GIB                                  */
    uint64_t light_record_bytes;        /* ... and what they take (all launches in flight)                                  */
    uint64_t device_bytes;              /* all device memory the context holds                                             */
} RtInfo;

/* render::create_instance (src/render/mod.rs:36-43) + Pipeline::new (pipeline.rs:36-76):
 * create device resources for one GPU. *out is NULL on failure; rt_last_error(NULL) explains. */
int rt_create(const RtConfig* cfg, RtContext** out);

/* impl Drop for Pipeline (pipeline.rs:258-277): wait idle, free everything. NULL is a no-op. */
void rt_destroy(RtContext* ctx);

/* Message for the last failure on this context (or the last rt_create failure on this thread
 * when ctx is NULL). Never NULL. */
const char* rt_last_error(RtContext* ctx);

/* RenderData::initialize -> full-region upload (render_data.rs:269-301; formats :54-108).
 * materials: u32[R^3], minefield: u8[R^3] (R = cfg.region, 256 in the reference), both x-fastest (util.rs:104-106),
 * texel = world + R/2 (render_data.rs:221-236). The library re-tiles into 4^3 bricks on the device. */
int rt_upload_world(RtContext* ctx, const uint32_t* materials, const uint8_t* minefield);

/* TerrainUploadManager::upload_slice (terrain_upload.rs:84-275) -> vkCmdCopyBufferToImage with an
 * offset (command_buffer.rs:262-298): replace one 16-thick slab of the region.  axis 0/1/2 = x/y/z;
 * texel_offset (multiple of 16, < 256) is the slab's start along that axis; the data is a dense box of
 * extent (16,R,R) / (R,16,R) / (R,R,16), x fastest (terrain_upload.rs:96-100).  Only the slab is re-tiled on the device (one
 * launch over its 16 R^2 voxels + the nibble-map words it touches); any region size.
 * Asynchronous: the slab is copied into pinned staging (the host's buffers are free again at return), transferred on the
 * library's upload stream and applied on the context's stream after the frames already submitted — the call does not wait
 * for them (the reference does: vkQueueWaitIdle, pipeline.rs:181-189).  There are two staging sets, used in turn: the call
 * waits (on the host) only until the slab BEFORE LAST has left its pinned buffer, and that slab's transfer waited only for the
 * re-tile of the one two before it — a host that uploads one slab per frame with one or two frames in flight never waits for
 * a frame; three slabs back to back behind a long frame do wait for it.  Without RT_FLAG_TRUSTED_WORLD the minefield
 * is checked first, on the host (values above 30 -> RT_ERR_INVALID_ARG); a rejected slab is NOT applied: the region and
 * what can be drawn stay as they were.
 * Accumulation: a slab resets RT_FLAG_ACCUMULATE's running sum — except on an RT_FLAG_REPROJECT context with
 * RtConfig.stream_history = 1, where an accepted slab keeps the history and takes a pending slot for the next frame instead (two
 * more launches per slab, each reading the slab's 16 R^2 minefield bytes) and a rejected one leaves history and slots alone. */
int rt_upload_slice(RtContext* ctx, int axis, int texel_offset,
                    const uint32_t* materials, const uint8_t* minefield);

/* The upload buffers of TerrainUploadManager::new (terrain_upload.rs:65-82) are host-visible mapped Vulkan buffers the CPU
 * fills in place; this is their counterpart: pinned host memory for ONE slab (u32[16 R^2] materials, u8[16 R^2] minefield) —
 * the staging set the NEXT rt_upload_slice will use (there are two, used in turn, so the pointers alternate from slab to slab:
 * ask again for every slab).  A host that assembles its slab there and hands these very pointers to rt_upload_slice saves the
 * copy into the staging buffer.  The memory is the host's to write from the return of this call until that rt_upload_slice
 * (the call waits until the slab before last has left the buffer); it must not be touched afterwards and is freed by rt_destroy. */
int rt_slice_staging(RtContext* ctx, uint32_t** materials, uint8_t** minefield);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Sparse voxel edits: a game that places and breaks blocks.  One
 * record per edited voxel, 16 bytes: */
typedef struct RtVoxelEdit {
    uint16_t x, y, z;             /* texel coordinates, < R (the space of rt_upload_slice's texel_offset: texel = world + R/2)  */
    uint16_t solid;               /* 1: the voxel is occupied (minefield 0); 0: air (any other non-zero value counts as 1)      */
    uint32_t material;            /* packed material word written to the voxel as is                                            */
    uint32_t reserved;            /* must be 0                                                                                  */
} RtVoxelEdit;
/* rt_edit_voxels — change `count` voxels of the resident region (the reference has no editing: it repacks whole chunks,
 * src/world/chunk.rs:125-184, and uploads slabs).
 *   Materials: each edited voxel gets the edit's `material` word.  Duplicates within one call are resolved by batch order: the
 *     last edit of a voxel wins.  No other material word changes.
 *   Minefield: each 64^3 chunk (texel-aligned) that holds at least one edit gets its whole minefield rebuilt with pack_into's
 *     rule.  Occupancy of an edited voxel is its `solid` field; for every other voxel it is "current minefield value == 0", the
 *     shader's hit test (raytrace.comp:146).  An occupied voxel gets 0; any other voxel gets the first level L in 1..6 whose
 *     aligned 2^L cube inside the chunk is occupied; a chunk with nothing occupied gets 6 everywhere.  Chunks without an edit are
 *     not touched: on a world that was not built by pack_into (arbitrary minefield values 0..30) the edited chunks become
 *     pack_into-consistent and the other chunks keep their values.
 *   Nibble maps: the coarse and (R > 256) brick nibble-map words that cover the touched chunks are rebuilt; the other words stay.
 *   Validation: everything is checked on the host before anything is enqueued.  A coordinate >= R, reserved != 0 or count > 2^24
 *     returns RT_ERR_INVALID_ARG and changes nothing.  No world resident (rt_upload_world not called): RT_ERR_NOT_READY.
 *     count == 0 is a no-op (edits may then be NULL) and does not reset the accumulation.
 *   Ordering: asynchronous and stream-ordered like rt_upload_slice.  Frames already submitted read the old region; later frames,
 *     on every lane and frame slot and on a stream set with rt_set_stream, read the new one.  Edits and slabs apply in call order.
 *     The caller's array is free once the call returns: the binned batch is staged in pinned memory (two staging sets used in
 *     turn, grown when a batch needs more; the call waits on the host only until the batch before last has left its set).
 *   Accumulation: a call with count > 0 resets RT_FLAG_ACCUMULATE's running sum, as the uploads do — except on an RT_FLAG_REPROJECT
 *     context with RtConfig.edit_radius > 0, which keeps its history and records the edited boxes for the next frame instead.
 * Device work per call: one launch that scatters the material words and rebuilds the touched chunks (one workgroup per chunk), one
 * that rebuilds their nibble-map words (counted by RT_FLAG_TIMING_ALL). */
int rt_edit_voxels(RtContext* ctx, const RtVoxelEdit* edits, uint32_t count);

/* (ABI 1.3, additive; hosts detect the feature by the rt_edit_shapes symbol) Shape edits: boxes and spheres filled, painted or
 * carved on the device — an explosion, a build tool, a brush.  A shape is 32 bytes whatever its volume: */
#define RT_SHAPE_BOX    0
#define RT_SHAPE_SPHERE 1
#define RT_WHERE_ALL    0   /* every voxel of the shape is selected                   */
#define RT_WHERE_SOLID  1   /* only voxels that are occupied at that moment (paint)   */
#define RT_WHERE_AIR    2   /* only voxels that are not (fill without overwriting)    */
typedef struct RtShapeEdit {      /* 32 bytes */
    int32_t  a[3];      /*  0  BOX: low corner, texels, inclusive.  SPHERE: twice the centre, in half texels */
    uint32_t material;  /* 12  written as is to every selected voxel                                        */
    int32_t  b[3];      /* 16  BOX: high corner, inclusive.  SPHERE: b[0] = (2 r)^2, b[1] = b[2] = 0         */
    uint8_t  kind, where, solid, reserved;   /* 28  solid: 0 air, non-zero occupied; reserved must be 0     */
} RtShapeEdit;
/* rt_edit_shapes — apply `count` shapes to the resident region, in batch order, each to the world the previous one left.  All of
 * it is integer arithmetic, so the result is exact.
 *   Coordinates: texels, the space of RtVoxelEdit; a voxel's centre in half texels is 2 x + 1.
 *   Membership: BOX a[k] <= x_k <= b[k] on every axis; SPHERE sum_k (2 x_k + 1 - a[k])^2 <= b[0] (radius 3.5 round voxel
 *     (10, 10, 10): a = (21, 21, 21), b[0] = 49; with b[0] = 0 an odd `a` selects one voxel and an even `a` none).
 *   Clipping: a shape may reach or lie outside [0, R)^3; only its voxels inside count.  A host applies a shape that crosses the
 *     window's seam by issuing it again shifted by +-R texels (+-2 R in `a` of a sphere).  The shape's BOUNDING BOX is, per axis,
 *     the texels of [0, R) that pass that axis's own test (a box's range; a sphere's (2 x + 1 - a[k])^2 <= b[0]); a shape whose
 *     bounding box is empty on an axis does nothing.
 *   Selection: `where` narrows the shape to the voxels that are occupied (minefield 0) or not at that moment, earlier shapes of
 *     the call included.  A selected voxel gets `material` and its occupancy becomes `solid`; any other voxel keeps both.
 *   Touched chunks: every 64^3 chunk that meets the bounding box of at least one shape — whether or not a voxel of it is
 *     selected — gets its whole minefield rebuilt by rt_edit_voxels' rule and its nibble-map words rebuilt; every other chunk
 *     keeps its bytes.  In a chunk that holds a selected voxel the result equals rt_edit_voxels with one record per selected
 *     voxel in shape order.
 *   Validation: on the host, before anything is enqueued; a rejected call changes nothing.  RT_ERR_INVALID_ARG: count > 4096; a
 *     NULL pointer with count > 0; kind > 1, where > 2 or reserved != 0; an a[k] or a box's b[k] outside [-4 R, 4 R]; a box with
 *     a[k] > b[k]; a sphere with b[0] outside [0, 2^26] or b[1], b[2] != 0 (the sphere's sum then stays below 2^27).  No world
 *     resident: RT_ERR_NOT_READY.  count == 0, or a call that touches no chunk: RT_OK, nothing is enqueued or reset.
 *   Ordering, staging, accumulation: rt_edit_voxels' — stream-ordered after the frames and queries already submitted and before
 *     later ones, also under rt_set_stream; the same two staging sets, so that shapes, voxel edits and slabs apply in call order.
 *     A call that touches a chunk resets RT_FLAG_ACCUMULATE's sum — except with RtConfig.edit_radius > 0, where it records one
 *     pending box per shape that has a bounding box (that box, in shape order; at most 16 wait, rt_edit_boxes_pending).
 * Device work per call: one launch that applies the shapes and rebuilds the touched chunks (one workgroup per chunk; only the
 * shape records and the chunk list travel), one that rebuilds their nibble-map words (counted by RT_FLAG_TIMING_ALL). */
int rt_edit_shapes(RtContext* ctx, const RtShapeEdit* shapes, uint32_t count);

/* (ABI 1.3, additive; hosts detect the feature by the rt_edit_stamps symbol) Voxel stamps: a STAMP is a dense box of voxels with
 * their own materials that lives in device memory of a context — a tree, a house, a schematic, a moving platform, the undo of an
 * explosion — created from host arrays or captured from the resident region, and pasted anywhere, turned or mirrored, from 32
 * bytes per placement.  Its extent is E = (ex, ey, ez), each 1..256; per voxel it holds a packed material word and a state: */
#define RT_STAMP_ABSENT 0          /* not part of the stamp: the world keeps what it has                         */
#define RT_STAMP_AIR    1          /* the placed voxel becomes unoccupied                                        */
#define RT_STAMP_SOLID  2          /* the placed voxel becomes occupied (minefield 0)                            */
#define RT_STAMP_SKIP_AIR 0x1u     /* rt_stamp_capture: unoccupied voxels become ABSENT, not AIR */
/*   Layout: `materials` and `state` are [ez][ey][ex], x fastest.  The material word of an ABSENT voxel is ignored, and
 *     rt_stamp_read returns it as 0.  All of it is integer arithmetic, so results are exact.
 *   Ids: non-zero; an id is valid from the call that returned it until rt_stamp_destroy.  Any other id is RT_ERR_INVALID_ARG in
 *     every call.  At most 1024 live stamps per context: one more returns RT_ERR_INVALID_ARG.  Stamps belong to their context.
 * rt_stamp_create — a stamp from host arrays.  The call returns when the stamp is on the device, so the caller's arrays are free
 *   again.  RT_ERR_INVALID_ARG: an extent outside 1..256, a state above 2, or a NULL pointer.  RT_ERR_OOM: the stamp cannot be
 *   allocated.  (It needs no resident world.)
 * rt_stamp_capture — a stamp from the texel box [lo, lo + extent) of the resident region, device to device, without a host round
 *   trip: one launch.  The box must lie inside [0, R)^3 with extents 1..256; anything else (an unknown flag bit included) is
 *   RT_ERR_INVALID_ARG.  No resident world: RT_ERR_NOT_READY.  It is stream-ordered like the edits: it sees every earlier upload,
 *   edit, shape, stamp, slab and generated region, and later world changes do not disturb it.  A voxel is SOLID iff its minefield
 *   byte is 0; otherwise it is AIR, or ABSENT with RT_STAMP_SKIP_AIR.  The material word is the voxel's (0 where ABSENT).  It
 *   changes nothing the renderer reads: no accumulation reset, no pending box, no prepass dropped.
 * rt_stamp_info — the extent.  rt_stamp_read — the stamp's arrays back to the host (either may be NULL; synchronises).
 * rt_stamp_destroy — placements already enqueued still read the stamp; the call may wait for them.  RtInfo.device_bytes counts
 *   live stamps; rt_destroy frees the rest. */
int rt_stamp_create (RtContext* ctx, const int32_t extent[3], const uint32_t* materials, const uint8_t* state, uint32_t* id_out);
int rt_stamp_capture(RtContext* ctx, const int32_t lo[3], const int32_t extent[3], uint32_t flags, uint32_t* id_out);
int rt_stamp_info   (RtContext* ctx, uint32_t id, int32_t extent_out[3]);
int rt_stamp_read   (RtContext* ctx, uint32_t id, uint32_t* materials, uint8_t* state);   /* either may be NULL; synchronises */
int rt_stamp_destroy(RtContext* ctx, uint32_t id);

typedef struct RtStampPlace {      /* 32 bytes */
    int32_t  at[3];                /*  0  texel of the low corner of the placed (oriented) box; RtVoxelEdit's space */
    uint32_t stamp;                /* 12  id */
    uint8_t  orient, where, reserved0[2];   /* 16  orient 0..47; where = RT_WHERE_ALL / SOLID / AIR */
    uint32_t reserved[3];          /* 20  must be 0 */
} RtStampPlace;
/* rt_edit_stamps — paste `count` placements into the resident region, in batch order, each to the world the previous one left.
 *   Orientation: orient = p << 3 | f.  p in 0..5 selects perm: (0,1,2), (0,2,1), (1,0,2), (1,2,0), (2,0,1), (2,1,0): world axis k
 *     of the placed box is stamp axis perm[k].  Bit j of f flips stamp axis j.  The placed extent is E'_k = E[perm[k]].
 *     Placed-local cell d (0 <= d_k < E'_k) lies at world texel at + d and shows stamp voxel s, with
 *     s[perm[k]] = (f >> perm[k]) & 1 ? E[perm[k]] - 1 - d_k : d_k.  orient >= 48 is invalid.  An orientation is a proper rotation
 *     iff the permutation's parity plus the number of flips is even; the other 24 mirror.
 *   Placement: the BOUNDING BOX of a placement is [at, at + E') clipped to [0, R)^3; a placement whose box is empty does nothing.
 *     A host reissues a placement shifted by +-R when it crosses the window's seam.  Selected voxels are those of the box whose
 *     stamp voxel is not ABSENT; `where` narrows them to world voxels occupied (minefield 0) or not at that moment, earlier
 *     placements of the call included.  A selected voxel gets the stamp's material word and its occupancy becomes
 *     state == SOLID; any other voxel keeps both.
 *   Touched chunks: every 64^3 chunk that meets the bounding box of at least one placement — whether or not a voxel of it is
 *     selected — gets its whole minefield rebuilt by rt_edit_voxels' rule and its nibble-map words rebuilt; every other chunk
 *     keeps its bytes.  In a chunk that holds a selected voxel the result equals rt_edit_voxels with one record per selected
 *     voxel in placement order.
 *   Validation: on the host, before anything is enqueued; a rejected call changes nothing.  RT_ERR_INVALID_ARG: count > 4096; a
 *     NULL pointer with count > 0; an unknown id; orient >= 48; where > 2; a non-zero reserved byte or word; an at[k] outside
 *     [-4 R, 4 R].  No world resident: RT_ERR_NOT_READY.  count == 0, or a call that touches no chunk: RT_OK, nothing is enqueued
 *     or reset.
 *   Ordering, staging, accumulation: rt_edit_voxels' — stream-ordered after the frames and queries already submitted and before
 *     later ones, also under rt_set_stream; the same two staging sets, so that stamps, shapes, voxel edits and slabs apply in call
 *     order.  A call that touches a chunk resets RT_FLAG_ACCUMULATE's sum — except with RtConfig.edit_radius > 0, where it records
 *     one pending box per placement that has a bounding box (that box, in placement order; at most 16 wait,
 *     rt_edit_boxes_pending; an overflow empties the set).
 *   Undo: capture a box with flags 0, change the world inside it by any of the edit calls, place the stamp at `lo` with orient 0
 *     and RT_WHERE_ALL: every material word and every voxel's occupancy in the box is then what it was (on a world built by
 *     pack_into the touched chunks' minefield bytes and all nibble-map words are too).
 * Device work per call: one launch that applies the placements and rebuilds the touched chunks (one workgroup per chunk; only
 * a 64-byte record per placement and the chunk list travel), one that rebuilds their nibble-map words (counted by
 * RT_FLAG_TIMING_ALL). */
int rt_edit_stamps(RtContext* ctx, const RtStampPlace* places, uint32_t count);
/* Un-tile the box [x0, x0 + ex) x [y0, y0 + ey) x [z0, z0 + ez) of the resident region (texel coordinates) into the caller's layout:
 * materials u32[ex ey ez], minefield u8[ex ey ez], x fastest; either pointer may be NULL.  Waits for everything submitted before
 * (the region as the next frame would see it), then synchronises.  A box outside the region (or an extent < 1) returns
 * RT_ERR_INVALID_ARG; no world resident: RT_ERR_NOT_READY.  For tests and for a host that saves an edited world. */
int rt_read_box(RtContext* ctx, int x0, int y0, int z0, int ex, int ey, int ez, uint32_t* materials, uint8_t* minefield);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Ray queries against the resident region: what a ray hits, for
 * picking the block under the cursor (then rt_edit_voxels), line of sight and light probes (a body with a volume moves by
 * rt_sweep_boxes: a ray tunnels through corners).  One ray, 32 bytes: */
typedef struct RtRay {
    float origin[3];     uint32_t reserved0;   /* reserved words are ignored                                                  */
    float direction[3];  uint32_t reserved1;   /* need not be normalized: trace_ray normalizes it (raytrace.comp:83)          */
} RtRay;
#define RT_HIT_AIR   0   /* left the region (raytrace.comp:138-145)                                                        */
#define RT_HIT_SOLID 1   /* a texel whose minefield value is 0 (:146-160), or the border value 0 of a fetch outside the texture */
#define RT_HIT_LIMIT 2   /* the loop ran out (:109; Q8)                                                                    */
/* One hit, 48 bytes: */
typedef struct RtRayHit {
    float    position[3];    /*  0  as trace_ray returns it: after the 0.001 offset off the face (:166-180)                   */
    float    distance;       /* 12  length(origin - position before the offset) (:164)                                       */
    int32_t  texel[3];       /* 16  texel whose material word was fetched (:150-154), the space of RtVoxelEdit; -1,-1,-1 for
                                    air, limit exits and fetches that fell outside the texture (border value, NaN positions)  */
    uint32_t material;       /* 28  packed material word (0 for air, limit and border)                                       */
    uint32_t normal;         /* 32  the shader's normal code 0..5 of the last face crossed (:89-93)                          */
    uint32_t kind;           /* 36  RT_HIT_AIR / RT_HIT_SOLID / RT_HIT_LIMIT                                                 */
    uint32_t iterations;     /* 40  loop iterations (:113)                                                                   */
    uint32_t border_fetches; /* 44  minefield fetches outside [0,R)^3 or at NaN (Q7)                                          */
} RtRayHit;
/* Contract of the three calls:
 *   Results: every field equals the CPU oracle's trace_ray with the same `lr` and region, bit for bit (NaN positions and
 *     distances of rays that never moved are NaN).  `lr` is the uniform block's lr (raytrace.comp:104): the window of world
 *     coordinates the region covers is lr - R/2 .. lr + R/2.
 *   Which world: a query sees the region as left by every earlier rt_upload_world, rt_upload_slice and rt_edit_voxels on the
 *     context; later calls do not disturb it (an edit after rt_trace_rays_async waits on the device for the query).
 *   No waiting on frames: a query is not ordered after frames drawn before it unless a world change sits between them (queries
 *     run on a stream of their own, at the device's highest priority; a frame kernel that occupies every CU still delays its start
 *     until CUs free up — DESIGN.md "Ray queries").  After rt_set_stream(non-NULL) everything runs on the caller's stream, in order.
 *   No side effects: no output plane, accumulation sum or count, RtCounters or RtTiming changes.
 *   Errors: no world resident: RT_ERR_NOT_READY (no noise needed).  A NULL pointer with count > 0, count > 2^26 or a pixel
 *     outside width x height: RT_ERR_INVALID_ARG, checked before anything is enqueued.  count == 0: RT_OK, nothing enqueued.
 *   Tile contexts (tile_world > 1) answer for whole-frame pixels: they hold the whole region.  Every RtKernel answers the same.
 *   Device work per call: one launch, one lane per ray (DESIGN.md "Ray queries"); the synchronous calls add a transfer each way.
 * Arbitrary rays; host pointers; returns when the hits are in host memory. */
int rt_trace_rays(RtContext* ctx, const RtRay* rays, uint32_t count, const int32_t lr[3], RtRayHit* hits);
/* Same with device pointers, enqueued: the hits are valid after rt_sync (or, after rt_set_stream, in the caller's stream order).
 * Both pointers must be 16-byte aligned memory of the context's device (hipMalloc) or managed memory; anything else (a host
 * address, another device's memory, a misaligned pointer) returns RT_ERR_INVALID_ARG before anything is enqueued.  The rays must
 * be complete on the device when the call is made: the query runs on the library's query stream, which is ordered after neither
 * the caller's streams nor the frames — unless rt_set_stream gave the caller's stream, where stream order holds.  The hits buffer
 * must not be read or reused before rt_sync (or the caller's stream) says the query is done. */
int rt_trace_rays_async(RtContext* ctx, const RtRay* rays_dev, uint32_t count, const int32_t lr[3], RtRayHit* hits_dev);
/* Primary rays of whole-frame pixels xy[2 i], xy[2 i + 1] = (x, y), row 0 = the bottom row, of the camera in `u`
 * (raytrace.comp:296-297,306-315, including the move of a start below the region).  Only origin, forward, up, right and lr of `u`
 * are read.  Host pointers, synchronous. */
int rt_pick_pixels(RtContext* ctx, const RtUniforms* u, const int32_t* xy, uint32_t count, RtRayHit* hits);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Light probes: path-traced light at arbitrary points of the resident
 * region — what lights an entity, a particle, a held item or an irradiance grid, and "is this spot in the sun?".  The whole light
 * loop of the shader's non-air branch (raytrace.comp:317-350: shadow ray, diffuse bounce, sky, albedo chain, noise addressing) runs
 * on the device, `samples` times per probe.  One probe, 32 bytes: */
#define RT_PROBE_SPHERE 6          /* normal code: no hemisphere offset (the fall-through of diffuse_direction, raytrace.comp:198-210) */
typedef struct RtLightProbe {
    float    position[3];          /*  0  where light is gathered: a point just off a surface, e.g. RtRayHit.position as returned      */
    uint32_t normal;               /* 12  0..5: the shader's face code (RtRayHit.normal); RT_PROBE_SPHERE: whole sphere; else INVALID_ARG */
    uint16_t cell[2];              /* 16  noise cell: plays gl_WorkGroupID.xy in noise_offset (raytrace.comp:304)                       */
    uint32_t reserved[3];          /* 20  must be 0                                                                                     */
} RtLightProbe;
/* One result, 16 bytes: */
typedef struct RtProbeLight {
    float    light[3];             /*  0  the shader's `light` of a non-air primary (raytrace.comp:323-349), mean over the samples      */
    uint32_t sun_samples;          /* 12  samples whose level-1 shadow ray left the region (sun1.air): exact; / samples = sun visibility */
} RtProbeLight;
/* Contract of the two calls:
 *   Inputs read from `u`: sun_angle, seed and lr only (the camera fields play no part: there is no primary ray).
 *   Per sample: sample s of a probe is the non-air branch of the shader's main with the surface {position, normal}:
 *     seed_s = (seed + s) mod RT_NOISE_BYTES, noise_offset = base(seed_s) + cell * 8 (:298-304 with cell in place of gl_WorkGroupID.xy),
 *     then per level j = 1..depth the noise value of the level (:324, :336: + (j - 1) * 2 / 512), the shadow ray (trace_sun, :185-187)
 *     and the diffuse ray (diffuse_direction, :189-212) from the surface, the diffuse ray's hit being the surface of level j + 1; the
 *     path ends when a diffuse ray leaves the region (sample_sky of its direction) or at level `depth`, and the light is unwound
 *     innermost first with the albedo of each surface (light2 *= albedo2; light2 += emission; light += light2) — the loop RtConfig.depth
 *     generalises for frames, in the same fp32 operation order.  A probe whose normal is RT_PROBE_SPHERE draws its first diffuse
 *     direction from the whole sphere (diffuse_direction without the +-1 offset); deeper levels use the face their ray hit.
 *   Sum: the samples' lights are added in order s = 0 .. samples - 1 in fp32 starting from 0, light = sum / (float)samples per channel.
 *     The order does not depend on count, on the probe's place in the batch or on how the library splits a call into launches:
 *     equal probes give equal results, bit for bit.
 *   Identity with frames (what the feature means): take a pixel (px, py) whose primary ray hits, a probe with position / normal of
 *     that hit as rt_pick_pixels returns them and cell = (wg(px), wg(py)), wg(p) = (p / 128) * 16 + p % 16 (the workgroup that owns the
 *     coordinate, raytrace.comp:291-294).  Then light / 16 is bitwise equal to the .rgb of RT_BUF_LIGHTING_F32 of that pixel in a frame
 *     drawn with the same u, RtConfig.spp = samples and RtConfig.depth = depth (the division by RT_LIGHTING_SCALE is exact).
 *   Any position is legal: what trace_ray does from inside a solid voxel, outside the window or at a NaN is the result (as for the
 *     ray queries).
 *   Validation, before anything is enqueued (a rejected call changes nothing): samples outside 1..4096, depth outside 1..RT_MAX_DEPTH,
 *     count x samples > 2^26, a NULL pointer with count > 0: RT_ERR_INVALID_ARG.  rt_probe_light also rejects a normal above 6 and a
 *     non-zero reserved word (RT_ERR_INVALID_ARG).  No world resident or no noise uploaded: RT_ERR_NOT_READY.  count == 0: RT_OK,
 *     nothing enqueued.
 *   Which world, ordering and side effects: exactly those of the ray queries — probes see every earlier world change and run on the
 *     query stream, not after the frames; later edits, slabs and generated terrain wait for them; after rt_set_stream(non-NULL) they
 *     run on the caller's stream, in order.  No output plane, accumulation sum or history, RtCounters or RtTiming changes.  Tile
 *     contexts, every RtKernel and every region size answer the same.
 *   Device work per call: one launch, one lane per (probe, sample) path; a probe's samples are added by one lane, inside the launch
 *     when `samples` divides 256 and in a second small launch over a scratch buffer of the context otherwise (16 bytes per path,
 *     at most 64 MiB, grown on demand and counted in RtInfo.device_bytes; larger calls run as several launches of whole probes).
 *     DESIGN.md "Light probes".
 * Host pointers; returns when the results are in host memory. */
int rt_probe_light(RtContext* ctx, const RtUniforms* u, const RtLightProbe* probes, uint32_t count, uint32_t samples, int32_t depth,
                   RtProbeLight* out);
/* Same with device pointers, enqueued: `out_dev` is valid after rt_sync (or, after rt_set_stream, in the caller's stream order).  Both
 * pointers must pass rt_trace_rays_async's test (16-byte aligned memory of the context's device, or managed memory), else
 * RT_ERR_INVALID_ARG before anything is enqueued; the probes must be complete on the device when the call is made.  The library
 * cannot read device records on the host: here a normal above 6 is handled on the device as RT_PROBE_SPHERE and the reserved words
 * are ignored. */
int rt_probe_light_async(RtContext* ctx, const RtUniforms* u, const RtLightProbe* probes_dev, uint32_t count, uint32_t samples,
                         int32_t depth, RtProbeLight* out_dev);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Box sweeps: an axis-aligned box moved through the resident region until
 * it meets an occupied voxel — what moves a player, an entity or a particle through the world without passing through it (the
 * reference's camera flies through terrain: src/game/mod.rs:89-95).  A ray has no volume; a box swept by these rules neither tunnels
 * through corners nor catches on faces it only touches.  One sweep, 48 bytes: */
typedef struct RtBoxSweep {      /* 48 bytes */
    float lo[3];     uint32_t reserved0;   /* world coordinates of the box's low corner  */
    float hi[3];     uint32_t reserved1;   /* ... and high corner                        */
    float motion[3]; uint32_t reserved2;   /* displacement over the sweep                */
} RtBoxSweep;                    /* the reserved words are ignored */
#define RT_SWEEP_FREE     0   /* travelled the whole motion                        */
#define RT_SWEEP_BLOCKED  1   /* stopped against an occupied voxel at fraction t   */
#define RT_SWEEP_EMBEDDED 2   /* overlaps an occupied voxel before moving          */
#define RT_SWEEP_INVALID  3   /* async only: record outside the validated domain   */
/* One hit, 64 bytes: */
typedef struct RtSweepHit {      /* 64 bytes */
    float    t;  uint32_t kind;  uint32_t normal;  uint32_t material;   /*  0  fraction of the motion travelled; RT_SWEEP_*; face code    */
    int32_t  texel[3];           uint32_t axis;      /* 16  blocking / embedding texel (RtVoxelEdit's space); blocked axis 0..2, else 3 */
    float    lo[3];              uint32_t reserved0; /* 32  the box where the sweep ended: the next sweep's box                         */
    float    hi[3];              uint32_t reserved1; /* 48  (the reserved words are written as 0)                                       */
} RtSweepHit;
/* The rules.  All float arithmetic is fp32 with one rounding per operation; once the event times are known everything is integers.
 * Results are reproduced bit for bit by tests/sweep_ref.py (DESIGN.md "Box sweeps").
 *   Occupancy: world voxel v (the cell [v, v + 1) per axis) is occupied iff lr - R/2 <= v < lr + R/2 on every axis and the minefield
 *     byte at texel (v + R/2) mod R (Euclidean; the addressing of rt_upload_slice / rt_generate_*) is 0.  Outside the window is air.
 *   Cells of a box: per axis the closed integer range c = [floor(lo), ceil(hi) - 1]: a box that touches a face does not overlap the
 *     cell behind it (a box resting on a floor whose top is z = 10 has lo_z = 10.0 and does not include cell 9).
 *   Embedded: if a cell of c_x x c_y x c_z is occupied: kind EMBEDDED, t = 0, axis = 3, normal = 6, lo / hi = the inputs, texel /
 *     material of the first such voxel in ascending (z, y, x) order.
 *   Events: on every axis a with motion != 0 the leading face (hi moving +, lo moving -) and the trailing face cross integer planes g
 *     at t = (float(g) - face) / motion (one subtraction, one IEEE division); only events with t < 1 exist.  Moving +: leading planes
 *     g = ceil(hi), ceil(hi) + 1, ... enter cell layer g; trailing planes g = floor(lo) + 1, ... set c.lo = g.  Moving -: leading planes
 *     g = floor(lo), floor(lo) - 1, ... enter layer g - 1; trailing planes g = ceil(hi) - 1, ... set c.hi = g - 1.  Order: ascending t
 *     compared as floats; at equal t trailing before leading; then axis x, y, z.  A leading event tests its layer against the current
 *     ranges of the other two axes: an occupied cell gives kind BLOCKED, t = the event's, axis = a, texel / material of the first
 *     occupied cell in (z, y, x) order, normal = the code rt_trace_rays reports for a ray travelling along a in the motion's direction
 *     (2 a + 1 moving +, 2 a moving -); otherwise the layer joins c.  No event left: kind FREE, t = 1, axis = 3, normal = 6, texel
 *     (-1, -1, -1), material 0.
 *   Returned box, per moving axis: lo' = max(lo + motion * t, float(c.lo)), hi' = min(hi + motion * t, float(c.hi + 1)); on the blocked
 *     axis, with size = hi - lo: moving + hi' = float(g), lo' = max(g - size, float(c.lo)); moving - lo' = float(g), hi' =
 *     min(g + size, float(c.hi + 1)).  max / min keep the moved face unless it lies beyond the clamp.  An axis with motion == 0 returns
 *     its input bits.  The clamps close the contract: the returned box, swept again on an unchanged world, is never EMBEDDED (its
 *     cells are cells this sweep found free).
 *   Validated domain: every float finite; |lo|, |hi| <= 2^22; per axis 0 < hi - lo <= 8 (the fp32 difference); |motion| <= 64 per
 *     component.  rt_sweep_boxes checks every record on the host before anything is enqueued (RT_ERR_INVALID_ARG; a rejected call
 *     changes nothing, `hits` included).  rt_sweep_boxes_async cannot read its records on the host: the device gives a record outside
 *     the domain kind = RT_SWEEP_INVALID, t = 0, axis = 3, normal = 6, texel (-1, -1, -1), material 0, lo / hi = the input bits, and
 *     fetches no voxel for it.
 *   Errors: no world resident: RT_ERR_NOT_READY.  A NULL pointer with count > 0 or count > 2^24: RT_ERR_INVALID_ARG.  count == 0: RT_OK,
 *     nothing enqueued.
 *   Which world, ordering and side effects: exactly those of the ray queries — sweeps see every earlier upload, edit, slab and
 *     generated region and run on the query stream, not after the frames; later world changes wait for them; after
 *     rt_set_stream(non-NULL) they run on the caller's stream, in order.  No output plane, accumulation sum or history, RtCounters or
 *     RtTiming changes.  Tile contexts, every RtKernel and every region size answer the same.
 *   Device work per call: one launch, one lane per sweep (DESIGN.md "Box sweeps"); the synchronous call adds a transfer each way.
 * Host pointers; returns when the hits are in host memory. */
int rt_sweep_boxes(RtContext* ctx, const RtBoxSweep* sweeps, uint32_t count, const int32_t lr[3], RtSweepHit* hits);
/* Same with device pointers, enqueued: the hits are valid after rt_sync (or, after rt_set_stream, in the caller's stream order).  Both
 * pointers must pass rt_trace_rays_async's test (16-byte aligned memory of the context's device, or managed memory), else
 * RT_ERR_INVALID_ARG before anything is enqueued; the sweeps must be complete on the device when the call is made. */
int rt_sweep_boxes_async(RtContext* ctx, const RtBoxSweep* sweeps_dev, uint32_t count, const int32_t lr[3], RtSweepHit* hits_dev);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Entity boxes: world-space axis-aligned boxes — a player model, mobs,
 * dropped items, projectiles — composited by depth into the G-buffer of the frame drawn last, after rt_draw_frame and before the
 * post passes.  A box has RtBoxSweep's shape; a drawn pixel gets the box's depth, face code, albedo and emission and the light of that
 * face as rt_probe_light computed it, so rt_denoise, rt_denoise_history and rt_finalize treat it like any other pixel.  Entities cast
 * no shadow into the world by themselves (rt_shadow_entities adds the sun's) and do not appear in bounce light; boxes are not
 * rotated.  One box, 32 bytes: */
typedef struct RtDrawBox {        /* 32 bytes */
    float    lo[3];  uint32_t material;   /* world coordinates of the low corner; packed material word: albedo decoded as a voxel's (raytrace.comp:156-158) */
    float    hi[3];  uint32_t emission;   /* high corner; RGBA8 word written as is to RT_BUF_EMISSION_RGBA8 (a voxel's is 0xFF000000) */
} RtDrawBox;
/* The rules.  All arithmetic is fp32 with one rounding per operation; fused operations appear only where rtm_fma is written.  Results
 * are reproduced bit for bit by tests/draw_boxes_ref.py, which tests every box against every pixel (DESIGN.md "Entity boxes").
 *   Inputs: only origin, forward, up and right of `u` are read, as for rt_pick_pixels; the host passes the uniforms of the frame it
 *     drew.  `face_lights` holds 6 * count records: record 6 b + n is the light of box b's face with normal code n (0..5, the codes of
 *     RtRayHit.normal); only .light is read, in the shader's unit — what rt_probe_light returns, before the division by 16.
 *   Ray of pixel (px, py), row 0 the bottom row: sx = (float(px) / float(width)) * 2 - 1, sy likewise from py and height,
 *     d = normalize(forward + right * sx + up * sy) (rt_math.h's rtm_normalize3; the products and sums in this order), o = u.origin.
 *     The shader's "start below the region" slide is not applied: the depth plane is measured from u.origin too.
 *   Valid box: every float finite, |lo_k|, |hi_k| <= 2^22 and lo_k < hi_k on every axis.  The device skips an invalid box in both
 *     calls (it is never hit); rt_draw_boxes also rejects the whole call (RT_ERR_INVALID_ARG) before anything is enqueued.
 *   Slab test of box b: for each axis k = x, y, z with d_k != 0: inv = 1.0f / d_k, t0 = (lo_k - o_k) * inv, t1 = (hi_k - o_k) * inv,
 *     tn_k = rtm_min(t0, t1), tf_k = rtm_max(t0, t1).  An axis with d_k == 0 (either sign) passes iff lo_k < o_k && o_k < hi_k and gives
 *     no bound.  t_in is the largest tn_k and the entry axis the axis that supplied it, the lowest axis on equal values: the first
 *     bounded axis starts both, a later axis k replaces them iff tn_k > t_in.  t_out is the smallest tf_k: a later axis replaces it iff
 *     tf_k < t_out.  The box is hit iff some axis gave a bound, every d_k == 0 axis passes, t_in > 0 and t_in < t_out: a camera inside
 *     a box does not see it (the player's own box never blinds them) and a grazing ray misses.  Any comparison with a NaN is false.
 *   Winner: among the boxes hit the one with the smallest t_in, on equal t_in the lowest index.
 *   Depth test: P_k = rtm_fma(d_k, t_in, o_k); depth_f = rtm_length3(o - P) * 32.0f (the G-buffer's expression, raytrace.comp:356-359).
 *     The pixel is drawn iff depth_f < RT_BUF_DEPTH_F32[pixel]: strict, the world wins ties; sky is 65535.0, so a box 2048 or more
 *     units away is never drawn.
 *   Writes of a drawn pixel (every other pixel and plane keeps its bits): RT_BUF_DEPTH_F32 = depth_f; RT_BUF_DEPTH_R16UI =
 *     rtm_f2u16(depth_f); RT_BUF_NORMAL_R8UI = 2 a + 1 if d_a > 0, else 2 a, a the entry axis (the code trace_ray gives a ray crossing
 *     that face); RT_BUF_ALBEDO_RGBA8 = the UNORM8 pack of (albedo of `material`, 1); RT_BUF_EMISSION_RGBA8 = `emission`;
 *     RT_BUF_LIGHTING_F32 and RT_BUF_LIGHTING_RGBA16 exactly what a one-sample frame stores for light = face_lights[6 b + normal].light:
 *     (light / 1.0f) / 16 per channel and 1 / 16 in alpha, and their UNORM16.  The fog planes depend on the direction only and are
 *     not touched.
 *   Which frame, ordering: the call acts on the planes of the frame drawn last, on the stream rt_denoise uses — after that frame and
 *     before later post passes, also with RT_FLAG_FRAMES_IN_FLIGHT_2 and after rt_set_stream.  On the device it waits for the queries
 *     already enqueued on the context, so rt_probe_light_async can feed rt_draw_boxes_async through a device buffer without a host
 *     sync.
 *   Side effects: the frame slot's cached prepass is dropped (a still camera does not carry entity pixels into the next frame).  No
 *     accumulation sum, RT_FLAG_REPROJECT history set or count, RtCounters, pending edit box or slab changes.
 *   Errors: NULL ctx, NULL u, a NULL array with count > 0, count > 4096: RT_ERR_INVALID_ARG.  tile_world != 1: RT_ERR_UNIMPLEMENTED
 *     (whole-frame contexts only, as for rt_denoise).  No frame drawn yet: RT_ERR_NOT_READY.  count == 0: RT_OK, nothing enqueued,
 *     no prepass dropped.  A rejected call changes nothing.
 *   Device work per call: one launch, a wave per 8x8 pixel tile; per tile the boxes pass a conservative cull 64 at a time and only
 *     the survivors are tested per pixel (DESIGN.md "Entity boxes"); the synchronous call adds one transfer.
 * Host pointers; returns when the planes are written. */
int rt_draw_boxes(RtContext* ctx, const RtUniforms* u, const RtDrawBox* boxes, const RtProbeLight* face_lights, uint32_t count);
/* Same with device pointers, enqueued.  Both pointers must pass rt_trace_rays_async's test (16-byte aligned memory of the context's
 * device, or managed memory), else RT_ERR_INVALID_ARG before anything is enqueued.  The library cannot read device records on the
 * host: an invalid box is skipped on the device. */
int rt_draw_boxes_async(RtContext* ctx, const RtUniforms* u, const RtDrawBox* boxes_dev, const RtProbeLight* face_lights_dev, uint32_t count);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Voxel-model entities: a stamp (rt_stamp_create, rt_stamp_capture)
 * drawn as an entity — a mob, a dropped block, a held tool, a door, a moving platform — at any float position, at any scale (voxels
 * smaller than the world's, 1/16 say) and in any of the 48 orientations, composited by depth into the G-buffer of the frame drawn
 * last exactly as the entity boxes are.  Each pixel walks the model's voxels and takes the albedo of the voxel it hits.  No world
 * byte, accumulation sum or history is touched: the model is not part of the world it collides with.  Entities cast no shadow into
 * the world by themselves (rt_shadow_entities adds the sun's) and do not appear in bounce light; the light is one value per
 * bounding-box face, as for boxes.  One model, 32 bytes: */
typedef struct RtDrawStamp {      /* 32 bytes */
    float    origin[3];           /*  0  world coordinates of the low corner of the placed (oriented) model            */
    float    scale;               /* 12  edge of one model voxel in world units                                         */
    uint32_t stamp;               /* 16  id of a live stamp of this context                                             */
    uint8_t  orient, reserved0[3];/* 20  orient 0..47, RtStampPlace's; reserved bytes must be 0                         */
    uint32_t emission;            /* 24  RGBA8 word written as is to RT_BUF_EMISSION_RGBA8 (a voxel's is 0xFF000000)    */
    uint32_t reserved;            /* 28  must be 0                                                                      */
} RtDrawStamp;
/* The rules.  All arithmetic is fp32 with one rounding per operation; fused operations appear only where rtm_fma is written; any
 * comparison with a NaN is false.  Results are reproduced bit for bit by tests/draw_stamps_ref.py, which walks every model for every
 * pixel (DESIGN.md "Voxel-model entities").
 *   Inputs: `u` and `face_lights` as for rt_draw_boxes: record 6 i + n is the light of the face with normal code n of model i's
 *     bounding box; only .light is read.
 *   Placed model: orient is RtStampPlace's.  The placed extent is E'_k = E[perm[k]], and placed-local cell c (0 <= c_k < E'_k) shows
 *     the stamp voxel that rt_edit_stamps' placed-local cell d = c shows.  Cell c occupies [origin_k + c_k scale, origin_k + (c_k + 1) scale]
 *     on axis k, up to the rounding of the planes below.
 *   Valid record: a live id; orient < 48; reserved0 and reserved zero; every float finite; 2^-8 <= scale <= 64; |origin_k| <= 2^22
 *     and |hi_k| <= 2^22 on every axis, hi_k = rtm_fma(float(E'_k), scale, origin_k).
 *   Ray: rt_draw_boxes' — the same sx, sy and rtm_normalize3, o = u.origin, no slide.
 *   Bounding box: lo = origin, hi as above; rt_draw_boxes' slab test unchanged gives t_in, t_out and the entry axis a.  The model is
 *     entered iff that test says hit; so a camera inside the bounding box does not see the model (a limit kept from boxes), and a
 *     grazing ray misses.
 *   Planes of axis k: plane i (0..E'_k) lies at w = rtm_fma(float(i), scale, origin_k), and the ray reaches it at
 *     t_k(i) = (w - o_k) * inv_k with the slab test's inv_k = 1.0f / d_k; planes 0 and E'_k are the bounding box's own.
 *   First cell: c_a = d_a > 0 ? 0 : E'_a - 1.  On each other axis c_k = clamp(int(rtm_floor((p - origin_k) / scale)), 0, E'_k - 1)
 *     with p = rtm_fma(d_k, t_in, o_k), or p = o_k when d_k == 0; the division is IEEE.  t = t_in, axis = a.
 *   Walk: repeat — (1) if the stamp voxel shown by cell c has state RT_STAMP_SOLID, stop: a hit at t through `axis`; RT_STAMP_AIR and
 *     RT_STAMP_ABSENT are both see-through.  (2) Otherwise, over the axes with d_k != 0 in the order x, y, z, tk = t_k(d_k > 0 ?
 *     c_k + 1 : c_k); the first such axis starts the minimum, a later one replaces it iff its tk < the minimum, so the lowest axis
 *     wins ties.  (3) c_k moves by +1 (d_k > 0) or -1 on that axis; if it leaves [0, E'_k), stop: a miss.  (4) Otherwise
 *     t = t < tk ? tk : t and axis = k.  Every step moves one coordinate the ray's way, so the walk ends within E'_x + E'_y + E'_z
 *     steps (at most 768).
 *   Winner: among the models hit the one with the smallest t, on equal t the lowest index.
 *   Depth test and writes: rt_draw_boxes' with t in place of t_in — P_k = rtm_fma(d_k, t, o_k), depth_f = rtm_length3(o - P) * 32.0f,
 *     drawn iff depth_f < RT_BUF_DEPTH_F32[pixel]; RT_BUF_NORMAL_R8UI = 2 axis + 1 if d_axis > 0, else 2 axis; RT_BUF_ALBEDO_RGBA8 = the
 *     UNORM8 pack of (albedo of the hit voxel's material word, 1); RT_BUF_EMISSION_RGBA8 = the record's `emission`; the two depth
 *     planes and the two lighting planes as for a box, with light = face_lights[6 i + normal].light.  The fog planes are not touched;
 *     every other pixel and plane keeps its bits.
 *   Which frame, ordering, side effects: rt_draw_boxes' — the planes of the frame drawn last, on the stream rt_denoise uses, behind
 *     the queries already enqueued; the frame slot's cached prepass is dropped; no accumulation sum, RT_FLAG_REPROJECT history set or
 *     count, RtCounters, pending edit box or slab changes.  Boxes and models drawn one after the other composite by the depth test,
 *     in either order.  A draw names its stamps as a placement does: rt_stamp_destroy after an enqueued draw waits for it.
 *   Errors: NULL ctx, NULL u, a NULL array with count > 0, count > 4096, a record that is not valid: RT_ERR_INVALID_ARG.
 *     tile_world != 1: RT_ERR_UNIMPLEMENTED.  No frame drawn yet: RT_ERR_NOT_READY.  count == 0: RT_OK, nothing enqueued, no prepass
 *     dropped.  All of it is checked on the host before anything is enqueued; a rejected call changes nothing.  No world need be
 *     resident beyond what a drawn frame implies.
 *   Device work per call: one transfer of a 64-byte record per model and one launch, a wave per 8x8 pixel tile; per tile the
 *     bounding boxes pass rt_draw_boxes' cull 64 at a time and only the survivors are walked per pixel.
 * `models` and `face_lights` are host pointers; returns when the planes are written. */
int rt_draw_stamps(RtContext* ctx, const RtUniforms* u, const RtDrawStamp* models, const RtProbeLight* face_lights, uint32_t count);
/* Same, enqueued.  `models` is a host pointer here too (ids, extents and orientations are resolved on the host, where entity
 * positions live) and is free again when the call returns; only `face_lights_dev` is device memory — what rt_probe_light_async
 * wrote, so probes feed models without a host sync.  It must pass rt_trace_rays_async's test (16-byte aligned memory of the context's
 * device, or managed memory), else RT_ERR_INVALID_ARG before anything is enqueued. */
int rt_draw_stamps_async(RtContext* ctx, const RtUniforms* u, const RtDrawStamp* models, const RtProbeLight* face_lights_dev, uint32_t count);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Particles: many small cubes — debris and dust of an explosion,
 * sparks, rain, snow, leaves, smoke puffs — composited by depth into the G-buffer of the frame drawn last exactly as the entity boxes
 * are, up to 2^20 per call.  The cost follows the pixels the cubes cover, not count x tiles: each 8x8 tile reads only the particles
 * binned to it.  The calls draw; they do not simulate: rt_step_particles_async ("Particle simulation" below) moves, bounces and
 * ages particles on the device and writes these records there, and the asynchronous draw takes device pointers, so particle state
 * need never visit the host.  One particle, 32 bytes: */
typedef struct RtParticle {       /* 32 bytes */
    float    center[3]; float half;         /* world coordinates of the cube's centre; half its edge */
    uint32_t material;  uint32_t emission;  /* as RtDrawBox's */
    uint32_t light;     uint32_t reserved;  /* index into `lights`; reserved must be 0 */
} RtParticle;
/* The rules, by reduction to rt_draw_boxes (tests/draw_particles_ref.py is that reduction and nothing more):
 *   Derived box: particle i is the box lo_k = center_k - half, hi_k = center_k + half, one fp32 rounding each, with the particle's
 *     material and emission.
 *   Light: all six faces take lights[light].light — one probe may serve a whole emitter or cluster; the host decides the sharing.
 *   Planes: every pixel and every plane ends with exactly the bits rt_draw_boxes leaves for the derived boxes in index order with
 *     face_lights[6 i + n] = lights[particle_i.light]: its ray, slab test, entry axis and winner (the smallest t_in, the lowest index
 *     on equal t_in), its strict depth test against RT_BUF_DEPTH_F32 and its seven plane writes.  A camera inside a cube does not
 *     see it.  Two runs of one call on equal planes give equal bits.
 *   Valid record: every float finite, half > 0, the derived box a valid RtDrawBox (|lo_k|, |hi_k| <= 2^22 and lo_k < hi_k after the
 *     rounding: a half that vanishes beside a large centre makes the record invalid), light < nlights, reserved == 0.  The device
 *     skips an invalid record in both calls; rt_draw_particles also rejects the whole call (RT_ERR_INVALID_ARG) before anything is
 *     enqueued.
 *   Limits: count <= 2^20 and 1 <= nlights <= 2^20 (with count > 0), else RT_ERR_INVALID_ARG.  half has no limit of its own.
 *   Errors, frame, ordering, side effects: rt_draw_boxes' — the frame drawn last, on the stream rt_denoise uses, behind the queries
 *     already enqueued (rt_probe_light_async feeds `lights_dev` without a host sync); the frame slot's cached prepass is dropped; no
 *     accumulation sum, history set or count, RtCounters, pending edit box or slab changes; NULL ctx, NULL u, a NULL array with
 *     count > 0: RT_ERR_INVALID_ARG; tile_world != 1: RT_ERR_UNIMPLEMENTED; no frame drawn yet: RT_ERR_NOT_READY; count == 0: RT_OK,
 *     nothing enqueued.  A rejected call changes nothing.
 *   Compositing: particles, boxes and models drawn one after another composite by the depth test.
 *   Device work per call: one memset and four launches — a thread per particle bins it to the 8x8 tiles it may touch (a conservative
 *     cull: it drops a tile only if the exact test rejects the particle for every pixel of it), a thread per list claims the list's
 *     room, a thread per particle fills the lists, a wave per tile draws from its lists.  A particle that may touch more than 16 tiles
 *     is listed by the blocks of 8x8 tiles it may touch; one that may touch more than 16 blocks is near the camera or huge: it goes to
 *     one wide list that every tile reads, at rt_draw_boxes' cost per record — the worst case.  Scratch: 8 + 8 lists + 72 count bytes
 *     of the context's, lists = tiles + blocks, grown on demand and never shrunk (RtInfo.device_bytes; a call that grows it waits for
 *     the launches that use the old one), freed by rt_destroy.  DESIGN.md "Particles".
 * Host pointers; returns when the planes are written. */
int rt_draw_particles(RtContext* ctx, const RtUniforms* u, const RtParticle* particles, uint32_t count, const RtProbeLight* lights,
                      uint32_t nlights);
/* Same with device pointers, enqueued: no host read-back and, once the scratch has its size, no host sync.  Both pointers must pass
 * rt_trace_rays_async's test (16-byte aligned memory of the context's device, or managed memory), else RT_ERR_INVALID_ARG before
 * anything is enqueued.  The library cannot read device records on the host: an invalid record is skipped on the device. */
int rt_draw_particles_async(RtContext* ctx, const RtUniforms* u, const RtParticle* particles_dev, uint32_t count,
                            const RtProbeLight* lights_dev, uint32_t nlights);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Particle simulation: one tick of up to 2^20 particles against the
 * resident region, on the device — explosion debris, rain that stops on roofs, sparks that bounce, snow that settles on terrain the
 * player has just edited.  A call integrates velocity, moves each particle's box through the world by rt_sweep_boxes' own rules (up
 * to four sub-sweeps per tick), responds to contact (die, stick, slide or bounce), ages the particle and writes both the next state
 * and the RtParticle record rt_draw_particles reads.  rt_step_particles_async -> rt_probe_light_async -> rt_draw_particles_async
 * runs without a host read.  Responses (RtParticleState.flags & RT_PSTATE_RESPONSE) and the other flag bits: */
#define RT_PARTICLE_DIE    0   /* contact kills the particle (rain, sparks that vanish)      */
#define RT_PARTICLE_STICK  1   /* contact stops it: velocity = 0 (snow, dust that settles)   */
#define RT_PARTICLE_SLIDE  2   /* the blocked axis of velocity and motion is zeroed          */
#define RT_PARTICLE_BOUNCE 3   /* the blocked axis is reflected times restitution            */
#define RT_PSTATE_RESPONSE 0x3u
#define RT_PSTATE_DEAD     0x100u     /* inactive: copied through, not drawn */
#define RT_PSTATE_INVALID  0x200u     /* set by the device on a record outside the domain; inactive */
#define RT_PSTATE_CONTACT  0x70000u   /* output: bit 16 + a set iff axis a blocked a sub-sweep this tick */
/* One particle's state, 64 bytes: */
typedef struct RtParticleState {   /* 64 bytes */
    float lo[3];       float life;        /*  0  the swept box (rt_sweep_boxes' lo / hi); seconds left, +inf = for ever */
    float hi[3];       uint32_t flags;    /* 16  RT_PARTICLE_* | RT_PSTATE_* */
    float velocity[3]; uint32_t light;    /* 32  units per second; RtParticle.light */
    uint32_t material; uint32_t emission; /* 48  RtParticle's */
    float half;        uint32_t reserved; /* 56  half edge of the DRAWN cube (constant; the swept box may differ from it); must be 0 */
} RtParticleState;
/* The parameters of one call, 48 bytes: */
typedef struct RtParticleStep {    /* 48 bytes */
    float dt;          float accel[3];    /*  0  seconds; gravity, wind: units per second^2 */
    float damping;     float restitution; float friction; float rest_speed;   /* 16 */
    int32_t lr[3];     uint32_t sweeps;   /* 32  the window, as rt_sweep_boxes'; sub-sweeps per tick 1..4 */
} RtParticleStep;
/* The rules.  All float arithmetic is fp32 with one rounding per operation and no fused multiply-add; max(x, c) is "x unless x < c",
 * min(x, c) is "x unless x > c".  Results are reproduced bit for bit by tests/particle_step_ref.py, which calls tests/sweep_ref.py
 * for every sub-sweep (DESIGN.md "Particle simulation").
 *   Inactive records: a record with DEAD or INVALID set on input is copied to `out` bit for bit.  Its draw record has half = 0, which
 *     rt_draw_particles_async skips as invalid; the other fields are as for a live particle.
 *   Valid records: every float finite, except that life may be +inf; half > 0; reserved == 0; no flag bit outside RESPONSE | DEAD |
 *     CONTACT (input CONTACT bits are ignored and overwritten); the box lo / hi inside rt_sweep_boxes' validated domain (|lo|, |hi| <=
 *     2^22, per axis 0 < hi - lo <= 8, the fp32 difference).  The device copies an active invalid record through with INVALID set and
 *     no other bit changed, draws it with half = 0 and fetches no voxel for it; rt_step_particles also refuses the whole call on the
 *     host (RT_ERR_INVALID_ARG) before anything is enqueued.  The rest is about the records that are active and valid on input.
 *   Integration: v_k = (v_k + accel_k * dt) * damping (three roundings), then the tick's motion m_k = min(max(v_k * dt, -64), 64).
 *   Sub-sweeps, for s = 0 .. sweeps - 1; stop when every m_k == 0.  h = what rt_sweep_boxes returns for (lo, hi, m) under lr, every
 *     field.  INVALID (a later sub-sweep's box collapsed by rounding): set INVALID and stop.  EMBEDDED (a block was placed onto the
 *     particle): set DEAD and stop.  Otherwise lo, hi = h.lo, h.hi.  FREE: stop.  BLOCKED on axis a: set contact bit 16 + a, then by
 *     response — DIE: set DEAD and stop.  STICK: v = (0, 0, 0) and stop.  Otherwise rest = 1 - h.t and m_k = m_k * rest for every k;
 *     SLIDE: m_a = 0, v_a = 0.  BOUNCE: w = -(v_a * restitution); if |w| < rest_speed then w = 0; v_a = w; m_a = (w != 0) ?
 *     -(m_a * restitution) : 0; on the other two axes v_k = v_k * friction and m_k = m_k * friction.  Motion left when the budget ends
 *     is dropped.
 *   Ageing: life = life - dt; if !(life > 0), set DEAD — also on a particle a sub-sweep has stopped, killed or marked.  The tick that
 *     kills a particle no longer draws it.
 *   Output state: lo, hi, velocity, life and flags as computed (RESPONSE kept, CONTACT this tick's); light, material, emission, half
 *     and reserved copied.
 *   Draw record: center_k = (lo_k + hi_k) * 0.5 of the output box; half = state.half, or 0 if DEAD or INVALID after the tick; material,
 *     emission and light copied; reserved 0.  (Where lo_k or hi_k of an inactive record is a NaN, center_k is a NaN whose sign and
 *     payload are not specified.)
 *   Call parameters, checked on the host in both calls (RT_ERR_INVALID_ARG): every float finite; 0 < dt <= 1; |accel_k| <= 4096;
 *     damping, restitution and friction in [0, 1]; rest_speed >= 0; sweeps in 1..4.
 *   Pointers: `out` may equal `in` for an in-place step (a lane reads its record whole before it writes); `draw` may be NULL.  No
 *     other overlap is allowed: ranges that overlap otherwise are RT_ERR_INVALID_ARG.
 *   Errors, world, ordering and side effects: rt_sweep_boxes' — no world resident: RT_ERR_NOT_READY; a NULL params, in or out with
 *     count > 0, or count > 2^20: RT_ERR_INVALID_ARG; count == 0: RT_OK, nothing enqueued.  The call sees every earlier upload, edit,
 *     slab and generated region and runs on the query stream, or on the caller's stream after rt_set_stream(non-NULL); later world
 *     changes wait for it.  No output plane, accumulation sum or history, RtCounters or RtTiming changes.  A rejected call writes
 *     nothing.  Tile contexts, every RtKernel and every region size answer the same.
 *   Closing property: on an unchanged world a live particle is never EMBEDDED, because each box it holds is one a sweep returned
 *     (the sweeps' clamps: "Box sweeps", Returned box) — given a first box that overlaps no occupied voxel.
 *   Out of scope: compaction of dead slots (it would make draw ties depend on atomics; a dead slot costs one record's traffic);
 *     emitters (a host overwrites the oldest slots of a ring with hipMemcpyAsync); collision events reported to the host;
 *     particle-particle and particle-entity contact; tile-split special cases (the call answers as the sweeps do).
 *     (Emitters, since then: rt_emit_particles — "Particle emitters" below — spawns debris from a shape's voxels on the device; rain and
 *     sparks, whose start the host knows, stay the host's overwrite.)
 *   Device work per call: one launch, one lane per particle: 64 bytes read, 64 (96 with `draw`) written, and the sub-sweeps' voxel
 *     fetches; the synchronous call adds a transfer each way.
 * Host pointers; returns when `out` (and `draw`) are in host memory. */
int rt_step_particles(RtContext* ctx, const RtParticleStep* params, const RtParticleState* in, RtParticleState* out, RtParticle* draw,
                      uint32_t count);
/* Same with device pointers, enqueued: `out_dev` and `draw_dev` are valid after rt_sync (or, after rt_set_stream, in the caller's
 * stream order); `params` is a host pointer, free again when the call returns.  in_dev, out_dev and a non-NULL draw_dev must pass
 * rt_trace_rays_async's test (16-byte aligned memory of the context's device, or managed memory), else RT_ERR_INVALID_ARG before
 * anything is enqueued; the states must be complete on the device when the call is made.  The library cannot read device records on
 * the host: an invalid record gets RT_PSTATE_INVALID on the device. */
int rt_step_particles_async(RtContext* ctx, const RtParticleStep* params, const RtParticleState* in_dev, RtParticleState* out_dev,
                            RtParticle* draw_dev, uint32_t count);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Particle emitters: debris spawned on the device from the voxels of a
 * shape — the explosion rt_edit_shapes carves, the block rt_edit_voxels breaks — one particle per occupied voxel, carrying that
 * voxel's material word, written into a ring of RtParticleState that rt_step_particles_async steps.  Which voxels are solid and what
 * they are made of lives in the device's arrays; before this call a host had to rt_read_box the bounding box (which waits for
 * everything submitted), test membership itself and upload the states.  rt_emit_particles_async -> rt_edit_shapes (carve) ->
 * rt_step_particles_async -> rt_probe_light_async -> rt_draw_particles_async runs without a host read.  One emitter, 96 bytes: */
typedef struct RtParticleEmit {      /* 96 bytes */
    int32_t  a[3];      uint32_t seed;                          /*  0  shape: RtShapeEdit's a; hash seed            */
    int32_t  b[3];      uint8_t kind, response, reserved0[2];   /* 16  RtShapeEdit's b; RT_SHAPE_*; RT_PARTICLE_*   */
    float    origin[3]; float speed;                            /* 32  blast centre, world units; radial speed      */
    float    drift[3];  float spread;                           /* 48  added velocity; amplitude of the jitter      */
    float    half;      float life_min; float life_span; uint32_t density;   /* 64  density 1..256: share of voxels kept, /256 */
    uint32_t light;     uint32_t emission; uint32_t reserved[2];             /* 80 */
} RtParticleEmit;
/* The ring's cursor, 16 bytes, in host memory for rt_emit_particles and in device memory for rt_emit_particles_async: */
typedef struct RtEmitCursor { uint32_t next, emitted, dropped, reserved; } RtEmitCursor;   /* 16 bytes */
/* The rules.  Everything up to the float block of a particle's state is integer arithmetic.  Results are reproduced bit for bit by
 * tests/emit_particles_ref.py, which calls tests/shape_edits.py for membership and restates no shape rule (DESIGN.md "Particle
 * emitters").
 *   Shape: (a, b, kind) mean exactly what they mean in RtShapeEdit — membership, clipping to [0, R)^3, the per-axis BOUNDING BOX and
 *     the +-R reissue of a shape that crosses the window's seam (+-2 R in `a` of a sphere).
 *   Selection: a voxel (texel x of the region) is SELECTED iff it is a member of the shape, its minefield byte is 0 at the moment
 *     the call runs in stream order, and (h & 255) < density with the voxel's hash h (below).  An emitter whose bounding box is empty
 *     selects nothing.
 *   World voxel of a texel: the sweeps' addressing — v_k is the one integer in [lr_k - R/2, lr_k + R/2) with (v_k + R/2) mod R ==
 *     x_k (Euclidean).  lr must satisfy |lr_k| <= 2^22 - R, else RT_ERR_INVALID_ARG: every emitted corner then lies inside
 *     rt_sweep_boxes' |lo|, |hi| <= 2^22.
 *   Hash, in uint32: mix(h): h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16.  h = mix(seed ^
 *     mix(uint32(v_x) ^ mix(uint32(v_y) ^ mix(uint32(v_z))))); g_i = mix(h + i) for i = 1..4; u_i = float(g_i >> 8) * 2^-24.  The
 *     hash takes world coordinates, not texels: a block's debris is the same wherever the window sits.
 *   Order: the selected voxels are numbered j = 0, 1, ... by ascending emitter index, and within an emitter by the key (z >> 2,
 *     y >> 2, x >> 2, z & 3, y & 3, x & 3) of the texel, compared lexicographically — brick-major, then the order inside a brick of
 *     the swizzled layout (one brick is 64 contiguous bytes, brick_index << 6).  A voxel selected by two emitters is emitted twice.
 *     No atomic decides a slot: two runs give equal bits.
 *   Ring and cursor: N = the number of selected voxels, n = min(N, max_emit).  Particle j < n is written whole, 64 bytes, to slot
 *     (next + j) mod capacity; the particles j >= n are dropped; every other slot keeps its bits.  Afterwards next = (next + n) mod
 *     capacity, emitted += n, dropped += N - n (wrapping uint32); `reserved` is untouched.  On the device an input next >= capacity
 *     is taken mod capacity; rt_emit_particles refuses such a cursor, and one with reserved != 0 (RT_ERR_INVALID_ARG).  Because the
 *     cursor lives on the device, a second rt_emit_particles_async can be chained behind the first without the host knowing n.
 *   State of one emitted particle, fp32 with one rounding per operation and no fused multiply-add (as in the step), in this order:
 *     c_k = float(v_k) + 0.5f; lo_k = c_k - half, hi_k = c_k + half (half <= 0.5: the box lies inside the voxel's own cell [v, v + 1];
 *     beside a large c the box may collapse — it is written as computed and the step marks it INVALID by its own rule); r_k = c_k -
 *     origin_k; len = rtm_length3(r); dir_k = len > 0 ? r_k / len : 0; velocity_k = (dir_k * speed + (u_{k+1} * 2 - 1) * spread) +
 *     drift_k; life = life_min + u_4 * life_span; flags = response; material = the voxel's material word; light, emission and half
 *     the emitter's; reserved = 0.
 *   Valid emitter, checked on the host in both calls (RT_ERR_INVALID_ARG; the message names the first invalid emitter): the shape
 *     valid by rt_edit_shapes' rule; response <= 3; the reserved bytes and words 0; density in 1..256; every float finite, except
 *     that life_min may be +inf; 2^-8 <= half <= 0.5; 0 <= speed, spread <= 4096; |drift_k| <= 4096; |origin_k| <= 2^22; life_min >
 *     0; 0 <= life_span <= 4096.
 *   Limits: count <= 256; 1 <= max_emit <= capacity <= 2^20; the clipped bounding boxes of one call cover at most 2^18 bricks (4^3
 *     voxels each) in total — a whole 256^3 region.  Anything else is RT_ERR_INVALID_ARG.
 *   Errors: a NULL pointer with count > 0: RT_ERR_INVALID_ARG.  count == 0: RT_OK, nothing enqueued.  A call whose bounding boxes
 *     are all empty: RT_OK, nothing enqueued, the cursor unchanged.  No world resident: RT_ERR_NOT_READY.  A rejected call writes
 *     nothing.
 *   Which world, ordering and side effects: the sweeps', exactly — the call runs on the query stream, or on the caller's stream
 *     after rt_set_stream(non-NULL); it sees every earlier upload, edit, slab and generated region; later world changes wait for it
 *     (so an emit enqueued before a carve reads the voxels the carve removes).  No output plane, accumulation sum or history,
 *     RtCounters, RtTiming, pending box or prepass changes.  Tile contexts, every RtKernel and every region size answer the same.
 *   The debris recipe: emit with the explosion's shape, then rt_edit_shapes with the same shape and solid = 0, then step.  Every
 *     emitted box lies in a cell the carve has just emptied, so the step's closing property holds from the first tick.  Emitting
 *     without carving leaves the particles EMBEDDED, and the first step kills them.
 *   Out of scope: emission from air or from entities, per-particle lights, velocity models beyond radial + jitter + drift, draw
 *     records (the next step writes those).
 *   Device work per call: the emitters' records (128 bytes each) through a staging set, then three launches — count (a wave per
 *     (emitter, brick): the brick's 64 minefield bytes, one ballot), scan (the cursor update among it), write (64 bytes per particle)
 *     — over a scratch of 12 bytes per brick that the context keeps (RtInfo.device_bytes).
 * `emitters` is a host pointer in both calls (the host sizes the launch from the bounding boxes), free again when the call returns.
 * Host pointers: `states` is the host's ring of `capacity` records, of which only the written slots change (at most two contiguous
 * copies); `cursor` is read and written on the host.  Returns when both are in host memory. */
int rt_emit_particles(RtContext* ctx, const RtParticleEmit* emitters, uint32_t count, const int32_t lr[3], RtParticleState* states,
                      uint32_t capacity, uint32_t max_emit, RtEmitCursor* cursor);
/* Same with a device ring and a device cursor, enqueued: both are valid after rt_sync (or, after rt_set_stream, in the caller's
 * stream order).  states_dev and cursor_dev must pass rt_trace_rays_async's test (16-byte aligned memory of the context's device, or
 * managed memory), else RT_ERR_INVALID_ARG before anything is enqueued; the cursor must be complete on the device when the call's
 * launches run (stream order: an earlier rt_emit_particles_async is). */
int rt_emit_particles_async(RtContext* ctx, const RtParticleEmit* emitters, uint32_t count, const int32_t lr[3], RtParticleState* states_dev,
                            uint32_t capacity, uint32_t max_emit, RtEmitCursor* cursor_dev);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Particle deposits: particles that have come to rest become voxels of
 * the resident region, on the device — rubble where the debris of an explosion lands, snow cover under snowfall, sand poured from a
 * tool.  Without this call a STICK particle stays a particle until its life runs out; a host that wants the pile must read 64 bytes
 * per particle back (which drains the pipeline), pick the resting ones, call rt_edit_voxels and upload the ring again with the dead
 * marked.  rt_emit_particles_async -> rt_edit_shapes (carve) -> rt_step_particles_async -> rt_deposit_particles_async ->
 * rt_probe_light_async -> rt_draw_particles_async runs without a host read.  The parameters of one call, 48 bytes: */
typedef struct RtParticleDeposit {   /* 48 bytes */
    int32_t lo[3];  float    max_speed;   /*  0  box of texels, inclusive, as a RT_SHAPE_BOX's a; rest threshold, units per second */
    int32_t hi[3];  uint32_t reserved0;   /* 16  as a RT_SHAPE_BOX's b; must be 0                                               */
    int32_t lr[3];  uint32_t reserved1;   /* 32  the window, as rt_step_particles'; must be 0                                   */
} RtParticleDeposit;
/* What a call did, 16 bytes, in host memory for rt_deposit_particles and in device memory for rt_deposit_particles_async: */
typedef struct RtDepositCount { uint32_t deposited, voxels, occupied, outside; } RtDepositCount;   /* 16 bytes */
/* The rules.  Results are reproduced bit for bit by tests/deposit_particles_ref.py, which applies the world change through
 * tests/voxel_edits.py and clips the box through tests/shape_edits.py (DESIGN.md "Particle deposits").
 *   Box: lo / hi mean what a RT_SHAPE_BOX's a / b mean — texels, inclusive — with the same validity (|lo_k|, |hi_k| <= 4 R, lo_k <=
 *     hi_k) and the same clipping to [0, R)^3.  The clipped box covers at most 2^24 texels, else RT_ERR_INVALID_ARG.  A host covers
 *     the window's seam with a second call whose box is shifted by +-R, as for shapes.
 *   Candidate: record i is a candidate iff DEAD and INVALID are clear, (flags & RT_PSTATE_CONTACT) != 0, |velocity_k| <= max_speed
 *     on every axis, and every lo_k, hi_k is finite with |.| <= 2^22.  Any comparison with a NaN is false.  STICK particles have
 *     velocity 0 and pass with max_speed = 0; BOUNCE and SLIDE debris passes once it has come to rest under rest_speed and friction.
 *   Target: c_k = (lo_k + hi_k) * 0.5f (fp32, one rounding each), v_k = (int)floorf(c_k): the world voxel that holds the box's
 *     centre.  Its texel is the emit's and the sweeps': x_k = (v_k + R/2) mod R (Euclidean), valid only if lr_k - R/2 <= v_k < lr_k
 *     + R/2.  lr must satisfy |lr_k| <= 2^22 - R, as for rt_emit_particles, else RT_ERR_INVALID_ARG.
 *   Outcome of a candidate: target outside the window or outside the clipped box: outside += 1 and nothing else.  Otherwise, the
 *     target's minefield byte is 0 at the moment the call runs in stream order, before any deposit of this call: occupied += 1 and
 *     nothing else.  Otherwise the record DEPOSITS: deposited += 1.
 *   Writes of a depositing record: RT_PSTATE_DEAD is ORed into its flags; if `draw` is non-NULL the 4 bytes draw[i].half become
 *     +0.0f (rt_draw_particles skips the record).  No other byte of `states` or `draw` changes, for any record.
 *   World: every texel targeted by at least one depositing record becomes occupied, and its material word becomes the `material`
 *     of the depositing record with the LOWEST INDEX; voxels += the number of such texels.  Every 64^3 chunk that holds at least one
 *     of them has its minefield rebuilt by rt_edit_voxels' rule — in such a chunk the result equals rt_edit_voxels with one solid = 1
 *     record per deposited texel — and no other chunk's bytes change.  The coarse / brick nibble-map words over the clipped box's
 *     chunks are rebuilt: rt_selftest(RT_SELFTEST_SCENE_MAPS) counts 0 afterwards.
 *   Counts: the four RtDepositCount fields are ADDED to (wrapping uint32); `counts` may be NULL.  The winner of a texel is a minimum
 *     and the counts are sums of integers, neither of which depends on arrival order: two runs give equal bits everywhere.
 *   Ordering: the call is a world change with rt_edit_shapes' stream order, lane join, fence and staging.  It waits for the queries
 *     and steps already enqueued, so a deposit enqueued behind rt_step_particles_async reads that step's states; later frames,
 *     queries and steps see the new world and the new flags.
 *   Side effects: rt_edit_shapes' for ONE box shape equal to the box, whenever the clipped box is non-empty and count > 0 — whether
 *     or not anything deposits, because the host cannot know: the accumulation restarts, or with RtConfig.edit_radius one box (the
 *     clipped box) waits for the next frame.  A host with a kept history deposits every few ticks and keeps the box tight round
 *     where its particles land.  (Bounds found on the device, as the slabs', are the follow-up.)
 *   Errors: NULL ctx, NULL params, NULL states with count > 0, count > 2^20, a non-finite or negative max_speed, a reserved word !=
 *     0, a bad box or window: RT_ERR_INVALID_ARG.  states, draw and counts must not overlap (RT_ERR_INVALID_ARG).  No world
 *     resident: RT_ERR_NOT_READY.  count == 0 or an empty clipped box: RT_OK, nothing enqueued or reset.  A rejected call changes
 *     nothing.  Tile contexts, every RtKernel and every region size answer as rt_edit_shapes does.
 *   Consequence: a live particle whose box overlaps a freshly deposited voxel is EMBEDDED at its next step and dies, by the step's
 *     existing rule ("Particle simulation", Sub-sweeps).  Nothing in the step changes.
 *   Out of scope: history bounds found on the device; particles larger than a voxel deposited into several voxels; falling or
 *     unsupported voxels.
 *   Device work per call: the box's chunk ids through an edit staging set, one fill of the scratch (4 bytes per texel of the clipped
 *     box, at most 64 MiB, that the context keeps: RtInfo.device_bytes), then three launches — claim (a lane per particle: 48 bytes
 *     read, one minefield byte, one atomic per depositing lane), chunks (a workgroup per chunk of the box; one that holds no deposit
 *     returns at once) and rt_edit_voxels' nibble-map rebuild.
 * Host pointers: states (and a non-NULL draw) go through the pinned block, the same launches run, and states, draw and counts are
 * copied back; returns when they are in host memory.  The world change itself stays stream-ordered. */
int rt_deposit_particles(RtContext* ctx, const RtParticleDeposit* params, RtParticleState* states, RtParticle* draw, uint32_t count,
                         RtDepositCount* counts);
/* Same with device pointers, enqueued: states_dev, draw_dev and counts_dev are valid after rt_sync (or, after rt_set_stream, in the
 * caller's stream order); `params` is a host pointer, free again when the call returns.  states_dev and a non-NULL draw_dev or
 * counts_dev must pass rt_trace_rays_async's test (16-byte aligned memory of the context's device, or managed memory), else
 * RT_ERR_INVALID_ARG before anything is enqueued. */
int rt_deposit_particles_async(RtContext* ctx, const RtParticleDeposit* params, RtParticleState* states_dev, RtParticle* draw_dev,
                               uint32_t count, RtDepositCount* counts_dev);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Voxel settling: loose voxels fall, on the device — sand or gravel
 * placed with rt_edit_voxels, the rubble a deposit poured, snow cover, the top of a pile after rt_edit_shapes carved a tunnel through
 * it.  Without this call they hang in the air; a host that wants them to fall reads the box back with rt_read_box (which drains both
 * lanes), walks the columns on the CPU and sends thousands of RtVoxelEdit records, every tick while anything is still falling.
 * rt_deposit_particles_async -> rt_edit_shapes (carve) -> rt_settle_voxels_async runs without a host read.  The terrain's up axis is
 * z: a game passes axis = 2, toward = 0.  The parameters of one call, 48 bytes: */
typedef struct RtVoxelSettle {          /* 48 bytes */
    int32_t  lo[3];  uint32_t max_fall;      /*  0  box of texels, inclusive, as RT_SHAPE_BOX's a; cells a voxel may fall in this call, >= 1; 0xFFFFFFFF = until it rests */
    int32_t  hi[3];  uint32_t air_material;  /* 16  as RT_SHAPE_BOX's b; material word left in a cell that ends the call unoccupied after a voxel left it */
    uint32_t loose_mask, loose_value;        /* 32  an occupied voxel is LOOSE iff (material & loose_mask) == loose_value; 0, 0: every occupied voxel */
    uint8_t  axis, toward, reserved0[2];     /* 40  axis 0..2 = x, y, z; toward 0: voxels fall to lower texel coordinates, 1: to higher */
    uint32_t reserved1;                      /* 44  must be 0 */
} RtVoxelSettle;
/* What a call did, 16 bytes, in host memory for rt_settle_voxels and in device memory for rt_settle_voxels_async: */
typedef struct RtSettleCount { uint32_t moved, falling, distance, chunks; } RtSettleCount;   /* 16 bytes, ADDED to, wrapping */
/* The rules.  Integer arithmetic only and a closed form: results are exact and do not depend on scheduling.  They are reproduced bit
 * for bit by tests/settle_voxels_ref.py, which changes the world only through tests/voxel_edits.py and clips the box through
 * tests/shape_edits.py (DESIGN.md "Voxel settling").
 *   Box: lo / hi mean what a RT_SHAPE_BOX's a / b mean — texels, inclusive — with the same validity (|lo_k|, |hi_k| <= 4 R, lo_k <=
 *     hi_k) and the same clipping to [0, R)^3, giving lo' / hi'.  There is no texel limit: the call needs no per-texel scratch.
 *     Nothing outside the clipped box is read or written.  The far face of the box in the fall direction is a floor: a voxel never
 *     leaves the box, and so never the region.  A host keeps the box off the window's seam.
 *   Cells of a column: fix the two other coordinates and number the clipped box's cells along `axis` by height: h = x - lo' for
 *     toward = 0, h = hi' - x for toward = 1; h = 0 .. H - 1.  A cell is OCCUPIED iff its minefield byte is 0 at the moment the call
 *     runs in stream order, an occupied cell is LOOSE iff (material & loose_mask) == loose_value, and an occupied cell that is not
 *     loose is FIXED.
 *   Fall: for a loose cell at h let f = 1 + the highest fixed h' < h (0 if there is none) and E(h) = the number of unoccupied cells
 *     h' with f <= h' < h.  The voxel moves to h - min(max_fall, E(h)) and keeps its material word.  Targets are distinct and the
 *     order inside a column is kept, because E(h2) - E(h1) <= h2 - h1 - 1.  T calls with max_fall = 1 equal one call with max_fall =
 *     T; 0xFFFFFFFF compacts every segment between fixed cells.
 *   Final state of the box: a cell that is the target of a voxel is occupied and holds that voxel's word; a cell that a voxel left
 *     and no voxel arrived at is unoccupied and holds air_material; every other cell keeps its occupancy and its material word —
 *     a cell a voxel only passed on its way included, so T single steps and one call of T agree on every voxel and on the whole
 *     minefield, while the single steps leave air_material in the unoccupied cells along the way.
 *   Dirty chunks: a 64^3 chunk is DIRTY iff it holds the source or the target cell of a voxel that moved.  Dirty chunks have their
 *     whole minefield rebuilt by rt_edit_voxels' rule and no other chunk's byte changes: in a dirty chunk the result equals
 *     rt_edit_voxels with one solid = 0, air_material record per source followed by one solid = 1 record per target (the last record
 *     of a voxel wins).  The coarse / brick nibble-map words over the clipped box's chunks are rebuilt:
 *     rt_selftest(RT_SELFTEST_SCENE_MAPS) counts 0 afterwards.  A call in which nothing moves leaves every minefield and material
 *     byte as it was.
 *   Counts: the four RtSettleCount fields are ADDED to (wrapping uint32); `counts` may be NULL.  moved: voxels with a non-zero drop.
 *     falling: loose voxels that could still fall after the call, E - drop > 0 — the host reads it to know when to stop calling.
 *     distance: the sum of all drops.  chunks: the number of dirty chunks.
 *   Ordering: the call is a world change with rt_edit_shapes' stream order, lane join, fence and staging, also under rt_set_stream.
 *   Side effects: rt_edit_shapes' for ONE box shape equal to the box, whenever the clipped box is non-empty — whether or not anything
 *     moved, because the host cannot know: the accumulation restarts, or with RtConfig.edit_radius one box (the clipped box) waits
 *     for the next frame.
 *   Errors: NULL ctx, NULL params, a bad box, axis > 2, toward > 1, max_fall == 0, loose_value & ~loose_mask != 0, a reserved byte or
 *     word != 0: RT_ERR_INVALID_ARG.  No world resident: RT_ERR_NOT_READY.  An empty clipped box: RT_OK, nothing enqueued or reset.
 *     A rejected call changes nothing.  Tile contexts, every RtKernel and every region size answer as rt_edit_shapes does.
 *   Out of scope: sideways sliding (an angle of repose); falling across the window's seam; history bounds found on the device;
 *     turning falling voxels into particles.  (Connectivity — a floating island that should fall as a body — is rt_detach_voxels',
 *     "Voxel detachment" below.)
 *   Device work per call: the box's chunk ids through an edit staging set, one fill of a flag word per chunk of the box, then three
 *     launches — columns (a lane per column of the clipped box walks it upwards and writes in place), chunks (a workgroup per chunk
 *     of the box; one that holds no moved voxel returns at once) and rt_edit_voxels' nibble-map rebuild.
 * With non-NULL `counts` (host memory) the call returns when the counts are in host memory; the world change itself stays
 * stream-ordered. */
int rt_settle_voxels(RtContext* ctx, const RtVoxelSettle* params, RtSettleCount* counts);
/* Same with device counts, enqueued: counts_dev is valid after rt_sync (or, after rt_set_stream, in the caller's stream order);
 * `params` is a host pointer, free again when the call returns.  A non-NULL counts_dev must pass rt_trace_rays_async's test (16-byte
 * aligned memory of the context's device, or managed memory), else RT_ERR_INVALID_ARG before anything is enqueued. */
int rt_settle_voxels_async(RtContext* ctx, const RtVoxelSettle* params, RtSettleCount* counts_dev);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Voxel detachment: what is no longer held up is found and lifted out
 * of the world, on the device — the top of a pillar an explosion cut through, a bridge whose supports were carved, an overhang.
 * rt_settle_voxels lets loose columns fall but knows nothing of connectivity: such a body stays hanging in the air unless the host
 * reads the box back with rt_read_box (which drains both lanes), flood-fills it on the CPU, sends one RtVoxelEdit per voxel and
 * builds a stamp from host arrays.  This call decides which voxels of a box are unsupported, carves them and captures them into a
 * stamp, which rt_draw_stamps draws as an entity, rt_sweep_entities moves without tunnelling, rt_shadow_entities shadows and
 * rt_edit_stamps pastes back where it lands: carve -> detach -> (draw, sweep, shadow) -> paste runs without a host read. */
#define RT_DETACH_CARVE            0x1u  /* detached voxels become unoccupied and hold air_material            */
#define RT_DETACH_CAPTURE          0x2u  /* detached voxels are written into a new stamp (id in *stamp_out)    */
#define RT_DETACH_ANCHOR_MATERIAL  0x4u  /* an occupied voxel with (material & anchor_mask) == anchor_value anchors too */
typedef struct RtVoxelDetach {           /* 48 bytes */
    int32_t  lo[3];  uint32_t flags;          /*  0  box of texels, inclusive, as RT_SHAPE_BOX's a; RT_DETACH_* bits */
    int32_t  hi[3];  uint32_t air_material;   /* 16  as RT_SHAPE_BOX's b; word left in a carved cell */
    uint32_t anchor_mask, anchor_value;       /* 32  read only with RT_DETACH_ANCHOR_MATERIAL, else both 0 */
    uint32_t max_passes;                      /* 40  1..256 */
    uint8_t  anchor_faces, reserved0[3];      /* 44  bit 2k: low face of axis k of the CLIPPED box, bit 2k+1: high */
} RtVoxelDetach;
/* What a call found, 48 bytes, in host memory for rt_detach_voxels and in device memory for rt_detach_voxels_async.  The counters
 * are ADDED to (wrapping uint32), the bounds MERGED (min into lo, max into hi): a host starts lo at INT32_MAX and hi at INT32_MIN. */
typedef struct RtDetachResult {          /* 48 bytes */
    uint32_t detached, supported, passes, unconverged;
    int32_t  lo[3];  uint32_t chunks;         /* texel bounds of the detached voxels; `chunks` = dirty chunks */
    int32_t  hi[3];  uint32_t reserved;       /* never written */
} RtDetachResult;
/* The rules.  Integer arithmetic only: results are exact and do not depend on scheduling.  They are reproduced bit for bit by
 * tests/detach_voxels_ref.py, which states them twice (a global flood fill, and the chunk passes below), changes the world only
 * through tests/voxel_edits.py and clips the box through tests/shape_edits.py (DESIGN.md "Voxel detachment").
 *   Box: lo / hi mean what a RT_SHAPE_BOX's a / b mean — texels, inclusive — with the same validity (|lo_k|, |hi_k| <= 4 R, lo_k <=
 *     hi_k) and the same clipping to [0, R)^3, giving lo' / hi'.  Every extent hi'_k - lo'_k + 1 of the clipped box must be at most
 *     256: the stamps' limit, and the bound of the per-texel scratch.  Nothing outside the clipped box is read, and nothing outside
 *     it is written apart from the minefield bytes of dirty chunks.  A host keeps the box off the window's seam.
 *   Occupied and anchor: a cell of the clipped box is OCCUPIED iff its minefield byte is 0 at the call's place in stream order.  An
 *     occupied cell is an ANCHOR iff it lies on a face of the clipped box whose bit is set in anchor_faces, or — with
 *     RT_DETACH_ANCHOR_MATERIAL — iff (material & anchor_mask) == anchor_value.  A call with no anchors is valid: every occupied
 *     cell is then detached.
 *   Supported and detached: SUPPORTED is the set of occupied cells reachable from an anchor by steps between face-adjacent occupied
 *     cells of the clipped box (6-connectivity: contact along an edge or at a corner does not connect).  DETACHED = occupied and
 *     not supported.
 *   Passes: the pass count is part of the contract, so that max_passes behaves the same on every run.  Partition the clipped box by
 *     the 64^3 texel-aligned chunks and let S_0 be the anchors.  For p >= 1 and every chunk part C, S_p within C is the closure
 *     inside C, through occupied cells, of (S_{p-1} within C) and the occupied cells of C that are face-adjacent across a chunk face
 *     to a cell of S_{p-1}.  The first p with S_p = S_{p-1} ends the process (S_p is SUPPORTED) and passes += p.  If no p <=
 *     max_passes ends it: unconverged += 1, passes += max_passes, no world byte changes, detached / supported / chunks and the bounds
 *     get nothing, and a requested stamp holds no voxel.  A box inside one chunk ends with p = 1 or 2.
 *   RT_DETACH_CARVE: every detached cell becomes unoccupied and holds air_material.  A chunk is DIRTY iff it holds a detached cell;
 *     dirty chunks have their whole minefield rebuilt by rt_edit_voxels' rule — the result equals rt_edit_voxels with one solid = 0,
 *     air_material record per detached voxel — and no other chunk's byte changes.  The coarse / brick nibble-map words over the
 *     box's chunks are rebuilt: rt_selftest(RT_SELFTEST_SCENE_MAPS) counts 0 afterwards.  Side effects are rt_edit_shapes' for ONE
 *     box shape equal to the clipped box whenever it is non-empty — detached or not, converged or not, because the host cannot know:
 *     the accumulation restarts, or with RtConfig.edit_radius one box (the clipped box) waits for the next frame.  The call is a
 *     world change with rt_edit_shapes' stream order, lane join, fence and staging, also under rt_set_stream.
 *   RT_DETACH_CAPTURE: stamp_out must be non-NULL.  A stamp of the clipped box's extent is created before anything is enqueued and
 *     its id is valid on return, in both variants.  Stamp voxel d corresponds to texel lo' + d: a detached voxel is RT_STAMP_SOLID
 *     with its material word, every other voxel RT_STAMP_ABSENT with word 0.  The capture reads the world before the carve of the
 *     same call.  The limit of 1024 live stamps and RT_ERR_OOM behave as in rt_stamp_capture; rt_stamp_read, rt_stamp_destroy,
 *     rt_edit_stamps and rt_draw_stamps treat the stamp like any other.  One stamp holds every detached body of the box.
 *   Neither flag: a query, ordered like rt_stamp_capture.  It changes nothing the renderer reads, does not reset the accumulation
 *     and records no pending box.  RT_DETACH_CAPTURE alone is ordered the same way.
 *   Result: `result` may be NULL.  detached and supported count cells; chunks counts dirty chunks (with or without
 *     RT_DETACH_CARVE); lo / hi are merged with the texel bounds of the detached cells.
 *   Errors: NULL ctx or params, a bad box, a clipped extent above 256, an unknown flag bit, max_passes outside 1..256, anchor_faces
 *     above 63, anchor_value & ~anchor_mask != 0, a mask or value set without RT_DETACH_ANCHOR_MATERIAL, a reserved byte != 0,
 *     RT_DETACH_CAPTURE with a NULL stamp_out, RT_DETACH_CAPTURE with 1024 stamps live: RT_ERR_INVALID_ARG.  No world resident:
 *     RT_ERR_NOT_READY.  An empty clipped box: RT_OK, nothing enqueued or reset, and *stamp_out = 0 if given.  A rejected call
 *     changes nothing and creates no stamp.  Tile contexts, every RtKernel and every region size answer as rt_edit_shapes does.
 *   Out of scope: stamps cut to the detached bounds; one stamp per body; boxes across the window's seam; history bounds found on
 *     the device; 18- or 26-connectivity; rotation or physics of the falling body (the host moves it with rt_sweep_entities).
 *   Device work per call: a seed launch (a workgroup per chunk of the box: occupancy bits and anchors), max_passes reach launches (a
 *     workgroup per chunk closes its reach bits in LDS; every workgroup of a launch after the end returns at once), an apply launch
 *     and, with RT_DETACH_CARVE, the chunk rebuild (a chunk without a detached voxel returns at once) and rt_edit_voxels' nibble-map
 *     rebuild.  No host read sits in between.
 * With non-NULL `result` (host memory) the call returns when the result is in host memory; a world change stays stream-ordered. */
int rt_detach_voxels(RtContext* ctx, const RtVoxelDetach* params, RtDetachResult* result, uint32_t* stamp_out);
/* Same with a device result, enqueued: result_dev is valid after rt_sync (or, after rt_set_stream, in the caller's stream order);
 * `params` and `stamp_out` are host pointers.  A non-NULL result_dev must pass rt_trace_rays_async's test (16-byte aligned memory of
 * the context's device, or managed memory), else RT_ERR_INVALID_ARG before anything is enqueued. */
int rt_detach_voxels_async(RtContext* ctx, const RtVoxelDetach* params, RtDetachResult* result_dev, uint32_t* stamp_out);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Fluid flow: a level-based fluid spreads, falls and dries up, on the
 * device — the water behind a dam rt_edit_shapes broke, a spring on a ledge, lava down a slope.  Without this call the fluid hangs
 * where it was placed; a host that wants it to run reads the box back with rt_read_box (which drains both lanes), runs a cellular
 * automaton on the CPU and sends thousands of RtVoxelEdit records, every tick while anything still moves.  Each call advances the
 * fluid by `ticks` synchronous steps inside a box of texels: rt_edit_shapes (carve the dam) -> rt_flow_voxels_async runs without a
 * host read.  It is the familiar game rule: sources never run out, fluid falls, spreads sideways only where it stands on something,
 * loses one level per sideways cell and dries when nothing feeds it.  The parameters of one call, 64 bytes: */
typedef struct RtVoxelFlow {             /* 64 bytes */
    int32_t  lo[3];  uint32_t ticks;          /*  0  box of texels, inclusive, as RT_SHAPE_BOX's a; 1..256 */
    int32_t  hi[3];  uint32_t air_material;   /* 16  as RT_SHAPE_BOX's b; word left in a cell that was fluid and ends the call unoccupied */
    uint32_t fluid_mask, fluid_value;         /* 32  an occupied voxel is FLUID iff (material & fluid_mask) == fluid_value */
    uint32_t fluid_word, reserved0;           /* 40  word a newly wetted cell gets (level field 0; the call writes it); must be 0 */
    uint8_t  level_shift, max_level, reserved1[2];  /* 48  0..28; 1..13 */
    uint32_t reserved2[3];                    /* 52  must be 0 (an up axis other than +z would go here) */
} RtVoxelFlow;
/* What a call did, 32 bytes, in host memory for rt_flow_voxels and in device memory for rt_flow_voxels_async: */
typedef struct RtFlowCount { uint32_t wetted, dried, changed, active, chunks, reserved[3]; } RtFlowCount;  /* 32 bytes, ADDED to, wrapping; reserved never written */
/* The rules.  Integer arithmetic only, and every cell's next state is a function of the previous state of its neighbourhood: results
 * are exact, do not depend on scheduling and are equal from run to run.  They are reproduced bit for bit by tests/flow_voxels_ref.py,
 * which states them twice (a loop per cell over explicit neighbours, and whole-array shifts), changes the world only through
 * tests/voxel_edits.py and clips the box through tests/shape_edits.py (DESIGN.md "Fluid flow").
 *   Box: lo / hi mean what rt_settle_voxels' mean — texels, inclusive — with the same validity (|lo_k|, |hi_k| <= 4 R, lo_k <= hi_k)
 *     and the same clipping to [0, R)^3, giving lo' / hi'.  Every extent hi'_k - lo'_k + 1 of the clipped box must be at most 256:
 *     the bound of the per-texel scratch, and rt_detach_voxels' limit too.  Up is +z.  Nothing outside the clipped box is read, and
 *     nothing outside it is written apart from the minefield bytes of dirty chunks.  Under the low z face is a floor, which counts
 *     as FIXED.  Above the high z face and sideways there are no cells: nothing feeds in from there and nothing leaves.  A host
 *     keeps the box off the window's seam.
 *   Field: FIELD = 0xF << level_shift.  For a fluid cell v = (material >> level_shift) & 0xF: v == 15 is a SOURCE, otherwise the
 *     cell is FLOWING with strength min(v, max_level) — strength 0 is possible, and so are raw values above max_level, 14 included.
 *   Cell kinds, taken at the call's place in stream order: OCCUPIED iff the minefield byte is 0; FLUID iff occupied and (material &
 *     fluid_mask) == fluid_value; FIXED iff occupied and not fluid; EMPTY otherwise.  Other fluids are FIXED to this call.
 *   Giving strength: e(n) = max_level + 1 for a source, the strength for a flowing cell, 0 for anything else.
 *   Spreading: a fluid cell n is SPREADING iff it is a source, or the cell n - z is FIXED (the floor included).
 *   One tick, all reads from the state before the tick: FIXED and SOURCE cells keep their state.  Every other cell c gets s' =
 *     max(D, S): D = max_level if c + z is in the box and is a source or a flowing cell of strength >= 1, else 0; S = the maximum of
 *     e(n) - 1 over the four horizontal neighbours n in the box that are SPREADING and have e(n) >= 1, or 0 with no such neighbour.
 *     s' >= 1: c is flowing with strength s'.  s' = 0: c is empty.  (A flowing cell of strength 0 gives nothing and holds nothing
 *     up: to the tick it is an empty cell.)
 *   After `ticks` ticks, compared with the state before the call: a cell that is flowing at the end is occupied and its word is (w &
 *     ~FIELD) | s << level_shift, where w is its own word if it was fluid at the start, else fluid_word.  A cell that was fluid at
 *     the start and is empty at the end is unoccupied and holds air_material.  Every other cell keeps its byte and its word — a
 *     cell that was wetted and dried again inside the call included.  So T calls of one tick and one call of T ticks agree on every
 *     occupied cell and on the whole minefield, while the single ticks leave air_material in the unoccupied cells that were wet on
 *     the way (rt_settle_voxels' precedent).  One corner: a fluid cell that dries and is wetted again on the way keeps the bits of
 *     its own word outside FIELD in the one call and has fluid_word's after the single ticks; its level agrees.
 *   Dirty chunks: a 64^3 chunk is DIRTY iff it holds a cell whose occupancy changed.  Dirty chunks have their whole minefield rebuilt
 *     by rt_edit_voxels' rule — the result equals rt_edit_voxels with one record per such cell — and no other chunk's minefield byte
 *     changes.  A cell whose level alone changed gets its word written and dirties nothing.  The coarse / brick nibble-map words
 *     over the clipped box's chunks are rebuilt: rt_selftest(RT_SELFTEST_SCENE_MAPS) counts 0 afterwards.
 *   Counts: the RtFlowCount fields are ADDED to (wrapping uint32); `counts` may be NULL; reserved is never written.  wetted: cells
 *     unoccupied at the start and fluid at the end.  dried: fluid at the start, unoccupied at the end.  changed: cells of the box
 *     whose occupancy or material word differs from before the call — wetted, dried and those whose level alone changed; the bytes
 *     the rebuild of a dirty chunk gives its other unoccupied cells are not counted.  chunks: dirty chunks.  active: cells whose
 *     state (empty, strength, source, fixed) would change in one more tick — the host stops ticking when active is 0.
 *   Ordering and side effects are exactly rt_settle_voxels': a world change with rt_edit_shapes' stream order, lane join, fence and
 *     staging, also under rt_set_stream; one pending box, the clipped box, whenever it is non-empty — whether or not anything
 *     changed, because the host cannot know: the accumulation restarts, or with RtConfig.edit_radius the box waits for the next frame.
 *   Errors: NULL ctx or params, a bad box, a clipped extent above 256, ticks outside 1..256, level_shift above 28, max_level outside
 *     1..13, fluid_mask == 0, fluid_mask & FIELD != 0, fluid_value & ~fluid_mask != 0, fluid_word & FIELD != 0, (fluid_word &
 *     fluid_mask) != fluid_value, a reserved byte or word != 0: RT_ERR_INVALID_ARG.  No world resident: RT_ERR_NOT_READY.  An empty
 *     clipped box: RT_OK, nothing enqueued or reset.  A rejected call changes nothing.  Tile contexts, every RtKernel and every
 *     region size answer as rt_edit_shapes does.
 *   Out of scope: volume conservation and pressure; two fluids meeting; an up axis other than +z; boxes across the window's seam;
 *     history bounds found on the device.  Queries and sweeps go on treating fluid cells as occupied voxels (a passable mask for
 *     rt_sweep_boxes and the navigation fields — swimming — is the follow-up), and the renderer shows a fluid by its albedo, opaque.
 *   Device work per call: the box's chunk ids through an edit staging set, a seed launch (a lane per cell: its state — empty, a
 *     strength, source or fixed — into a byte of a scratch the context keeps: two state arrays of the clipped box, at most 2 x 256^3
 *     bytes), ceil(ticks / G) tick launches that ping-pong the arrays (a workgroup per tile of 32 x 16 x 16 cells runs G ticks in LDS
 *     on the tile and a halo of G cells; G = 4, RT_FLOW_TICKS = 1, 2, 4 or 8 for A/B timing; the workgroups of launches after one
 *     that changed nothing return at once), an apply launch (a lane per cell writes what differs and counts), the chunk rebuild (a
 *     chunk without a cell whose occupancy changed returns at once) and rt_edit_voxels' nibble-map rebuild.  No host read sits in
 *     between.
 * With non-NULL `counts` (host memory) the call returns when the counts are in host memory; the world change itself stays
 * stream-ordered. */
int rt_flow_voxels(RtContext* ctx, const RtVoxelFlow* params, RtFlowCount* counts);
/* Same with device counts, enqueued: counts_dev is valid after rt_sync (or, after rt_set_stream, in the caller's stream order);
 * `params` is a host pointer, free again when the call returns.  A non-NULL counts_dev must pass rt_trace_rays_async's test (16-byte
 * aligned memory of the context's device, or managed memory), else RT_ERR_INVALID_ARG before anything is enqueued. */
int rt_flow_voxels_async(RtContext* ctx, const RtVoxelFlow* params, RtFlowCount* counts_dev);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Navigation fields: where a mob goes.  A mob can be drawn, moved
 * without tunnelling, hit, seen, shadowed and lit; in a world that explosions carve, sand fills and pillars leave, a precomputed
 * navmesh is wrong after the first edit, and the host answer — rt_read_box round the player (which drains both lanes), a breadth-
 * first search on the CPU, an upload of the steps — is the host path the last calls removed.  A NAV FIELD holds, for every cell of a
 * box of texels a walker can stand in, the number of moves to the nearest goal and the move to make next: built on the device once
 * per change (rt_nav_build), sampled for any number of agents in one launch (rt_nav_sample).  Breadth-first distances are integers
 * and unique, so results are exact and do not depend on scheduling; tests/nav_field_ref.py states the rules twice.
 *
 * Objects (they mirror the stamps').  rt_nav_create — a field of `extent` cells (each 1..256), all a build needs allocated with it:
 * the field (3 bytes per cell) and the bitmaps and launch record of the search; a build allocates nothing.  Ids are non-zero and
 * valid until rt_nav_destroy; at most 64 fields are live per context (the 65th: RT_ERR_INVALID_ARG); RT_ERR_OOM when the device has
 * no room.  RtInfo.device_bytes counts fields; rt_destroy frees the rest.  rt_nav_info — the extent, the `lo` of the build enqueued
 * last and whether there was one (any out pointer may be NULL).  rt_nav_read — dist and move of the build enqueued last,
 * [ez][ey][ex] with x fastest (either may be NULL; synchronises; RT_ERR_NOT_READY for a field never built).  rt_nav_destroy —
 * waits for the builds and samples already enqueued. */
int rt_nav_create (RtContext* ctx, const int32_t extent[3], uint32_t* id_out);
int rt_nav_info   (RtContext* ctx, uint32_t id, int32_t extent_out[3], int32_t lo_out[3], uint32_t* built_out);
int rt_nav_read   (RtContext* ctx, uint32_t id, uint16_t* dist, uint8_t* move);   /* either may be NULL; synchronises */
int rt_nav_destroy(RtContext* ctx, uint32_t id);

#define RT_NAV_UNREACHED  0xFFFFu   /* dist of a cell that is not standable, or farther than max_dist from every goal */
#define RT_NAV_NO_MOVE    0xFFu     /* move of a goal cell and of an unreached cell */
typedef struct RtNavBuild {            /* 32 bytes */
    int32_t  lo[3];  uint32_t max_dist;                  /*  0  low corner of the box in texels; 1..4096 */
    uint8_t  height, max_climb, max_drop, goal_snap;     /* 16  1..4, 0..2, 0..8, 0..8 */
    uint32_t reserved[3];                                /* 20  must be 0 (an up axis other than +z would go here) */
} RtNavBuild;
typedef struct RtNavGoal   { int32_t cell[3]; uint32_t reserved; } RtNavGoal;   /* 16 bytes; texel; `reserved` is not read */
typedef struct RtNavResult {           /* 32 bytes; `reserved` is never written */
    uint32_t standable, reached, levels, truncated, goals_used, goals_dropped, reserved[2];
} RtNavResult;
/* The rules.  Integer arithmetic only: results are exact.  tests/nav_field_ref.py reproduces them bit for bit, twice (an explicit
 * move graph with a queue, and whole-array dilation); DESIGN.md "Navigation fields" says why they are what they are.
 *   Box: [lo, lo + E) with E the field's extent; it must lie inside [0, R)^3, as rt_stamp_capture's box must — there is no clipping.
 *     Cell d of the field is texel lo + d.  Up is +z, the terrain's up axis.  Nothing outside the box is read.  Under the box's low
 *     z face is a floor: it counts as occupied.  Above its high z face everything counts as unoccupied.  Sideways there are no cells
 *     outside the box.  A host keeps the box off the window's seam.
 *   Occupied, clearance, standable: a cell is OCCUPIED iff its minefield byte is 0 at the call's place in stream order.  CLEAR(c)
 *     is the number of consecutive unoccupied cells c, c+z, c+2z, ... (the cells above the box count as unoccupied).  c is STANDABLE
 *     iff c-z is occupied and CLEAR(c) >= height.
 *   Moves: a -> b is a MOVE iff both cells are standable, b.xy - a.xy is one of (+1,0), (-1,0), (0,+1), (0,-1) — h = 0..3 in that
 *     order —, k = b.z - a.z satisfies -max_drop <= k <= max_climb, and the LOWER of the two cells has CLEAR >= |k| + height: its
 *     column is free up to head height at the higher level, so no head bumps while stepping up and no ledge is in the way while
 *     dropping.  Moves are directed: a cliff of 3 with max_drop 3 and max_climb 1 goes down only.  A move's CODE is
 *     h | (k + 8) << 2.  The ORDER of moves is h ascending and, inside one h, k descending.
 *   Goals: goal_count <= 4096; 0 is valid: nothing is reached.  The goal cell of a record is the first standable cell among c, c-z,
 *     ..., c - goal_snap z that lies in the box.  A record without one — any outside the box among them — counts in goals_dropped,
 *     the others in goals_used; duplicates count each time.
 *   Field: dist[c] is the least number of moves from c to any goal cell if that number is <= max_dist, else 0xFFFF; it is 0xFFFF
 *     as well for every cell that is not standable.  move[c] is the code of the first move in ORDER to a cell with dist =
 *     dist[c] - 1 when 0 < dist[c] < 0xFFFF, else 0xFF.  A build overwrites every cell of the field: nothing of an earlier build
 *     survives, whatever lo it had.
 *   Result: standable, reached (cells with dist < 0xFFFF), truncated, goals_used and goals_dropped are ADDED to (wrapping uint32);
 *     truncated += 1 iff some cell's least number of moves is exactly max_dist + 1; levels is MERGED by maximum with the largest
 *     dist assigned.  `result` may be NULL.
 *   Ordering: a query, ordered like rt_stamp_capture: it sees every earlier world change and changes nothing the renderer reads,
 *     causes no accumulation reset and records no pending box.  A later edit makes the field stale: the host rebuilds.
 *   Errors: NULL ctx or params, an unknown id, a parameter outside its range above, a non-zero reserved word of RtNavBuild, a box not
 *     inside the region, NULL goals with goal_count > 0, goal_count > 4096: RT_ERR_INVALID_ARG.  No world resident:
 *     RT_ERR_NOT_READY.  A rejected call changes nothing.  Tile contexts, every RtKernel and every region size answer as
 *     rt_stamp_capture does.
 *   Out of scope: agents wider than one cell; diagonal moves; move costs other than 1; swimming or flying; entities as obstacles;
 *     boxes across the window's seam; an up axis other than +z; incremental repair after an edit.
 *   Device work per build: a seed launch (the box's unoccupied bits, the field's fill), a launch that finds and counts the
 *     standable cells, a launch with a lane per goal, ceil((max_dist + 1) / G) level launches (G = 8 levels each, run in LDS by one
 *     workgroup per tile of 16 x 16 columns; every workgroup of a launch after the frontier has died returns at once) and a launch
 *     that gives every reached cell its move code.  No host read sits in between.
 * rt_nav_build: `goals` and `result` are host memory; the call returns when the result is in host memory. */
int rt_nav_build(RtContext* ctx, uint32_t id, const RtNavBuild* params, const RtNavGoal* goals, uint32_t goal_count, RtNavResult* result);
/* Same with device goals and a device result, enqueued: result_dev is valid after rt_sync (or, after rt_set_stream, in the caller's
 * stream order); `params` is a host pointer.  goals_dev (with goal_count > 0) and a non-NULL result_dev must pass
 * rt_trace_rays_async's test (16-byte aligned memory of the context's device, or managed memory), else RT_ERR_INVALID_ARG before
 * anything is enqueued. */
int rt_nav_build_async(RtContext* ctx, uint32_t id, const RtNavBuild* params, const RtNavGoal* goals_dev, uint32_t goal_count,
                       RtNavResult* result_dev);

/* Sampling a field: a pure lookup — the world is not read.  `pos` is the agent's foot point: the centre of its box in x and y, its lo
 * in z (texel coordinates, as the box's lo).  With c0 = floor(pos) per component the candidates are, in this order: c0; c0-z ...
 * c0 - snap_down z; c0+z ... c0 + snap_up z.  Candidates outside the box are skipped.  The agent's cell is the first candidate with
 * dist < 0xFFFF: `cell` is its texel, `dist` its distance, `move` its code and `next` the texel the move leads to; with dist 0,
 * next = cell and move = 0xFF.  With no such candidate: cell = next = c0, dist = 0xFFFFFFFF, move = 0xFF.  With a non-finite
 * component or one of magnitude >= 2^20, a non-zero reserved byte, snap_down above 8 or snap_up above 2: cell = next = (-1,-1,-1),
 * dist = 0xFFFFFFFF, move = 0xFF (the asynchronous call cannot refuse a record it has not read — RT_SWEEP_INVALID's precedent — and
 * the synchronous call answers the same).  Every record is written.  count <= 2^20; 0 enqueues nothing.  The sample is ordered
 * after the builds enqueued before it and reads the box of the build enqueued last.  Errors: NULL ctx, an unknown id, count above
 * 2^20, NULL agents or steps with count > 0: RT_ERR_INVALID_ARG; a field never built: RT_ERR_NOT_READY. */
typedef struct RtNavAgent { float pos[3]; uint8_t snap_down, snap_up, reserved[2]; } RtNavAgent;          /* 16 bytes; 0..8, 0..2 */
typedef struct RtNavStep  { int32_t cell[3]; uint32_t dist; int32_t next[3]; uint32_t move; } RtNavStep;  /* 32 bytes */
int rt_nav_sample(RtContext* ctx, uint32_t id, const RtNavAgent* agents, uint32_t count, RtNavStep* steps);
/* Same on device memory, enqueued: agents_dev and steps_dev must pass rt_trace_rays_async's test; steps_dev is valid after rt_sync
 * (or, after rt_set_stream, in the caller's stream order). */
int rt_nav_sample_async(RtContext* ctx, uint32_t id, const RtNavAgent* agents_dev, uint32_t count, RtNavStep* steps_dev);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Point lights: light sources that move — a torch in the player's
 * hand, a glowing projectile, a muzzle flash, the flash of an explosion — added to the two lighting planes of the frame drawn last,
 * after rt_draw_frame (and rt_draw_boxes) and before or after rt_denoise.  Each light reaches a pixel through one hard shadow ray
 * against the resident region; rt_finalize multiplies lighting by albedo, so the added light is diffuse shading.  Entities cast no
 * shadow in a point light here (rt_add_lights_occluded is the call in which they do), the source gives no bounce light, and the light belongs to one frame: it enters no accumulation sum or history.  One light,
 * 32 bytes: */
typedef struct RtPointLight {     /* 32 bytes */
    float    position[3];  float    radius;     /* world coordinates; nothing is lit at or beyond `radius` */
    float    color[3];     uint32_t reserved;   /* the shader's light unit (what RtProbeLight.light is in); reserved must be 0 */
} RtPointLight;
/* The rules.  All arithmetic is fp32 with one rounding per operation; fused operations appear only where rtm_fma or rtm_dot3 is
 * written.  Results are reproduced bit for bit by tests/point_light_ref.py, which tests every light against every pixel (DESIGN.md
 * "Point lights").
 *   Inputs: origin, forward, up, right and lr of `u` are read; the host passes the uniforms of the frame it drew.
 *   Surface pixel: RT_BUF_NORMAL_R8UI < 6 and RT_BUF_DEPTH_F32 < 65535.0f (a NaN depth fails).  Every other pixel keeps all its bits.
 *   Surface point: d is the ray of rt_draw_boxes (the same sx, sy and rtm_normalize3, from o = u.origin, no slide);
 *     t = depth_f / 32.0f; P_k = rtm_fma(d_k, t, o_k).  With a = normal >> 1: P'_a = P_a + 0.03125f for an even code (it faces +axis)
 *     and P_a - 0.03125f for an odd one; the other two components of P' are P's.  (1/32 is far above the error of a rebuilt point,
 *     about 1e-3 at 2048 units.)  Entity pixels written by rt_draw_boxes go through the same rule with the box's depth and face code.
 *   Valid light: every float finite, |position_k| <= 2^22, 0 < radius <= 1024, 0 <= color_k <= 2^20, reserved == 0.  The device skips
 *     an invalid light in both calls; rt_add_lights also rejects the whole call (RT_ERR_INVALID_ARG) before anything is enqueued.
 *   Light i against the pixel ("skip": the light adds nothing to this pixel): v = position - P' per component; dist2 = rtm_dot3(v, v);
 *     r2 = radius * radius; skip unless dist2 > 0 && dist2 < r2; c = v_a for an even code, -v_a for an odd one; skip unless c > 0.
 *     A comparison with a NaN is false: a NaN skips.
 *   Shadow ray: trace_ray (raytrace.comp:82-183) from P' in direction v (trace_ray normalises it), with u.lr and the resident region,
 *     and one added exit: in each loop iteration, after the sky test (:138-145) found the new position inside the window and before
 *     the hit test (:146), if rtm_dot3(pos - P', pos - P') >= dist2 the ray has reached the light: visible.  The other exits are the
 *     shader's: leaving the window: visible; a minefield value of 0 (the border value and a start inside an occupied texel, the
 *     mod(x, 0) case, included): blocked; the loop limit: blocked.  A light inside a solid voxel lights nothing; a solid voxel behind
 *     the light does not shadow it.
 *   Weight and sum: len = rtm_sqrt(dist2); cosine = c / len; x = 1.0f - dist2 / r2; w = (cosine * (x * x)) / (1.0f + dist2);
 *     add_k = add_k + color_k * w over the visible lights in index order, starting from +0.0f.  (Colours are >= 0, so a skipped light
 *     leaves the sum's bits as they are.)
 *   Writes, only for a pixel with at least one visible light: s_k = add_k / 16.0f; RT_BUF_LIGHTING_F32.rgb += s; independently
 *     RT_BUF_LIGHTING_RGBA16.rgb = rtm_unorm(float(q_k) / 65535.0f + s_k, 65535.0f), q the texel as it stands.  Both alphas are
 *     untouched.  Each plane gets the light in its own representation, so the host chooses where to call: before rt_denoise the light
 *     is filtered with the rest, after it point-light shadows stay crisp.  No other plane, pixel or byte changes.
 *   Which frame, ordering: the call acts on the planes of the frame drawn last, on the stream rt_denoise uses, also with
 *     RT_FLAG_FRAMES_IN_FLIGHT_2 and after rt_set_stream.  It sees the region as every earlier upload, edit, shape, slab and generated
 *     region left it, and later world changes wait for it.
 *   Side effects: the frame slot's cached prepass is dropped.  No accumulation sum, RT_FLAG_REPROJECT history set or count,
 *     RtCounters, pending edit box or slab changes.
 *   Errors: NULL ctx, NULL u, a NULL array with count > 0, count > 1024: RT_ERR_INVALID_ARG.  tile_world != 1: RT_ERR_UNIMPLEMENTED
 *     (whole-frame contexts only).  No frame drawn yet, or no world resident: RT_ERR_NOT_READY.  count == 0: RT_OK, nothing enqueued.
 *     A rejected call changes nothing.
 *   Device work per call: one launch, a wave per 8x8 pixel tile; per tile the lights pass a conservative sphere-against-bounds cull
 *     64 at a time and only the survivors are tested, and traced, per pixel; the synchronous call adds one transfer.
 * Host pointer; returns when the planes are written. */
int rt_add_lights(RtContext* ctx, const RtUniforms* u, const RtPointLight* lights, uint32_t count);
/* Same with a device pointer, enqueued.  The pointer must pass rt_trace_rays_async's test (16-byte aligned memory of the context's
 * device, or managed memory), else RT_ERR_INVALID_ARG before anything is enqueued.  The library cannot read device records on the
 * host: an invalid light is skipped on the device. */
int rt_add_lights_async(RtContext* ctx, const RtUniforms* u, const RtPointLight* lights_dev, uint32_t count);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Entity shadows: the entities the host drew — the very RtDrawBox and
 * RtDrawStamp records of rt_draw_boxes and rt_draw_stamps — cast the sun's shadow into the frame drawn last: onto the world, onto
 * each other and onto their own averted faces.  The shader's direct sun term of a lit surface is the per-frame constant `sunlight`,
 * with no cosine and no albedo (raytrace.comp:325-328), so the call removes exactly that term, times `strength`, from the pixels an
 * entity shades and the world does not; it holds for one-sample, multi-sample, accumulated and reprojected lighting alike, whose
 * planes hold a mean of samples with a sun term of `sunlight` or 0.  `material`, `emission` and the face lights play no part.  The
 * intended order is boxes, models, shadows, point lights, denoise.
 * The rules.  All arithmetic is fp32 with one rounding per operation; fused operations appear only where rtm_fma or rtm_dot3 is
 * written; any comparison with a NaN is false.  Results are reproduced bit for bit by tests/entity_shadow_ref.py, which tests every
 * occluder against every pixel (DESIGN.md "Entity shadows").
 *   Inputs: sun_angle, origin, forward, up, right and lr of `u` are read; the host passes the uniforms of the frame it drew.  s is the
 *     sun's direction and sunlight its colour, exactly the values the frame uses (raytrace.comp:317-318, sun_color :259-269): s is
 *     normalised once there, and it is NOT jittered as the frame's own shadow rays are.
 *   Surface pixel and its point P': rt_add_lights' rules, word for word — a surface pixel has RT_BUF_NORMAL_R8UI < 6 and
 *     RT_BUF_DEPTH_F32 < 65535.0f; P lies on the ray of rt_draw_boxes at t = depth_f / 32.0f; P' is P moved 0.03125f off its face along
 *     the normal code.  The planes are read as they stand: entity pixels written by rt_draw_boxes / rt_draw_stamps take part with
 *     their own depth and face.  Every other pixel keeps all its bits.
 *   A box shades the pixel: rt_draw_boxes' slab test with o = P', d = s and inv_k = 1.0f / s_k gives t_in and t_out by the same
 *     replacement rules; an axis with s_k == 0 passes iff lo_k < o_k && o_k < hi_k and gives no bound.  The box shades iff some axis
 *     gave a bound, every zero axis passes, t_out > 0 and t_in < t_out.  The one change from the draw rule is t_out > 0 in place of
 *     t_in > 0: a point inside a box is shaded by it (an entity sunk into the ground shades the ground inside it).  An entity's own
 *     pixels have P' 1/32 outside their face: a face turned from the sun re-enters its own box and goes dark, a face turned to the sun
 *     leaves it.  Valid box: rt_draw_boxes'.  The device skips an invalid box in both calls; rt_shadow_entities also rejects the whole
 *     call (RT_ERR_INVALID_ARG) before anything is enqueued.
 *   A model shades the pixel: the bounding box is lo = origin, hi_k = rtm_fma(float(E'_k), scale, origin_k), and the model is entered
 *     iff the box rule above holds for it.  First cell if t_in > 0: rt_draw_stamps' rule — the entry axis a gets c_a = s_a > 0 ? 0 :
 *     E'_a - 1, every other axis c_k = clamp(int(rtm_floor((p - origin_k) / scale)), 0, E'_k - 1) with p = rtm_fma(s_k, t_in, o_k), or
 *     p = o_k when s_k == 0.  First cell if not (P' lies inside the bounding box, or on it): on EVERY axis p = o_k and c_k by the same
 *     clamp.  Then rt_draw_stamps' walk steps (1) to (3) unchanged, with the same plane expression t_k(i) = (rtm_fma(float(i), scale,
 *     origin_k) - o_k) * inv_k, the same tie rule and the same step bound; no t and no axis is tracked.  The model shades iff the walk
 *     stops on an RT_STAMP_SOLID cell.  Valid record: rt_draw_stamps'; an invalid record rejects either call on the host.
 *   Sunlit: a pixel shaded by at least one occluder is CHANGED iff trace_ray (raytrace.comp:82-183) from P' in direction s (trace_ray
 *     normalises it again), with u.lr against the resident region, leaves the window (RT_HIT_AIR).  A hit, the border value, a start
 *     inside an occupied texel and the loop limit all leave the pixel as it is: the world shades it already and there is no sun term
 *     to remove.  (Entities first, the world's ray only for shaded pixels: that order is the cost model's, the result does not depend
 *     on it.)
 *   Writes, only for a changed pixel: sub_k = (sunlight_k * strength) / 16.0f; RT_BUF_LIGHTING_F32.rgb = rtm_max(L_k - sub_k, 0.0f);
 *     independently RT_BUF_LIGHTING_RGBA16.rgb = rtm_unorm(rtm_max(float(q_k) / 65535.0f - sub_k, 0.0f), 65535.0f), q the texel as it
 *     stands.  Both alphas, every other plane and every other pixel keep their bits.  The clamp serves the pixels at a world-shadow
 *     edge, whose frame's jittered sun ray was blocked while the un-jittered one here is not.  As with point lights each plane gets
 *     the change in its own representation: before rt_denoise the shadow's edge is filtered with the rest, after it the edge stays
 *     crisp.
 *   Which frame, ordering: rt_add_lights' — the planes of the frame drawn last, on the stream rt_denoise uses, also with
 *     RT_FLAG_FRAMES_IN_FLIGHT_2 and after rt_set_stream, behind the queries already enqueued on the context.  The call sees the region
 *     as every earlier upload, edit, shape, slab and generated region left it, and later world changes wait for it.
 *   Side effects: the frame slot's cached prepass is dropped.  No accumulation sum, RT_FLAG_REPROJECT history set or count, RtCounters,
 *     pending edit box or slab changes.  The call names its stamps as a draw does: rt_stamp_destroy after an enqueued call waits for it.
 *   Errors: NULL ctx, NULL u, a NULL array with its count above 0, a count above 4096, strength not finite or outside (0, 1], a model
 *     record that is not valid: RT_ERR_INVALID_ARG.  tile_world != 1: RT_ERR_UNIMPLEMENTED.  No frame drawn yet, or no world resident:
 *     RT_ERR_NOT_READY.  nboxes + nmodels == 0, or sunlight == (0, 0, 0): RT_OK, nothing enqueued, no prepass dropped.  (sunlight is
 *     (0, 0, 0) for no sun angle the tests know: below the horizon the shader's sun colour is negative, and the call then removes that
 *     negative term, as the rule says.)  A rejected call changes nothing.
 *   Limits, not bugs: hard shadows only.  The sun only: in rt_add_lights point lights still ignore entities
 *     (rt_add_lights_occluded is the call in which they do not).  No entity shadow in bounce light.  The
 *     shadow belongs to one frame and enters no accumulation sum or history.  Crevices narrower than 1/32 of a model whose voxels are
 *     smaller than 1/16 may shade themselves.
 *   Device work per call: one transfer of a 64-byte record per model and one launch, a wave per 8x8 pixel tile; per tile the boxes and
 *     the models' bounding boxes pass a conservative cull 64 at a time, only the survivors are tested (and walked) per pixel, and only
 *     the shaded pixels trace the world's sun ray; the synchronous call adds one transfer of the boxes.
 * Host pointers; returns when the planes are written. */
int rt_shadow_entities(RtContext* ctx, const RtUniforms* u, const RtDrawBox* boxes, uint32_t nboxes, const RtDrawStamp* models,
                       uint32_t nmodels, float strength);
/* Same, enqueued.  `boxes_dev` is device memory and must pass rt_trace_rays_async's test (16-byte aligned memory of the context's
 * device, or managed memory), else RT_ERR_INVALID_ARG before anything is enqueued; the library cannot read device records on the host:
 * an invalid box is skipped on the device.  `models` is a host pointer here too, as for rt_draw_stamps_async and for the same reason,
 * and is free again when the call returns. */
int rt_shadow_entities_async(RtContext* ctx, const RtUniforms* u, const RtDrawBox* boxes_dev, uint32_t nboxes, const RtDrawStamp* models,
                             uint32_t nmodels, float strength);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Point-light shadows of entities: rt_add_lights with the entities the
 * host drew — the very RtDrawBox and RtDrawStamp records of rt_draw_boxes, rt_draw_stamps and rt_shadow_entities — as occluders.  A
 * torch in the hand, a glowing projectile or an explosion flash is the light a mob standing next to it blocks; indoors and at night
 * it is the only shadow an entity has.  The call stands in rt_add_lights' place in the order boxes, models, sun shadows, lights,
 * denoise.  rt_add_lights itself does not change.
 * The rules.  All arithmetic is fp32 with one rounding per operation; fused operations appear only where rtm_fma or rtm_dot3 is
 * written; any comparison with a NaN is false.  Results are reproduced bit for bit by tests/light_shadow_ref.py, which tests every
 * occluder against every (pixel, light) pair that passed the pair test (DESIGN.md "Point-light shadows of entities").
 *   Everything of rt_add_lights holds word for word: the surface pixel, P', the valid light, the pair test (dist2 > 0 && dist2 < r2 &&
 *     c > 0), the world's shadow ray with its added exit, weight, sum, writes, which frame, ordering and side effects.  One thing is
 *     added to the verdict on a (pixel, light) pair that passed the pair test:
 *   Segment: o = P'; d = rtm_normalize3(v), the direction the world's shadow ray travels in (v times one reciprocal of its length);
 *     inv_k = 1.0f / d_k; len = rtm_sqrt(dist2), the value the weight uses.
 *   A box blocks the pair: rt_shadow_entities' slab rule with this o, d and inv — some axis gave a bound, every d_k == 0 axis passes
 *     (lo_k < o_k && o_k < hi_k), t_out > 0 and t_in < t_out — and also t_in < len.  So a box beyond the light does not shade it, a
 *     surface point inside a box is shaded by it, and a light inside a box lights nothing outside it.  Valid box: rt_draw_boxes'.  The
 *     device skips an invalid box in both calls; rt_add_lights_occluded also rejects the whole call (RT_ERR_INVALID_ARG) before
 *     anything is enqueued.
 *   A model blocks the pair: the bounding box is rt_shadow_entities' (lo = origin, hi_k = rtm_fma(float(E'_k), scale, origin_k)) and is
 *     entered iff the box rule above holds for it, t_in < len included.  The first cell follows rt_shadow_entities' two cases:
 *     entered from outside when t_in > 0, started inside otherwise.  The walk is rt_draw_stamps' steps (1) to (3) with one added stop
 *     between (2) and (3): if the minimum plane time tk of step (2) is not < len, the light lies in the current cell or before its
 *     far plane; the walk stops there and the model does not block.  The model blocks iff the walk stops on an RT_STAMP_SOLID cell; a
 *     solid cell of the same model behind the light does not block.  The step bound E'_x + E'_y + E'_z stays.  Valid record:
 *     rt_draw_stamps'; an invalid record rejects either call on the host.
 *   Verdict: the light is visible at the pixel iff no valid box and no model blocks the pair and rt_add_lights' shadow ray says
 *     visible.  (Entities first, the world's ray only for the pairs no entity blocks: that order is the cost model's, the result does
 *     not depend on it.)
 *   Zero occluders: with nboxes + nmodels == 0 the call is rt_add_lights, every bit and every side effect.
 *   Self-shadowing follows from the rules: a box's own lit faces have c > 0, their segment leaves the box and t_out <= 0 on the
 *     face's axis; a concave model shades itself through the walk; crevices narrower than 1/32 of a model whose voxels are smaller
 *     than 1/16 may shade themselves, as for rt_shadow_entities.
 *   Side effects: rt_add_lights'.  The call names its stamps as a draw does: rt_stamp_destroy after an enqueued call waits for it.
 *   Errors, all checked on the host before anything is enqueued: NULL ctx or u, a NULL `lights` with count > 0, count > 1024, an
 *     invalid light in the synchronous call; for the occluder arrays a NULL array with its count above 0, a count above 4096, a model
 *     record that is not valid, an invalid box in the synchronous call: RT_ERR_INVALID_ARG.  tile_world != 1: RT_ERR_UNIMPLEMENTED.
 *     No frame drawn yet, or no world resident: RT_ERR_NOT_READY.  count == 0: RT_OK, nothing enqueued, no prepass dropped, whatever
 *     the occluder counts.  A rejected call changes nothing.
 *   Limits, not bugs: hard shadows only.  No per-light "owner" exemption: a host that carries a light inside an entity's box leaves
 *     that box out of this call's list.  The light and its shadows belong to one frame and enter no accumulation sum or history.
 *     Bounce light still ignores entities.
 *   Device work per call: one transfer of a 64-byte record per model and one launch, a wave per 8x8 pixel tile; per tile the lights
 *     pass rt_add_lights' cull, the boxes and the models' bounding boxes pass ONE conservative cull against the hull of the tile's
 *     surface points and candidate lights, and only the survivors (up to 64 of a kind; beyond that the tile scans every record) are
 *     tested per pair; the synchronous call adds one transfer of the lights and boxes.
 * Host pointers; returns when the planes are written. */
int rt_add_lights_occluded(RtContext* ctx, const RtUniforms* u, const RtPointLight* lights, uint32_t count, const RtDrawBox* boxes,
                           uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels);
/* Same, enqueued.  `lights_dev` and `boxes_dev` are device memory and must pass rt_trace_rays_async's test (16-byte aligned memory of
 * the context's device, or managed memory), else RT_ERR_INVALID_ARG before anything is enqueued; an invalid light or box is skipped on
 * the device.  `models` is a host pointer here too, as for rt_shadow_entities_async and for the same reason, and is free again when
 * the call returns. */
int rt_add_lights_occluded_async(RtContext* ctx, const RtUniforms* u, const RtPointLight* lights_dev, uint32_t count,
                                 const RtDrawBox* boxes_dev, uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Entity queries: what a ray or a pixel hits among the entities a host
 * draws — clicking a mob, a projectile against it, whether one mob sees another past a third, whether the cursor is on the mob or on
 * the block behind it.  The calls take the records of rt_draw_boxes and rt_draw_stamps and apply their slab test, their walk and
 * their depth test against the world, so the answer for a pixel is exactly the entity those draws put there.  One answer, 48 bytes: */
#define RT_ENTITY_NONE  0
#define RT_ENTITY_BOX   1
#define RT_ENTITY_MODEL 2
typedef struct RtEntityHit {        /* 48 bytes */
    float    position[3];  float t;          /*  0  P_k = rtm_fma(d_k, t, o_k); t along the NORMALISED direction                    */
    uint32_t kind, index, normal, material;  /* 16  RT_ENTITY_*; index into boxes / models; face code 0..5; the box's material word
                                                    or the hit voxel's                                                             */
    int32_t  cell[3];      uint32_t voxel;   /* 32  MODEL: placed-local cell c of the hit, and the hit voxel's index in the stamp's own
                                                    arrays (rt_stamp_read's layout, x + ex (y + ey z))                              */
} RtEntityHit;
/* The rules.  All arithmetic is fp32 with one rounding per operation; fused operations appear only where rtm_fma is written; any
 * comparison with a NaN is false.  Results are reproduced bit for bit by tests/entity_query_ref.py, which tests every entity against
 * every ray (DESIGN.md "Entity queries").
 *   World part: world_hits[i] (where the pointer is not NULL) is exactly what rt_trace_rays writes for the same ray, `lr` and region —
 *     for rt_pick_entities exactly what rt_pick_pixels writes, the slide of a start below the region included — every field, bit for
 *     bit.  The entity part is the same with world_hits NULL.
 *   Entity ray: rt_trace_entities: o = the ray's origin, d = rtm_normalize3(direction).  rt_pick_entities: the ray of rt_draw_boxes —
 *     o = u.origin, the same sx, sy and rtm_normalize3, and NO slide.  In both inv_k = 1.0f / d_k.  A ray whose o or d holds a NaN
 *     hits no entity; that follows from the comparisons and is no special case.
 *   Box b: rt_draw_boxes' valid box and slab test, word for word: the box is hit iff some axis bounds the ray, every zero-direction
 *     axis passes, t_in > 0 and t_in < t_out; the hit's t = t_in and its axis the entry axis.  A ray that starts inside a box does not
 *     hit it, so a mob never hits its own box.
 *   Model m: rt_draw_stamps' valid record, bounding box, planes, first cell and walk, word for word, with the ray's o in place of the
 *     camera's.  The hit's t and axis are the walk's, `cell` the cell c the walk stopped on, `voxel` the index of the stamp voxel that
 *     cell shows and `material` that voxel's word.
 *   Winner: the smallest t over boxes and models together; on equal t boxes come before models, and within each kind the lowest index
 *     wins.
 *   Depth test against the world: P_k = rtm_fma(d_k, t, o_k); depth_f = rtm_length3(o - P) * 32.0f.  D = 65535.0f if the world hit's
 *     kind is RT_HIT_AIR, otherwise D = rtm_length3(o - world position as returned) * 32.0f (store_primary_planes' expression; a limit
 *     exit counts as a hit there, so it does here).  For rt_pick_entities o in both expressions is u.origin, and D is bitwise what
 *     RT_BUF_DEPTH_F32 holds for that pixel in a frame drawn with `u`.  The entity is reported iff depth_f < D: strict, the world wins
 *     ties; a NaN D reports none, and an entity 2048 or more units away under the sky reports none — the draws' own rules.
 *   Record of a reported entity: kind RT_ENTITY_BOX or RT_ENTITY_MODEL; index, position = P and t the winner's; normal = 2 axis + 1 if
 *     d_axis > 0, else 2 axis; material the box's word or the voxel's; for a box cell = (-1, -1, -1) and voxel = 0xFFFFFFFF.
 *   Record otherwise — nothing hit, the hit occluded, or nboxes + nmodels == 0: kind RT_ENTITY_NONE, index = 0xFFFFFFFF, normal = 6,
 *     material = 0, t = 0, position = (0, 0, 0), cell = (-1, -1, -1), voxel = 0xFFFFFFFF.  Every byte of every record is written.
 *   Ordering and side effects: the ray queries' — on the query stream behind the earlier world changes, not behind frames; later
 *     world changes wait for it; after rt_set_stream(non-NULL) on the caller's stream, in order.  No plane, prepass, accumulation sum,
 *     history, RtCounters or RtTiming changes.  The call names its stamps as a draw does: rt_stamp_destroy after an enqueued call
 *     waits for it, and the call itself waits on the device for an earlier rt_stamp_capture, so a stamp captured a moment ago can be
 *     queried with no host sync in between.
 *   Errors, all checked before anything is enqueued (a rejected call changes nothing, outputs included): NULL ctx; NULL rays / xy / u /
 *     lr / entity_hits with count > 0; a NULL entity array with its count above 0; count > 2^24; nboxes or nmodels above 4096; a pixel
 *     outside the frame; a model record that is not valid; in the synchronous calls a box that is not valid (the asynchronous call
 *     cannot read device boxes: the device skips an invalid box); in the asynchronous call a device pointer that fails
 *     rt_trace_rays_async's test: RT_ERR_INVALID_ARG.  No world resident: RT_ERR_NOT_READY (no noise and no drawn frame are needed).
 *     count == 0: RT_OK, nothing enqueued.  Tile contexts answer for whole-frame pixels, as the ray queries do; every RtKernel and
 *     every region size answers the same.
 *   Device work per call: one transfer of a 64-byte record per model and one launch, one lane per ray.  A wave of 64 consecutive rays
 *     culls the entities against the bounds of its rays 64 at a time and tests only the survivors per ray.  Coherent rays — the pixels
 *     of a screen region, a volley of projectiles — are culled well; incoherent rays in one wave are not, and the cost then tends to
 *     rays x entities slab tests.  Send rays that lie together in consecutive order.  There is no acceleration structure over
 *     entities.
 * Arbitrary rays; host pointers; returns when the hits are in host memory. */
int rt_trace_entities(RtContext* ctx, const RtRay* rays, uint32_t count, const int32_t lr[3], const RtDrawBox* boxes, uint32_t nboxes,
                      const RtDrawStamp* models, uint32_t nmodels, RtRayHit* world_hits, RtEntityHit* entity_hits);
/* Same, enqueued.  rays_dev, boxes_dev, world_hits_dev (may be NULL) and entity_hits_dev are device memory and must pass
 * rt_trace_rays_async's test; `models` is a HOST pointer, as for rt_draw_stamps_async and for the same reason, and is free again when
 * the call returns. */
int rt_trace_entities_async(RtContext* ctx, const RtRay* rays_dev, uint32_t count, const int32_t lr[3], const RtDrawBox* boxes_dev,
                            uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels, RtRayHit* world_hits_dev,
                            RtEntityHit* entity_hits_dev);
/* The pixels xy[2 i], xy[2 i + 1] = (x, y), row 0 = the bottom row, of the camera in `u`, as for rt_pick_pixels.  Host pointers,
 * synchronous. */
int rt_pick_entities(RtContext* ctx, const RtUniforms* u, const int32_t* xy, uint32_t count, const RtDrawBox* boxes, uint32_t nboxes,
                     const RtDrawStamp* models, uint32_t nmodels, RtRayHit* world_hits, RtEntityHit* entity_hits);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Entity sweeps: rt_sweep_boxes' box swept against the resident world
 * AND the entities a host draws, so that what is drawn is solid too — a player stands on the moving platform and stops at the door
 * that rt_draw_stamps shows, mobs drawn by rt_draw_boxes do not walk through one another, a projectile box meets the mob and not only
 * the voxels behind it.  The calls take rt_sweep_boxes' sweeps and the records of rt_draw_boxes and rt_draw_stamps.  One answer about
 * the entities, five 16-byte words, 80 bytes: */
typedef struct RtEntitySweepHit {     /* 80 bytes */
    float    t;  uint32_t kind;  uint32_t normal;  uint32_t material;   /*  0  fraction travelled; RT_SWEEP_*; face code; the box's material
                                                                                word or the cell's voxel word                             */
    uint32_t entity, index, axis, voxel;     /* 16  RT_ENTITY_NONE / BOX / MODEL; index into boxes / models; blocked axis 0..2, else 3;
                                                    MODEL: the cell's voxel index in the stamp's own arrays (rt_stamp_read's layout)      */
    int32_t  cell[3];  uint32_t reserved0;   /* 32  MODEL: the placed-local cell c; otherwise (-1, -1, -1)                               */
    float    lo[3];    uint32_t reserved1;   /* 48  the box where the COMBINED sweep ended: the next sweep's box                         */
    float    hi[3];    uint32_t reserved2;   /* 64  (the reserved words are written as 0)                                                */
} RtEntitySweepHit;
/* The rules.  All arithmetic is fp32 with one rounding per operation; fused operations appear only where rtm_fma is written; any
 * comparison with a NaN is false.  Results are reproduced bit for bit by tests/sweep_entities_ref.py, which tests every box and every
 * SOLID cell of every model against every sweep (DESIGN.md "Entity sweeps").
 *   World part: world_hits[i] (where the pointer is not NULL) is exactly what rt_sweep_boxes writes for the same record, `lr` and
 *     region, every field, bit for bit: W.  The validated domain of a sweep is rt_sweep_boxes'.  The entity part is the same with
 *     world_hits NULL.
 *   Self exemption: in these calls RtBoxSweep.reserved0 is read: a value s in 1..nboxes makes the sweep ignore box s - 1, any other
 *     value ignores none.  reserved1 does the same for models.  A mob swept against the list that holds its own box needs this:
 *     without it every mob is EMBEDDED in itself.  reserved2 stays ignored.
 *   One obstacle box O = [olo, ohi] against the sweep (lo, hi, motion m).  A box b is an obstacle iff it is valid by rt_draw_boxes'
 *     rule; the device skips an invalid box, rt_sweep_entities also rejects the whole call.  Per axis k the sweep overlaps O at the
 *     start iff lo_k < ohi_k && olo_k < hi_k: strict, touching is not overlap.  Moving + (m_k > 0): te_k = (olo_k - hi_k) / m_k and
 *     tx_k = (ohi_k - lo_k) / m_k; moving - (m_k < 0): te_k = (ohi_k - lo_k) / m_k and tx_k = (olo_k - hi_k) / m_k; each is one
 *     subtraction and one IEEE division.  An axis with m_k == 0 (either sign) is not moving and has no times.  O EMBEDS the sweep iff
 *     every axis overlaps at the start.  Otherwise let a be the moving axis with the largest te_k, the HIGHEST axis on equal values:
 *     O BLOCKS at t = te_a on axis a iff every axis that is not moving overlaps at the start, te_a >= 0, te_a < 1, and te_a < tx_k on
 *     every moving axis.  This is the world's event order restated per obstacle — trailing events come before leading events at equal
 *     t, then the order is x, y, z — so a corner met exactly blocks on the later axis and a face that is only touched does not catch:
 *     with every occupied voxel v taken as the box [v, v + 1] the rule gives rt_sweep_boxes' kind, t, axis and voxel.
 *   One model: a valid record by rt_draw_stamps' rule, with its planes: plane_k(i) = rtm_fma(float(i), scale, origin_k), i = 0..E'_k.
 *     Placed-local cell c is the obstacle box [plane_k(c_k), plane_k(c_k + 1)] and exists iff the stamp voxel it shows has state
 *     RT_STAMP_SOLID; a cell with two equal planes on some axis (far from the origin rounding merges planes) is absent.  A model is
 *     nothing but its cells under the obstacle rule.  Within one model the blocking cell is the one with the smallest t, then the
 *     lowest blocked axis, then the first in ascending (z, y, x) order of c; a model embeds iff some cell does, and reports the first
 *     such cell in that order.
 *   Entity part: EMBEDDED beats BLOCKED: the first embedding obstacle in the order boxes by index, then models by index.  Otherwise the
 *     smallest t; on equal t boxes come before models, and within a kind the lowest index wins.  The t reported is the winner's own
 *     te_a, bit for bit (0 / m_a is -0 for a touching start moving -: it compares equal to 0 and stays -0, as in rt_sweep_boxes).
 *   What is reported.  W is INVALID: kind = RT_SWEEP_INVALID, t = 0, the rest as for "nothing" below, lo / hi = the input bits.  The
 *     entity part is EMBEDDED: reported whatever W is: kind = RT_SWEEP_EMBEDDED, t = 0, axis = 3, normal = 6, lo / hi = the input bits.
 *     The entity part is BLOCKED at t_e: reported iff W is FREE or BLOCKED and t_e < W.t: strict, the world wins ties.  A reported
 *     record holds entity = RT_ENTITY_BOX or RT_ENTITY_MODEL, index, material = the box's material word or the cell's voxel word; for a
 *     model cell = c and voxel = the index of the stamp voxel the cell shows; for a box cell = (-1, -1, -1) and voxel = 0xFFFFFFFF.
 *     Nothing reported: kind = RT_SWEEP_FREE, entity = RT_ENTITY_NONE, index = 0xFFFFFFFF, t = 1, axis = 3, normal = 6, material = 0,
 *     voxel = 0xFFFFFFFF, cell = (-1, -1, -1), lo / hi = W's returned lo / hi — also when W is BLOCKED or EMBEDDED: the world's own
 *     answer is world_hits'.  In every case entity_hits[i].lo / hi is the next sweep's box.  Every byte of every record is written.
 *   Returned box of a reported block: rt_sweep_boxes' "Returned box" rule at t = t_e, with the cell ranges c as they stand after every
 *     world event with time < t_e (none of them blocked, because t_e < W.t).  On the blocked axis a, with F the obstacle's near face
 *     (olo_a moving +, ohi_a moving -; for a cell the plane) and size = hi_a - lo_a: moving + hi' = F, lo' = max(F - size,
 *     float(c.lo_a)); moving - lo' = F, hi' = min(F + size, float(c.hi_a + 1)).  normal = 2 a + 1 moving +, 2 a moving -.  The clamps
 *     close the contract against the world: the returned box, swept again on an unchanged world, is never world-EMBEDDED.  Against
 *     the entities only the blocker is covered: the snapped face touches it and does not overlap it, but the rounding of the other
 *     axes may graze a second entity.  Entities move between calls, so a host handles entity-EMBEDDED in any case.
 *   Limits: count <= 2^24; nboxes, nmodels <= 4096.
 *   Ordering and side effects: rt_trace_entities' — on the query stream behind the earlier world changes, not behind frames; later
 *     world changes wait for it; after rt_set_stream(non-NULL) on the caller's stream, in order.  No plane, prepass, accumulation sum,
 *     history, RtCounters or RtTiming changes.  The call names its stamps as a draw does: rt_stamp_destroy after an enqueued call
 *     waits for it, and the call itself waits on the device for an earlier rt_stamp_capture, so a stamp captured a moment ago can be
 *     swept against with no host sync in between.
 *   Errors, all checked before anything is enqueued (a rejected call changes nothing, outputs included): NULL ctx; NULL sweeps / lr /
 *     entity_hits with count > 0; a NULL entity array with its count above 0; count > 2^24; nboxes or nmodels above 4096; a model
 *     record that is not valid; in the synchronous call a sweep outside the validated domain or a box that is not valid (the
 *     asynchronous call cannot read device records: the device answers RT_SWEEP_INVALID and skips an invalid box); in the
 *     asynchronous call a device pointer that fails rt_trace_rays_async's test: RT_ERR_INVALID_ARG.  No world resident:
 *     RT_ERR_NOT_READY.  count == 0: RT_OK, nothing enqueued.  Every RtKernel and every region size answers the same.
 *   Device work per call: one transfer of a 64-byte record per model and one launch, one lane per sweep.  A wave of 64 consecutive
 *     sweeps culls the entities against the bounds of its sweeps 64 at a time; a lane tests a surviving box once and a surviving
 *     model once per cell of the part its own swept hull reaches.  Sweeps that lie together belong in consecutive order.  Worst case:
 *     a tiny-scale model under a large box — scale 2^-8 under an 8-unit box puts up to 256^2 cells in every layer the sweep crosses,
 *     and 256 layers; keep collision models coarse.
 *   Out of scope: entities are no obstacles of rt_step_particles; entities do not move against one another during the call (every
 *     obstacle stands still for the sweep); entities are not rotated; there is no acceleration structure over entities.
 * Host pointers; returns when the hits are in host memory.  world_hits may be NULL. */
int rt_sweep_entities(RtContext* ctx, const RtBoxSweep* sweeps, uint32_t count, const int32_t lr[3], const RtDrawBox* boxes, uint32_t nboxes,
                      const RtDrawStamp* models, uint32_t nmodels, RtSweepHit* world_hits, RtEntitySweepHit* entity_hits);
/* Same, enqueued.  sweeps_dev, boxes_dev, world_hits_dev (may be NULL) and entity_hits_dev are device memory and must pass
 * rt_trace_rays_async's test; `models` is a HOST pointer, as for rt_trace_entities_async and for the same reason, and is free again
 * when the call returns. */
int rt_sweep_entities_async(RtContext* ctx, const RtBoxSweep* sweeps_dev, uint32_t count, const int32_t lr[3], const RtDrawBox* boxes_dev,
                            uint32_t nboxes, const RtDrawStamp* models, uint32_t nmodels, RtSweepHit* world_hits_dev,
                            RtEntitySweepHit* entity_hits_dev);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) Terrain generated on the device: the project's deterministic
 * procedural world (raytrace_amd/host/world.cpp: generate_chunk + pack_into per world chunk, MATERIALS[id].pack()) written straight
 * into the resident region, byte for byte what the host generator assembles — no host bytes, no staging, no transfer.
 *   Window: the world box each call writes.  rt_generate_world writes [lo, lo + R) on every axis (window_lo NULL = (-R/2, -R/2, -R/2),
 *     the region of world.generate_region); rt_generate_slice writes [lo_m, lo_m + 16) on `axis` m (0/1/2 = x/y/z) and [lo_a, lo_a + R)
 *     on the other two.  World voxel v lands at texel (v + R/2) mod R on each axis: the addressing of rt_upload_slice and
 *     TerrainUploadManager (a streamer's request origin[a]*64 + num_slices[a]*16 is its window_lo).  Each voxel takes the minefield of
 *     its own world chunk, also where a window that is not 64-aligned puts pieces of two chunks in one 64-texel block.
 *   Content: rt_generate_world(seed, NULL) equals rt_upload_world of world.generate_region(seed, R); any window equals rt_upload_world
 *     of world.toroidal_region(lo + R/2, seed, R); rt_generate_slice leaves the region as rt_upload_slice of the host manager's slab.
 *     Heights are FP64 with the host's operations in the host's order (DESIGN.md "Terrain on the device": the margin of pow).
 *   Nibble maps: rt_generate_world rebuilds every word; rt_generate_slice the words its slab touches, as rt_upload_slice does.
 *   Validation, before anything is enqueued (a rejected call changes nothing): window_lo not a multiple of 16, a window voxel outside
 *     int32 (RtUniforms.lr is int32), axis outside 0..2 or window_lo NULL (slice): RT_ERR_INVALID_ARG.  rt_generate_slice without a
 *     resident world: RT_ERR_NOT_READY.
 *   Ordering: asynchronous and stream-ordered like rt_upload_slice — after every frame already submitted on every lane and frame slot
 *     and after earlier queries; later frames, queries and edits see the new region; the host waits for nothing.  Works on a stream
 *     set with rt_set_stream and on tile-split contexts.  Resets RT_FLAG_ACCUMULATE's running sum (rt_generate_slice: unless
 *     RtConfig.stream_history keeps the history, as for rt_upload_slice).  rt_generate_world makes the world
 *     resident: a context may start from it with no rt_upload_world at all.
 * Device work per call: heights of the window's chunk columns, one workgroup per world chunk in the window that writes its voxels, one
 * launch that rebuilds the nibble-map words (counted by RT_FLAG_TIMING_ALL as one launch); scratch of (R + 64)^2 int32 on first use. */
int rt_generate_world(RtContext* ctx, uint64_t seed, const int64_t window_lo[3]);
int rt_generate_slice(RtContext* ctx, uint64_t seed, int axis, const int64_t window_lo[3]);

/* Allocation figures of the context (see RtInfo). */
int rt_get_info(RtContext* ctx, RtInfo* out);

/* (ABI 1.2) The launch-sizing rule behind RtInfo.samples_per_launch, as a pure function (no device needed): samples of every
 * pixel one path-kernel launch covers when `lane_bytes` are given to the 12-byte light records of ONE launch (the context's
 * budget divided by its launches in flight, RtInfo.launches_in_flight) and the frame queues `npix` pixels: at most 2^31 paths,
 * at most `spp`, at least 1; `env_batch` (the RT_PERSIST_BATCH string, or NULL) may only lower it. */
uint64_t rt_samples_per_launch(uint64_t lane_bytes, uint64_t npix, uint64_t spp, const char* env_batch);

/* Blue-noise table (render_data.rs:110-133; decoded by structures.rs:496-517): RGBA8 512x512. */
int rt_upload_noise(RtContext* ctx, const uint8_t* rgba8);

/* UBO write + queue submit of the raytrace dispatch (pipeline.rs:195-211,229-235; dispatch :86-90).
 * Asynchronous: returns after enqueue on the context's stream. */
int rt_draw_frame(RtContext* ctx, const RtUniforms* uniforms);

/* Fence wait (pipeline.rs:162-172). */
int rt_sync(RtContext* ctx);

/* Copy an output plane to host memory (synchronises first). bytes must equal rt_buffer_bytes. */
int rt_readback(RtContext* ctx, int buffer_id, void* dst, size_t bytes);

/* Size in bytes of an output plane for this context (tile-major planes are padded to whole tiles). */
size_t rt_buffer_bytes(RtContext* ctx, int buffer_id);

/* Device pointer of an output plane for zero-copy consumers (denoise/finalize, RCCL gather);
 * the images bound at descriptor_sets.rs:64-84. NULL on bad id. */
void* rt_device_ptr(RtContext* ctx, int buffer_id);

/* Run on a caller-provided hipStream_t.  NULL = the context's own non-blocking stream (NOT the legacy null stream: work on
 * the null stream is not ordered against the context's frames). */
int rt_set_stream(RtContext* ctx, void* hip_stream);

/* Multi-GPU tile split: number of 8x8 tiles this context renders, and the padded
 * per-rank tile capacity ceil(total_tiles / tile_world) used for equal-size gathers. */
int rt_tile_count(RtContext* ctx);
int rt_tile_capacity(RtContext* ctx);

/* Scatter `world` gathered tile-major planes (rank-major: world x capacity x 64 px x bpp, device
 * memory) into a row-major full-frame plane (device memory) on this context's stream. */
int rt_untile(RtContext* ctx, int buffer_id, const void* gathered_dev, int world, void* frame_dev);

/* The six reference-format planes (ids 0..5) of a context are one contiguous device block (each plane padded to 256 B),
 * so a multi-GPU host gathers a frame with ONE collective: rt_gbuffer_ptr/bytes give the block, rt_gbuffer_offset the
 * start of plane `id` inside it.  rt_untile_gbuffer scatters `world` gathered blocks (rank-major, device memory) into six
 * row-major full-frame planes frames_dev[0..5] (device pointers; NULL entries are skipped).  `world` must be the
 * context's own tile_world (>= 2): the block layout is the context's. */
void*  rt_gbuffer_ptr(RtContext* ctx);
size_t rt_gbuffer_bytes(RtContext* ctx);
size_t rt_gbuffer_offset(RtContext* ctx, int buffer_id);
int rt_untile_gbuffer(RtContext* ctx, const void* gathered_dev, int world, void* const* frames_dev);

/* The six bilateral_denoise.comp dispatches recorded at pipeline.rs:98-115 (sizes 1,2,4,8,8,16, ping/pong descriptor
 * sets): filters RT_BUF_LIGHTING_RGBA16 in place using the depth and normal planes.  faithful != 0 reproduces the
 * reference's pong descriptor set, which binds the normal and depth images swapped (descriptor_sets.rs:38-39 vs :31-32), so
 * passes 2, 4 and 6 only filter pixels whose DEPTH value is below 16; faithful == 0 binds them consistently.
 * Whole-frame contexts only (tile_world == 1): a 3*16-pixel halo is needed, so gather first. Asynchronous. */
int rt_denoise(RtContext* ctx, int faithful);

/* finalize.comp (pipeline.rs:117-123): albedo*light*16 + emission*4, distance fog, tone curve, blue-noise dither, Y flip
 * -> RT_BUF_FINAL_BGRA8.  Whole-frame contexts only. Asynchronous. */
int rt_finalize(RtContext* ctx);

/* Multi-GPU frame assembly behind the boundary (the reference is single-GPU, this replaces nothing of it): every
 * rank renders the tiles t % tile_world == tile_rank of the frame (RtConfig) and calls rt_gather_gbuffer on its context: the
 * six reference-format planes of every rank travel to `root` over RCCL (grouped ncclSend/ncclRecv on the context's stream, so
 * the transfer is ordered after the frame's kernels without any host synchronisation) and the root scatters them into the six
 * row-major full-frame device planes frames_dev[0..5] (NULL entries are skipped; ignored on the other ranks; a NULL array
 * selects planes the library owns, see rt_frame_ptr).  With
 * overlapped != 0 the transfer and the un-tiling run on a second stream from a staging copy, so the caller may draw the next
 * frame at once; rt_sync waits for both streams.  tile_world == 1: plain copies.  `comm` is an ncclComm_t over the tile_world
 * ranks in tile_rank order — from the host's own RCCL, or from the helpers below (librccl is loaded on first use only):
 *   rt_comm_unique_id   ncclGetUniqueId into a 128-byte buffer (one rank; the host distributes it)
 *   rt_comm_init_rank   ncclCommInitRank(tile_world, id, tile_rank) on the context's device (one process per GPU)
 *   rt_comm_init_all    ncclCommInitAll for one process that drives ndev devices (rt_bench --gpus N)
 *   rt_comm_destroy     ncclCommDestroy */
int rt_comm_unique_id(void* id_out, size_t bytes);
int rt_comm_init_rank(RtContext* ctx, const void* id, size_t bytes, void** comm_out);
int rt_comm_init_all(int ndev, const int* devices, void** comms_out);
int rt_comm_destroy(void* comm);
int rt_gather_gbuffer(RtContext* ctx, void* comm, int root, void* const* frames_dev, int overlapped);
/* frames_dev == NULL on the root: the frame is assembled in planes the library owns (W x H, reference formats, row-major),
 * so a host needs no device allocator of its own: rt_frame_ptr returns plane `id` (0..5; NULL before the first such gather)
 * for rt_denoise_planes / rt_finalize_planes, rt_frame_readback copies it to host memory after waiting for the gather. */
void* rt_frame_ptr(RtContext* ctx, int buffer_id);
int rt_frame_readback(RtContext* ctx, int buffer_id, void* dst, size_t bytes);

/* The same two passes on caller-owned row-major device planes of cfg.width x cfg.height pixels in the reference formats
 * (e.g. the frame rt_untile_gbuffer assembled on rank 0 from the ranks' tiles): rt_denoise_planes filters `lighting_rgba16`
 * in place, rt_finalize_planes writes `out_bgra8` (4 B/px, rows top-down).  Valid on any context, tile-split or not; the
 * context supplies the stream, the blue-noise texture and the working memory.  Asynchronous. */
int rt_denoise_planes(RtContext* ctx, void* lighting_rgba16, const void* depth_r16, const void* normal_r8, int faithful);
int rt_finalize_planes(RtContext* ctx, const void* albedo_rgba8, const void* emission_rgba8, const void* fog_rgba8,
                       const void* lighting_rgba16, const void* depth_r16, void* out_bgra8);

/* (ABI 1.3, additive; hosts detect the feature by these symbols) History-aware denoise: the six dispatches of rt_denoise with the
 * per-pixel sample counts of RT_FLAG_REPROJECT taken into account, so that a pixel with a long history is not blurred as hard as one
 * disoccluded this frame.  With m(p) = min(max(count(p), 1), 127), dispatch i (tap spacings 1, 2, 4, 8, 8, 16) is dispatch i of
 * rt_denoise -- same spacing, same binding rule for `faithful` -- with two changes:
 *   settle   when settle[i] != 0 and m(p) >= settle[i], pixel p takes the shader's copy branch in dispatch i: its working value
 *            passes through unchanged, whatever its normal / depth binding says.  It is still read as a tap by its neighbours.
 *   weight   with weight_by_count = 1 the centre starts from total_weight = 0.146634f * (float)m(c) and sum = L_c * total_weight,
 *            and each tap's weight is the existing quotient times (float)m(tap): one fp32 multiply behind the division, whose
 *            domain (RT_SELFTEST_DENOISE_DIVISION) is unchanged.
 * The fma accumulation, the tap order, the UNORM16 quantisation between dispatches and the alpha rule are rt_denoise's: alpha is
 * 65535 once any dispatch filtered the pixel, else the original texel's.  Neutral parameters -- weight_by_count = 0 with settle all
 * 0, or weight_by_count = 1 with every count equal to 1 -- give rt_denoise's bits exactly.  Same seven launches and working memory.
 * A block with a wrong struct_size, settle[i] > 127, weight_by_count outside 0 / 1 or a non-zero reserved word, or a NULL block, is
 * RT_ERR_INVALID_ARG, and nothing is enqueued. */
typedef struct RtDenoiseParams {   /* 48 bytes */
    uint32_t struct_size;          /* sizeof(RtDenoiseParams) */
    int32_t  faithful;             /* as rt_denoise: odd dispatches use the pong binding */
    int32_t  weight_by_count;      /* 0 / 1 */
    uint32_t settle[6];            /* per dispatch: 0 = nobody settles; 1..127 = pixels with m >= it are left alone */
    uint32_t reserved[3];          /* must be 0 */
} RtDenoiseParams;
/* Filters RT_BUF_LIGHTING_RGBA16 of the frame drawn last in place, like rt_denoise, with the counts that frame's pass wrote (what
 * rt_read_history returns).  The history sums, the counts and RT_BUF_LIGHTING_F32 are not touched.  Asynchronous, on rt_denoise's
 * stream; the counts are read before any later frame overwrites them, with two frames in flight too.  RT_ERR_UNIMPLEMENTED on a
 * tile-split context, RT_ERR_INVALID_ARG on one without RT_FLAG_REPROJECT, RT_ERR_NOT_READY before the first frame. */
int rt_denoise_history(RtContext* ctx, const RtDenoiseParams* params);
/* The same on caller-owned planes (as rt_denoise_planes) plus a row-major u32 device plane of width x height counts: the route for a
 * gathered multi-GPU frame.  Valid on any context. */
int rt_denoise_planes_counted(RtContext* ctx, void* lighting_rgba16, const void* depth_r16, const void* normal_r8,
                              const uint32_t* counts_dev, const RtDenoiseParams* params);

/* The traversal implementation the context runs: the kernel of a frame's last launch, the same before the first frame and after
 * it.  The choice is fixed per context when it is created (launch size, primary cache, region, depth, accumulation); a cached
 * frame of depth 0, which has no path launch, reports RT_KERNEL_PATHS or RT_KERNEL_PERSISTENT as configured.  Negative RtStatus on
 * a null context. */
int rt_kernel_in_use(RtContext* ctx);

/* Device self-tests.  RT_SELFTEST_DENOISE_DIVISION: the denoise passes compute weight / (distance + normal + 1)
 * (bilateral_denoise.comp:31) with a reciprocal and one residual correction; *result = number of quotients, over the complete
 * domain of that expression (37 weights x 131072 denominators), that differ from IEEE division on this device (expected 0). */
#define RT_SELFTEST_DENOISE_DIVISION 1
/* (ABI 1.3, additive) RT_SELFTEST_SCENE_MAPS: rebuilds every word of the coarse nibble map (and of the brick map above R = 256) from the
 * resident minefield; *result = number of words that differ from the resident maps (expected 0; RT_ERR_NOT_READY without a world). */
#define RT_SELFTEST_SCENE_MAPS 2
int rt_selftest(RtContext* ctx, int which, uint64_t* result);

/* (ABI 1.3, additive; hosts detect the feature by this symbol) RT_FLAG_ACCUMULATE: the next rt_draw_frame starts the running sum
 * from zero.  No effect on a context without the flag. */
int rt_reset_accumulation(RtContext* ctx);
/* Frames and samples the lighting planes of the frame drawn last hold: (k, k x spp) after k frames of an accumulation; 1 and spp
 * on a context without RT_FLAG_ACCUMULATE; 0 and 0 before the first frame.  Host-side state only: does not synchronise.
 * RT_FLAG_REPROJECT: frames = frames since the history last started from zero (a camera change does not restart it); samples = the
 * upper bound of any pixel's count: s + 1 after a still frame, min(s, history_cap) + 1 after a moved one. */
int rt_get_accumulation(RtContext* ctx, uint32_t* frames, uint32_t* samples);
/* (ABI 1.3, additive; hosts detect the feature by this symbol) RT_FLAG_REPROJECT: the per-pixel sample counts behind the lighting of
 * the frame drawn last, width x height u32, row-major, row 0 = bottom.  Synchronises first; bytes must equal width x height x 4;
 * RT_ERR_INVALID_ARG on a context without the flag; all zero before the first frame.  For tests, and for a host that wants to
 * denoise harder where the history is short. */
int rt_read_history(RtContext* ctx, uint32_t* counts, size_t bytes);
/* (ABI 1.3, additive; hosts detect the feature by this symbol) RtConfig.edit_radius > 0: *boxes = the edited boxes that wait for
 * the next rt_draw_frame (0..16; one per 64^3 chunk an rt_edit_voxels call touched), *overflowed = 1 when a call would have passed
 * 16, so that the set was emptied and the next frame restarts the history.  An upload, rt_generate_*, rt_upload_noise and
 * rt_reset_accumulation drop both; the next frame consumes both.  Host-side state only: does not synchronise.  0 and 0 on a
 * context without the feature. */
int rt_edit_boxes_pending(RtContext* ctx, uint32_t* boxes, uint32_t* overflowed);
/* (ABI 1.3, additive; hosts detect the feature by this symbol) RtConfig.stream_history = 1: *slabs = the slabs that wait for the next
 * rt_draw_frame (0..4; one per accepted rt_upload_slice / rt_generate_slice), *overflowed = 1 when a call would have needed a fifth
 * slot, so that the set was emptied and the next frame restarts the history.  rt_upload_world, rt_generate_world, rt_upload_noise
 * and rt_reset_accumulation drop both; the next frame consumes both; a rejected slab changes neither.  Host-side state only: does
 * not synchronise.  0 and 0 on a context without the feature. */
int rt_slabs_pending(RtContext* ctx, uint32_t* slabs, uint32_t* overflowed);
/* (ABI 1.3, additive) The world boxes the pending slabs of the frame drawn last produced on the device: boxes[8][6] = lo x y z, hi
 * x y z ([first voxel, last voxel + 1], per slab in call order what left, then what arrived; contents without an occupied voxel give
 * none), *count = how many (0..8) — 0 when that frame had no pending slab or restarted.  Waits for the frame.  RT_ERR_INVALID_ARG on
 * a context without the feature.  For tests, and for a host that wants to show the boxes. */
int rt_read_slab_boxes(RtContext* ctx, float* boxes, uint32_t* count);

int rt_get_counters(RtContext* ctx, RtCounters* out);
int rt_reset_counters(RtContext* ctx);
int rt_get_timing(RtContext* ctx, RtTiming* out);
/* (ABI 1.2) Device time of the rt_gather_gbuffer calls since the previous call of this function: *ms_sum = sum over the calls of
 * (transfer + un-tile), from HIP events recorded round them on the stream they run on, *calls = how many.  On a rank that is
 * not the root the time includes waiting for the root to post its receive.  Contexts created with RT_FLAG_TIMING; otherwise 0, 0.
 * Waits for the context's streams. */
int rt_get_gather_timing(RtContext* ctx, float* ms_sum, uint32_t* calls);

/* Library/ABI version: (major<<16)|minor.  History of the minor version (a host bound against an older header keeps working
 * within a major version; it cannot rely on what a later minor added):
 *   1.0  rounds 1-2.
 *   1.1  round 3: rt_slice_staging, rt_get_info / RtInfo; RtKernel value 4 (PERSISTENT2) rejected by rt_create; RtTiming.frame_ms
 *        is 0 unless RT_FLAG_TIMING_ALL; rt_upload_slice asynchronous, validates on the host BEFORE applying, and a rejected slab
 *        no longer makes rt_draw_frame fail.
 *   1.2  round 4: RT_FLAG_FRAMES_IN_FLIGHT_2; RtInfo.launches_in_flight / frames_in_flight (in the former `reserved` word);
 *        rt_samples_per_launch, rt_get_gather_timing; RtKernel value 6 (SEQ) rejected by rt_create; the sample batches of a multi-launch frame run on two
 *        streams of the library (results unchanged; rt_set_stream(non-NULL) keeps everything on the caller's stream).
 *   1.3  round 4: RtKernel value 7 (RT_KERNEL_FRAME); RT_KERNEL_DEFAULT runs frames with little work on it (rt_kernel_in_use tells);
 *        results unchanged.
 *        Additive, same minor version: RT_FLAG_ACCUMULATE, rt_reset_accumulation, rt_get_accumulation (progressive accumulation).
 *        Additive, same minor version: RtVoxelEdit, rt_edit_voxels, rt_read_box, RT_SELFTEST_SCENE_MAPS (sparse voxel edits).
 *        Additive, same minor version: RtRay, RtRayHit, RT_HIT_*, rt_trace_rays, rt_trace_rays_async, rt_pick_pixels (ray queries).
 *        Additive, same minor version: rt_generate_world, rt_generate_slice (terrain generated on the device).
 *        Additive, same minor version: RT_FLAG_REPROJECT, RtConfig.history_cap (was reserved[0]), rt_read_history (temporal
 *        reprojection of the accumulated lighting while the camera moves).
 *        Additive, same minor version: RtConfig.edit_radius (was reserved[0]), rt_edit_boxes_pending (the lighting history is kept
 *        across rt_edit_voxels and restarted only near an edit or in its sun shadow).
 *        Additive, same minor version: RtConfig.stream_history (was reserved[0]), rt_slabs_pending, rt_read_slab_boxes (the lighting
 *        history is kept across rt_upload_slice / rt_generate_slice and restarted only near what left or arrived).
 *        Additive, same minor version: RtLightProbe, RtProbeLight, RT_PROBE_SPHERE, rt_probe_light, rt_probe_light_async (light
 *        probes: path-traced light at arbitrary points).
 *        Additive, same minor version: RtDenoiseParams, rt_denoise_history, rt_denoise_planes_counted (history-aware denoise:
 *        converged pixels settle, taps may be weighted by their sample counts).
 *        Additive, same minor version: RtBoxSweep, RtSweepHit, RT_SWEEP_*, rt_sweep_boxes, rt_sweep_boxes_async (box sweeps: collision
 *        queries against the resident world).
 *        Additive, same minor version: RtShapeEdit, RT_SHAPE_*, RT_WHERE_*, rt_edit_shapes (shape edits: boxes and spheres filled
 *        or carved on the device).
 *        Additive, same minor version: RtDrawBox, rt_draw_boxes, rt_draw_boxes_async (entity boxes composited into the G-buffer by
 *        depth).
 *        Additive, same minor version: RtPointLight, rt_add_lights, rt_add_lights_async (point lights added to the lighting planes
 *        through one shadow ray per pixel and light).
 *        Additive, same minor version: RtStampPlace, RT_STAMP_*, rt_stamp_create, rt_stamp_capture, rt_stamp_info, rt_stamp_read,
 *        rt_stamp_destroy, rt_edit_stamps (voxel stamps: prefabs captured and pasted with rotation on the device).
 *        Additive, same minor version: RtDrawStamp, rt_draw_stamps, rt_draw_stamps_async (voxel-model entities: stamps drawn at
 *        float positions and scales, composited into the G-buffer by depth).
 *        Additive, same minor version: rt_shadow_entities, rt_shadow_entities_async (entity shadows: drawn boxes and models take the
 *        sun's direct term out of the lighting planes where they shade a pixel).
 *        Additive, same minor version: RtEntityHit, RT_ENTITY_*, rt_trace_entities, rt_trace_entities_async, rt_pick_entities (entity
 *        queries: what a ray or a pixel hits among the drawn boxes and models, under the draws' own rules).
 *        Additive, same minor version: rt_add_lights_occluded, rt_add_lights_occluded_async (point-light shadows of entities:
 *        rt_add_lights with the drawn boxes and models blocking the segment from a pixel's surface point to the light).
 *        Additive, same minor version: RtParticle, rt_draw_particles, rt_draw_particles_async (particles: up to 2^20 small cubes
 *        composited into the G-buffer by depth, binned to the tiles they cover).
 *        Additive, same minor version: RtParticleState, RtParticleStep, RT_PARTICLE_*, RT_PSTATE_*, rt_step_particles, rt_step_particles_async
 *        (particle simulation: a tick of integration, sub-sweeps, contact response and ageing on the device).
 *        Additive, same minor version: RtEntitySweepHit, rt_sweep_entities, rt_sweep_entities_async (entity sweeps: box sweeps that
 *        collide with the drawn boxes and models as well as with the world).
 *        Additive, same minor version: RtParticleEmit, RtEmitCursor, rt_emit_particles, rt_emit_particles_async (particle emitters:
 *        debris spawned on the device from the occupied voxels of a shape, into a ring of particle states).
 *        Additive, same minor version: RtParticleDeposit, RtDepositCount, rt_deposit_particles, rt_deposit_particles_async (particle
 *        deposits: particles at rest become voxels of the region on the device).
 *        Additive, same minor version: RtVoxelSettle, RtSettleCount, rt_settle_voxels, rt_settle_voxels_async (voxel settling: loose
 *        voxels fall along an axis inside a box of texels on the device).
 *        Additive, same minor version: RtVoxelDetach, RtDetachResult, RT_DETACH_*, rt_detach_voxels, rt_detach_voxels_async (voxel
 *        detachment: the unsupported voxels of a box of texels are found, carved and captured into a stamp on the device).
 *        Additive, same minor version: RtNavBuild, RtNavGoal, RtNavResult, RtNavAgent, RtNavStep, RT_NAV_*, rt_nav_create, rt_nav_info,
 *        rt_nav_read, rt_nav_destroy, rt_nav_build, rt_nav_build_async, rt_nav_sample, rt_nav_sample_async (navigation fields:
 *        walking distances to goals and the next move, built and sampled on the device).
 *        Additive, same minor version: RtVoxelFlow, RtFlowCount, rt_flow_voxels, rt_flow_voxels_async (fluid flow: a level-based
 *        fluid spreads, falls and dries inside a box of texels on the device). */
#define RT_ABI_VERSION_MAJOR 1
#define RT_ABI_VERSION_MINOR 3
uint32_t rt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_ABI_H */
