// render.hpp — C++ host mirror of the reference's `render` public API for the ray-trace path:
// Camera (src/render/mod.rs:20-34), create_instance (mod.rs:36-43), Pipeline::{new, draw_frame, drop}
// (src/render/pipeline/pipeline.rs:36-76,134-255,258-277), and the Game state it reads
// (src/game/mod.rs:14-58,103-125).  Everything GPU-side goes through the C ABI in include/rt_abi.h.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/rt_abi.h"
#include "terrain_upload.hpp"

namespace rt::render {

// Positive Y (angle PI/2) is forward, positive X is right, positive Z is up (mod.rs:14-18).
struct Camera {
    float origin[3] = {0.0f, 0.0f, 0.0f};
    float heading = 3.14159265358979323846f * 0.5f;  // Camera::new, mod.rs:27-33
    float pitch = 0.0f;
};

struct TripleEulerVector { float forward[3], up[3], right[3]; };
// src/util.rs:9-22
TripleEulerVector compute_triple_euler_vector(float heading, float pitch);

}  // namespace rt::render

namespace rt::game {

// Game — src/game/mod.rs:14-58.  Interactive controls (control.rs, tick) are out of scope; the world is the
// flattened 256^3 region rather than a ChunkStorage (disk cache is out of scope).
class Game {
 public:
    // Game::new (mod.rs:37-58): six optional positional floats `x y z heading pitch sun_angle`
    // (argv[1..6]); otherwise the default pose (-30, -128, 100), heading PI/2, pitch 0, sun 0.
    Game(int argc, const char* const* argv);
    const render::Camera& borrow_camera() const { return camera; }   // mod.rs:111-113
    float get_sun_angle() const { return sun_angle; }                // mod.rs:123-125
    int generate_world(uint64_t seed, int region = RT_ROOT_BLOCK_SIZE);   // region: 256 = the reference; 512 / 1024 = extension
    int world_region() const { return region_; }
    int set_world(const uint32_t* materials, const uint8_t* minefield, int region = RT_ROOT_BLOCK_SIZE);   // region^3 voxels each
    // The procedural world of generate_world(seed, region) without its host bytes: create_instance generates it on the device
    // (rt_generate_world) in place of rt_upload_world.  generate_world / set_world replace it with host bytes again.
    int use_device_world(uint64_t seed, int region = RT_ROOT_BLOCK_SIZE);
    bool device_world() const { return device_world_; }
    uint64_t device_world_seed() const { return device_seed_; }
    bool has_world() const { return device_world_ || !materials_.empty(); }
    const uint32_t* world_materials() const { return materials_.data(); }
    const uint8_t* world_minefield() const { return minefield_.data(); }

    render::Camera camera;
    float sun_angle = 0.0f;

 private:
    std::vector<uint32_t> materials_;
    std::vector<uint8_t> minefield_;
    int region_ = RT_ROOT_BLOCK_SIZE;
    bool device_world_ = false;
    uint64_t device_seed_ = 0;
};

}  // namespace rt::game

namespace rt::render {

class Pipeline {
 public:
    ~Pipeline();                       // impl Drop for Pipeline, pipeline.rs:258-277
    // pipeline.rs:134-255: wait for the previous frame, derive the 192-byte uniform block from the camera,
    // submit the ray-trace dispatch.  Returns an RtStatus instead of panicking.
    int draw_frame(game::Game& game);
    int wait();                        // the fence wait at pipeline.rs:162-172, callable on its own
    RtContext* context() const { return ctx_; }
    const RtUniforms& uniforms() const { return uniforms_; }
    void set_seed(uint32_t seed) { uniforms_.seed = seed; }
    const char* last_error() const;
    // Terrain streaming (pipeline.rs:174-189): when enabled, every draw_frame asks the TerrainUploadManager to move towards
    // the camera and uploads at most one slab; the render offset becomes the uniform block's `lr`.  Off by default
    // (static region).  `storage_dir` empty = no disk cache.
    void enable_terrain_streaming(uint64_t seed, const std::string& storage_dir);
    // on_device: every slab is generated on the device (rt_generate_slice on the request's window) instead of assembled from host
    // chunks and uploaded (rt_slice_staging + rt_upload_slice); no ChunkStorage, no host bytes.  storage_dir is then unused.
    void enable_terrain_streaming(uint64_t seed, const std::string& storage_dir, bool on_device);
    TerrainUploadManager* terrain_upload_manager() { return tum_.get(); }
    // The rest of the reference's per-frame command buffer (pipeline.rs:98-123): after the ray-trace dispatch, the six
    // bilateral_denoise.comp dispatches and finalize.comp, submitted together (:229-235).  When enabled, draw_frame enqueues
    // ray trace -> rt_denoise -> rt_finalize on the context's stream and RT_BUF_FINAL_BGRA8 holds the swapchain image of the
    // frame.  `faithful` = the reference's pong descriptor set with its swapped bindings (descriptor_sets.rs:38-39).
    // Off by default (the G-buffer planes are then the ray-trace dispatch's own output, which the parity tests compare);
    // whole-frame contexts only (RT_ERR_UNIMPLEMENTED on a tile-split one: the passes need a halo, gather first).
    int enable_post_passes(bool faithful);
    // With post passes on a context created with RT_FLAG_REPROJECT: draw_frame calls rt_denoise_history(params) in place of
    // rt_denoise, so that pixels with a long history are not blurred as hard as fresh ones (params.faithful replaces
    // enable_post_passes' flag for the denoise).  RT_ERR_INVALID_ARG on a context that does not reproject or for a block
    // rt_denoise_history would refuse.
    int enable_history_denoise(const RtDenoiseParams& params);
    // A context created with RT_FLAG_FRAMES_IN_FLIGHT_2: draw_frame no longer waits for the previous frame (the library orders a frame
    // after the one that used its slot before), so frame k + 1 is enqueued while frame k runs.  Off by default (the reference's fence).
    void set_frames_in_flight(int n) { no_fence_ = n == 2; }
    // The block under a pixel of the frame drawn last (its uniforms, the `lr` terrain streaming moved included): rt_pick_pixels on
    // pixel (x, height - 1 - y_from_top), the texel in front of the face it crossed (where a placed block goes) and the hit texel's
    // world coordinate in the lr window.  A game breaks the block with rt_edit_voxels on `hit.texel`, places one on `adjacent`.
    struct PickResult {
        RtRayHit hit;
        int32_t adjacent[3];   // meaningful for kind == RT_HIT_SOLID with texel >= 0
        int32_t world[3];
    };
    int pick(int x, int y_from_top, PickResult* out);
    // The entity under that pixel, if one is drawn there: rt_pick_entities with the pipeline's uniforms and the boxes and models of
    // set_boxes / set_models — the depth test against the world included, so entity.kind != RT_ENTITY_NONE means the cursor is on an
    // entity (entity.index counts within its kind's set) and not on the block behind it, which `world` describes as pick does.
    struct EntityPick {
        RtEntityHit entity;
        PickResult world;
    };
    int pick_entity(int x, int y_from_top, EntityPick* out);
    // Path-traced light at `count` points under the sun, seed and lr of the frame drawn last: rt_probe_light with the pipeline's
    // uniforms (a host that accumulates over calls advances the seed by `samples` between them: set_seed).
    int probe_light(const RtLightProbe* probes, uint32_t count, uint32_t samples, int32_t depth, RtProbeLight* out);
    // Boxes and spheres filled, painted or carved in the resident region, in order (an explosion, a brush): rt_edit_shapes.  The
    // texels are the region's, as PickResult::hit.texel; a shape that crosses the window's seam is issued again shifted by the
    // region's edge (INTEGRATION.md "Explosions and brushes").
    int edit_shapes(const RtShapeEdit* shapes, uint32_t count);
    // Voxel stamps: dense boxes of voxels kept on the device (a tree, a house, a saved box for undo), made from host arrays or
    // captured from the resident region, and pasted turned or mirrored from 32 bytes per placement: rt_stamp_*, rt_edit_stamps.
    // Ids belong to this pipeline's context (INTEGRATION.md "Prefabs and undo").
    int stamp_create(const int32_t extent[3], const uint32_t* materials, const uint8_t* state, uint32_t* id_out);
    int stamp_capture(const int32_t lo[3], const int32_t extent[3], uint32_t flags, uint32_t* id_out);
    int stamp_info(uint32_t id, int32_t extent_out[3]);
    int stamp_read(uint32_t id, uint32_t* materials, uint8_t* state);
    int stamp_destroy(uint32_t id);
    int edit_stamps(const RtStampPlace* places, uint32_t count);
    // Entity boxes: every draw_frame from now on enqueues rt_draw_boxes(boxes, face_lights, count) between the ray trace and the
    // denoise (both arrays are copied; face_lights holds 6 * count records, e.g. probe_light's for the boxes' face probes).
    // count == 0 draws none.  RT_ERR_INVALID_ARG for more than 4096 boxes or a NULL array with count > 0.
    int set_boxes(const RtDrawBox* boxes, const RtProbeLight* face_lights, uint32_t count);
    // Voxel-model entities: every draw_frame from now on enqueues rt_draw_stamps(models, face_lights, count) between the ray trace and
    // the denoise, after the boxes (both arrays are copied; the stamps are this pipeline's and must be live at every draw).
    // count == 0 draws none.  RT_ERR_INVALID_ARG for more than 4096 models or a NULL array with count > 0; an invalid record fails
    // the draw_frame that draws it.
    int set_models(const RtDrawStamp* models, const RtProbeLight* face_lights, uint32_t count);
    // Point lights: every draw_frame from now on enqueues rt_add_lights(lights, count) behind the ray trace and the entity boxes and
    // in front of the denoise (the array is copied).  count == 0 adds none.  RT_ERR_INVALID_ARG for more than 1024 lights or a NULL
    // array with count > 0.
    int set_lights(const RtPointLight* lights, uint32_t count);
    // Entity shadows: every draw_frame from now on enqueues rt_shadow_entities(boxes, models, strength) for the boxes and models set
    // above, behind their draws and in front of the point lights — the intended order: boxes, models, shadows, lights, denoise.
    // strength in (0, 1]; 0 switches it off again.  RT_ERR_INVALID_ARG for anything else.
    int enable_entity_shadows(float strength);
    // Point-light shadows of entities: every draw_frame from now on hands the boxes and models set above to the lights step, which
    // then runs rt_add_lights_occluded in rt_add_lights' place; the order stays boxes, models, sun shadows, lights, denoise.
    void enable_light_shadows(bool on) { light_shadows_ = on; }
    bool post_passes() const { return post_; }

 private:
    friend Pipeline* create_instance(const RtConfig&, const uint8_t*, game::Game&, std::string*);
    Pipeline() = default;
    void finish_pick(PickResult* out) const;   // adjacent and world of a pick whose `hit` is filled
    RtContext* ctx_ = nullptr;
    RtUniforms uniforms_{};            // RenderData::raytrace_uniform_data, render_data.rs:134-162
    int spp_ = 1;
    int region_ = RT_ROOT_BLOCK_SIZE;
    int render_offset_[3] = {0, 0, 0}; // TerrainUploadManager::get_render_offset (terrain_upload.rs:30-47)
    int tile_world_ = 1;
    int height_ = 0;                   // frame height (Pipeline::pick counts rows from the top)
    bool post_ = false, post_faithful_ = true;
    bool reproject_ = false;           // the context was created with RT_FLAG_REPROJECT
    bool history_denoise_ = false;     // enable_history_denoise
    RtDenoiseParams denoise_params_{};
    bool no_fence_ = false;            // set_frames_in_flight(2)
    std::vector<RtDrawBox> boxes_;     // set_boxes
    std::vector<RtProbeLight> box_lights_;
    std::vector<RtDrawStamp> models_;  // set_models
    std::vector<RtProbeLight> model_lights_;
    std::vector<RtPointLight> lights_; // set_lights
    float shadow_strength_ = 0.0f;     // enable_entity_shadows; 0 = off
    bool light_shadows_ = false;       // enable_light_shadows
    std::unique_ptr<TerrainUploadManager> tum_;
    std::unique_ptr<world::ChunkStorage> chunks_;
    bool stream_on_device_ = false;
    uint64_t stream_seed_ = 0;
};

// render::create_instance (mod.rs:36-43) -> Pipeline::new (pipeline.rs:36-76): creates the device context, uploads
// the game's world (RenderData::initialize, render_data.rs:269-301) and the blue-noise table
// (render_data.rs:110-133).  Returns nullptr and fills *error on failure.  `cfg` goes to rt_create as it is: history_cap and
// edit_radius (RT_FLAG_REPROJECT) included.
Pipeline* create_instance(const RtConfig& cfg, const uint8_t* blue_noise_rgba8, game::Game& game, std::string* error);

}  // namespace rt::render
