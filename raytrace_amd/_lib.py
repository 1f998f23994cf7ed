"""Loads the in-tree native libraries.  There is no Python or CPU fallback: if librt_amd.so is missing the
import fails loudly (build it with `python -m raytrace_amd.build`).

Each library's signatures are one table, name -> (restype, argtypes), applied when it is loaded; restype None is `void`.
tests/test_lib_signatures.py holds AMD_FUNCTIONS against include/rt_abi.h: the same functions, the same parameter counts."""
import ctypes as C
import os

from .abi import RtConfig, RtCounters, RtDenoiseParams, RtInfo, RtShapeEdit, RtStampPlace, RtTiming, RtUniforms, RtVoxelEdit

HERE = os.path.dirname(os.path.abspath(__file__))
# RT_AMD_LIB: load another build of the same library (same-box A/B timing of two kernel variants, tools/ab.sh)
LIB_AMD_PATH = os.environ.get("RT_AMD_LIB") or os.path.join(HERE, "librt_amd.so")
LIB_HOST_PATH = os.path.join(HERE, "librt_host.so")

P, PP, STR = C.c_void_p, C.POINTER(C.c_void_p), C.c_char_p
INT, LONG, SIZE, FLOAT, U8, U32, U64 = C.c_int, C.c_long, C.c_size_t, C.c_float, C.c_uint8, C.c_uint32, C.c_uint64
I32P, U32P, I64P = C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_int64)
UNI, DENOISE = C.POINTER(RtUniforms), C.POINTER(RtDenoiseParams)

# Every function include/rt_abi.h declares; P first is the RtContext*.
AMD_FUNCTIONS = {
    "rt_abi_version": (U32, []),
    "rt_create": (INT, [C.POINTER(RtConfig), PP]),
    "rt_destroy": (None, [P]),
    "rt_last_error": (STR, [P]),
    "rt_get_info": (INT, [P, C.POINTER(RtInfo)]),
    "rt_samples_per_launch": (U64, [U64, U64, U64, STR]),
    # the world: uploads, edits, stamps, generated terrain
    "rt_upload_world": (INT, [P, P, P]),
    "rt_upload_slice": (INT, [P, INT, INT, P, P]),
    "rt_slice_staging": (INT, [P, PP, PP]),
    "rt_upload_noise": (INT, [P, P]),
    "rt_edit_voxels": (INT, [P, C.POINTER(RtVoxelEdit), U32]),
    "rt_edit_shapes": (INT, [P, C.POINTER(RtShapeEdit), U32]),
    "rt_stamp_create": (INT, [P, I32P, P, P, U32P]),
    "rt_stamp_capture": (INT, [P, I32P, I32P, U32, U32P]),
    "rt_stamp_info": (INT, [P, U32, I32P]),
    "rt_stamp_read": (INT, [P, U32, P, P]),
    "rt_stamp_destroy": (INT, [P, U32]),
    "rt_edit_stamps": (INT, [P, C.POINTER(RtStampPlace), U32]),
    "rt_read_box": (INT, [P, INT, INT, INT, INT, INT, INT, P, P]),
    "rt_generate_world": (INT, [P, U64, I64P]),
    "rt_generate_slice": (INT, [P, U64, INT, I64P]),
    # queries
    "rt_trace_rays": (INT, [P, P, U32, I32P, P]),
    "rt_trace_rays_async": (INT, [P, P, U32, I32P, P]),
    "rt_pick_pixels": (INT, [P, UNI, P, U32, P]),
    "rt_probe_light": (INT, [P, UNI, P, U32, U32, C.c_int32, P]),
    "rt_probe_light_async": (INT, [P, UNI, P, U32, U32, C.c_int32, P]),
    "rt_sweep_boxes": (INT, [P, P, U32, I32P, P]),
    "rt_sweep_boxes_async": (INT, [P, P, U32, I32P, P]),
    "rt_step_particles": (INT, [P, P, P, P, P, U32]),
    "rt_step_particles_async": (INT, [P, P, P, P, P, U32]),
    "rt_emit_particles": (INT, [P, P, U32, I32P, P, U32, U32, P]),
    "rt_emit_particles_async": (INT, [P, P, U32, I32P, P, U32, U32, P]),
    "rt_deposit_particles": (INT, [P, P, P, P, U32, P]),
    "rt_deposit_particles_async": (INT, [P, P, P, P, U32, P]),
    "rt_settle_voxels": (INT, [P, P, P]),
    "rt_settle_voxels_async": (INT, [P, P, P]),
    "rt_detach_voxels": (INT, [P, P, P, P]),
    "rt_detach_voxels_async": (INT, [P, P, P, P]),
    "rt_flow_voxels": (INT, [P, P, P]),
    "rt_flow_voxels_async": (INT, [P, P, P]),
    "rt_nav_create": (INT, [P, I32P, U32P]),
    "rt_nav_info": (INT, [P, U32, I32P, I32P, U32P]),
    "rt_nav_read": (INT, [P, U32, P, P]),
    "rt_nav_destroy": (INT, [P, U32]),
    "rt_nav_build": (INT, [P, U32, P, P, U32, P]),
    "rt_nav_build_async": (INT, [P, U32, P, P, U32, P]),
    "rt_nav_sample": (INT, [P, U32, P, U32, P]),
    "rt_nav_sample_async": (INT, [P, U32, P, U32, P]),
    "rt_trace_entities": (INT, [P, P, U32, I32P, P, U32, P, U32, P, P]),
    "rt_trace_entities_async": (INT, [P, P, U32, I32P, P, U32, P, U32, P, P]),
    "rt_pick_entities": (INT, [P, UNI, P, U32, P, U32, P, U32, P, P]),
    "rt_sweep_entities": (INT, [P, P, U32, I32P, P, U32, P, U32, P, P]),
    "rt_sweep_entities_async": (INT, [P, P, U32, I32P, P, U32, P, U32, P, P]),
    # the frame and the passes over it
    "rt_draw_frame": (INT, [P, UNI]),
    "rt_draw_boxes": (INT, [P, UNI, P, P, U32]),
    "rt_draw_boxes_async": (INT, [P, UNI, P, P, U32]),
    "rt_draw_stamps": (INT, [P, UNI, P, P, U32]),
    "rt_draw_stamps_async": (INT, [P, UNI, P, P, U32]),
    "rt_draw_particles": (INT, [P, UNI, P, U32, P, U32]),
    "rt_draw_particles_async": (INT, [P, UNI, P, U32, P, U32]),
    "rt_shadow_entities": (INT, [P, UNI, P, U32, P, U32, FLOAT]),
    "rt_shadow_entities_async": (INT, [P, UNI, P, U32, P, U32, FLOAT]),
    "rt_add_lights": (INT, [P, UNI, P, U32]),
    "rt_add_lights_async": (INT, [P, UNI, P, U32]),
    "rt_add_lights_occluded": (INT, [P, UNI, P, U32, P, U32, P, U32]),
    "rt_add_lights_occluded_async": (INT, [P, UNI, P, U32, P, U32, P, U32]),
    "rt_denoise": (INT, [P, INT]),
    "rt_finalize": (INT, [P]),
    "rt_denoise_planes": (INT, [P, P, P, P, INT]),
    "rt_finalize_planes": (INT, [P, P, P, P, P, P, P]),
    "rt_denoise_history": (INT, [P, DENOISE]),
    "rt_denoise_planes_counted": (INT, [P, P, P, P, P, DENOISE]),
    # streams, planes, tiles
    "rt_sync": (INT, [P]),
    "rt_set_stream": (INT, [P, P]),
    "rt_readback": (INT, [P, INT, P, SIZE]),
    "rt_buffer_bytes": (SIZE, [P, INT]),
    "rt_device_ptr": (P, [P, INT]),
    "rt_tile_count": (INT, [P]),
    "rt_tile_capacity": (INT, [P]),
    "rt_untile": (INT, [P, INT, P, INT, P]),
    "rt_gbuffer_ptr": (P, [P]),
    "rt_gbuffer_bytes": (SIZE, [P]),
    "rt_gbuffer_offset": (SIZE, [P, INT]),
    "rt_untile_gbuffer": (INT, [P, P, INT, P]),
    # multi-GPU frame assembly
    "rt_comm_unique_id": (INT, [P, SIZE]),
    "rt_comm_init_rank": (INT, [P, P, SIZE, PP]),
    "rt_comm_init_all": (INT, [INT, C.POINTER(INT), PP]),
    "rt_comm_destroy": (INT, [P]),
    "rt_gather_gbuffer": (INT, [P, P, INT, P, INT]),
    "rt_frame_ptr": (P, [P, INT]),
    "rt_frame_readback": (INT, [P, INT, P, SIZE]),
    # instrumentation and host-side state
    "rt_kernel_in_use": (INT, [P]),
    "rt_selftest": (INT, [P, INT, C.POINTER(U64)]),
    "rt_get_counters": (INT, [P, C.POINTER(RtCounters)]),
    "rt_reset_counters": (INT, [P]),
    "rt_get_timing": (INT, [P, C.POINTER(RtTiming)]),
    "rt_get_gather_timing": (INT, [P, C.POINTER(FLOAT), U32P]),
    "rt_reset_accumulation": (INT, [P]),
    "rt_get_accumulation": (INT, [P, U32P, U32P]),
    "rt_read_history": (INT, [P, P, SIZE]),
    "rt_edit_boxes_pending": (INT, [P, U32P, U32P]),
    "rt_slabs_pending": (INT, [P, U32P, U32P]),
    "rt_read_slab_boxes": (INT, [P, P, U32P]),
}
ABI_SYMBOLS = tuple(AMD_FUNCTIONS)

# The C surface of the host mirror (host/host_capi.cpp) that the package calls.
HOST_FUNCTIONS = {
    "rth_material_pack": (U32, [INT]),
    "rth_material_unpack": (None, [U32, P, P]),
    "rth_material_get": (INT, [INT, P, P, P]),
    "rth_pack_chunk": (INT, [P, P, P]),
    "rth_generate_region": (INT, [U64, P, P]),
    "rth_generate_region_r": (INT, [U64, INT, P, P]),
    "rth_region_from_ids": (INT, [P, P, P]),
    "rth_heightmap": (INT, [LONG, LONG, U64, P]),
    "rth_copy_3d_u32": (INT, [P] * 7),
    "rth_copy_3d_auto_clip_u32": (None, [P, INT, P, P, INT]),
    "rth_copy_3d_bounded_auto_clip_u32": (None, [P] * 7),
    "rth_fill_slice_3d_auto_clip_u8": (None, [U8, P, INT, P, P]),
    "rth_chunk_codec_available": (INT, []),
    "rth_chunk_file_name": (None, [LONG, LONG, LONG, P]),
    "rth_chunk_write": (INT, [STR, P, P]),
    "rth_chunk_read": (INT, [STR, P, P]),
    "rth_chunk_storage_new": (P, [STR, U64]),
    "rth_chunk_storage_free": (None, [P]),
    "rth_chunk_storage_borrow": (INT, [P, LONG, LONG, LONG, P, P]),
    "rth_chunk_storage_stats": (None, [P, P, P]),
    "rth_tum_new": (P, [U64]),
    "rth_tum_new_r": (P, [U64, INT]),
    "rth_tum_free": (None, [P]),
    "rth_tum_request": (None, [P, INT, INT]),
    "rth_tum_move_towards": (None, [P, P]),
    "rth_tum_pending": (INT, [P]),
    "rth_tum_step": (INT, [P]),
    "rth_tum_render_offset": (None, [P, P]),
    "rth_tum_next_window": (INT, [P, P, P]),
    "rth_tum_region": (None, [P, P, P]),
    "rth_compute_triple_euler_vector": (None, [FLOAT, FLOAT, P, P, P]),
    "rth_game_new": (P, [INT, P]),
    "rth_game_free": (None, [P]),
    "rth_game_set_camera": (None, [P, P, FLOAT, FLOAT]),
    "rth_game_get_camera": (None, [P, P, P, P]),
    "rth_game_set_sun_angle": (None, [P, FLOAT]),
    "rth_game_get_sun_angle": (FLOAT, [P]),
    "rth_game_set_world": (INT, [P, P, P]),
    "rth_game_set_world_r": (INT, [P, P, P, INT]),
    "rth_game_generate_world": (INT, [P, U64]),
    "rth_game_generate_world_r": (INT, [P, U64, INT]),
    "rth_game_use_device_world": (INT, [P, U64, INT]),
    "rth_create_instance": (P, [C.POINTER(RtConfig), P, P, P, SIZE]),
    "rth_pipeline_free": (None, [P]),
    "rth_pipeline_draw_frame": (INT, [P, P]),
    "rth_pipeline_wait": (INT, [P]),
    "rth_pipeline_context": (P, [P]),
    "rth_pipeline_uniforms": (None, [P, UNI]),
    "rth_pipeline_set_seed": (None, [P, U32]),
    "rth_pipeline_enable_streaming": (None, [P, U64, STR]),
    "rth_pipeline_enable_streaming_on_device": (None, [P, U64]),
    "rth_pipeline_enable_post_passes": (INT, [P, INT]),
    "rth_pipeline_enable_history_denoise": (INT, [P, DENOISE]),
    "rth_pipeline_last_error": (STR, [P]),
    "rth_pipeline_pick": (INT, [P, INT, INT, P, I32P, I32P]),
    "rth_pipeline_pick_entity": (INT, [P, INT, INT, P, P, I32P, I32P]),
    "rth_pipeline_set_boxes": (INT, [P, P, P, U32]),
    "rth_pipeline_set_models": (INT, [P, P, P, U32]),
    "rth_pipeline_set_lights": (INT, [P, P, U32]),
    "rth_pipeline_enable_entity_shadows": (INT, [P, FLOAT]),
    "rth_pipeline_enable_light_shadows": (INT, [P, INT]),
}

_amd = None
_host = None


class NativeLibraryMissing(ImportError):
    pass


def _declare(lib, functions):
    for name, (restype, argtypes) in functions.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = restype, argtypes
    return lib


def amd():
    """librt_amd.so: the HIP kernels behind the C ABI."""
    global _amd
    if _amd is None:
        if not os.path.exists(LIB_AMD_PATH):
            raise NativeLibraryMissing(
                "%s not found: the HIP extension is required (run `python -m raytrace_amd.build`); "
                "there is no CPU fallback" % LIB_AMD_PATH)
        _amd = _declare(C.CDLL(LIB_AMD_PATH, mode=C.RTLD_GLOBAL), AMD_FUNCTIONS)
    return _amd


def host():
    """librt_host.so: C++ host mirror (world flattening, camera, Game, Pipeline)."""
    global _host
    if _host is None:
        amd()  # dependency; also enforces the loud failure
        if not os.path.exists(LIB_HOST_PATH):
            raise NativeLibraryMissing("%s not found (run `python -m raytrace_amd.build`)" % LIB_HOST_PATH)
        # RT_HOST_LIB: another build of the same sources (the CPU sanitizer build, `make -C oracle asan`)
        _host = _declare(C.CDLL(os.environ.get("RT_HOST_LIB") or LIB_HOST_PATH), HOST_FUNCTIONS)
    return _host
