"""ctypes mirror of include/rt_abi.h (structs, enums, constants).

`RtUniforms` is byte-identical to the reference's `RaytraceUniformData`
(src/render/pipeline/structs.rs:3-31) and the GLSL block at shaders/glsl/raytrace.comp:25-35.
"""
import ctypes as C

import numpy as np

ROOT_BLOCK_SIZE = 256      # src/render/constants.rs:27
CHUNK_SIZE = 64            # constants.rs:23
NOISE_SIZE = 512           # constants.rs:16-17
NOISE_BYTES = 512 * 512 * 4  # constants.rs:19 BLUE_NOISE_SIZE
MAX_DEPTH = 16

RT_OK = 0
RT_ERR_INVALID_ARG = -1
RT_ERR_NO_DEVICE = -2
RT_ERR_HIP = -3
RT_ERR_NOT_READY = -4
RT_ERR_UNIMPLEMENTED = -5
RT_ERR_OOM = -6

RT_FLAG_TRUSTED_WORLD = 0x10
RT_KERNEL_DEFAULT, RT_KERNEL_MEGA, RT_KERNEL_WAVEFRONT, RT_KERNEL_PERSISTENT, RT_KERNEL_PATHS, RT_KERNEL_FRAME = 0, 1, 2, 3, 5, 7   # 4 (PERSISTENT2) and 6 (SEQ): retired
RT_FLAG_FRAMES_IN_FLIGHT_2 = 0x20
RT_FLAG_ACCUMULATE = 0x40     # ABI 1.3, additive: progressive accumulation while the camera holds still
RT_FLAG_REPROJECT = 0x80      # ABI 1.3, additive: the accumulated lighting is reprojected when the camera moves (1-spp whole frames)
RT_FLAG_COUNTERS = 0x1
RT_SELFTEST_DENOISE_DIVISION = 1
RT_SELFTEST_SCENE_MAPS = 2    # ABI 1.3, additive: rebuild the nibble maps from the resident minefield, count differing words
RT_FLAG_CACHE_PRIMARY = 0x2
RT_FLAG_TIMING = 0x4
RT_FLAG_TIMING_ALL = 0xC

(RT_BUF_LIGHTING_RGBA16, RT_BUF_DEPTH_R16UI, RT_BUF_NORMAL_R8UI, RT_BUF_ALBEDO_RGBA8,
 RT_BUF_EMISSION_RGBA8, RT_BUF_FOG_RGBA8, RT_BUF_LIGHTING_F32, RT_BUF_FOG_F32,
 RT_BUF_DEPTH_F32, RT_BUF_FINAL_BGRA8, RT_BUF_COUNT) = range(11)

# (numpy dtype, channels) per output plane
BUFFER_FORMATS = {
    RT_BUF_LIGHTING_RGBA16: ("uint16", 4),
    RT_BUF_DEPTH_R16UI: ("uint16", 1),
    RT_BUF_NORMAL_R8UI: ("uint8", 1),
    RT_BUF_ALBEDO_RGBA8: ("uint8", 4),
    RT_BUF_EMISSION_RGBA8: ("uint8", 4),
    RT_BUF_FOG_RGBA8: ("uint8", 4),
    RT_BUF_LIGHTING_F32: ("float32", 4),
    RT_BUF_FOG_F32: ("float32", 4),
    RT_BUF_DEPTH_F32: ("float32", 1),
    RT_BUF_FINAL_BGRA8: ("uint8", 4),
}
BUFFER_NAMES = {
    RT_BUF_LIGHTING_RGBA16: "lighting_rgba16", RT_BUF_DEPTH_R16UI: "depth_r16", RT_BUF_NORMAL_R8UI: "normal_r8",
    RT_BUF_ALBEDO_RGBA8: "albedo_rgba8", RT_BUF_EMISSION_RGBA8: "emission_rgba8", RT_BUF_FOG_RGBA8: "fog_rgba8",
    RT_BUF_LIGHTING_F32: "lighting_f32", RT_BUF_FOG_F32: "fog_f32", RT_BUF_DEPTH_F32: "depth_f32",
    RT_BUF_FINAL_BGRA8: "final_bgra8",
}


class RtUniforms(C.Structure):
    _fields_ = [
        ("sun_angle", C.c_float), ("seed", C.c_uint32), ("_padding0", C.c_uint32 * 2),
        ("origin", C.c_float * 3), ("_padding1", C.c_uint32),
        ("forward", C.c_float * 3), ("_padding2", C.c_uint32),
        ("up", C.c_float * 3), ("_padding3", C.c_uint32),
        ("right", C.c_float * 3), ("_padding4", C.c_uint32),
        ("old_origin", C.c_float * 3), ("_padding5", C.c_uint32),
        ("old_transform_c0", C.c_float * 3), ("_padding6", C.c_uint32),
        ("old_transform_c1", C.c_float * 3), ("_padding7", C.c_uint32),
        ("old_transform_c2", C.c_float * 3), ("_padding8", C.c_uint32),
        ("region_offset", C.c_int32 * 3), ("_padding9", C.c_uint32),
        ("lr", C.c_int32 * 3), ("_padding10", C.c_uint32),
        ("lso", C.c_int32 * 3), ("_padding11", C.c_uint32),
    ]


assert C.sizeof(RtUniforms) == 192


class _RtConfigTailFields(C.Structure):
    _fields_ = [("edit_radius", C.c_int32), ("stream_history", C.c_int32), ("reserved2", C.c_int32 * 2)]


class _RtConfigTail(C.Union):
    """The last 16 bytes of RtConfig: the header's `edit_radius; stream_history; reserved[2]` (ABI 1.3, additive: each took the first
    reserved word of its time), and `reserved`, the four words seen whole as callers written before that knew them (reserved[0] IS
    edit_radius, reserved[1] IS stream_history)."""
    _anonymous_ = ("named",)
    _fields_ = [("named", _RtConfigTailFields), ("reserved", C.c_int32 * 4)]


class RtConfig(C.Structure):
    _anonymous_ = ("tail",)
    _fields_ = [
        ("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("region", C.c_int32),
        ("spp", C.c_int32), ("depth", C.c_int32), ("device", C.c_int32), ("tile_rank", C.c_int32),
        ("tile_world", C.c_int32), ("kernel", C.c_int32), ("flags", C.c_uint32),
        ("history_cap", C.c_int32), ("tail", _RtConfigTail),
    ]


class RtCounters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "rays", "rays_primary", "rays_shadow", "rays_diffuse", "iterations", "minefield_fetches",
        "material_fetches", "noise_fetches", "hits", "sky_exits", "limit_exits", "border_fetches",
        "pixels", "frames")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}

    def algorithmic_bytes(self):
        """B_alg of SURVEY.md 8(d) / BASELINE.md 5."""
        return self.minefield_fetches + 4 * self.material_fetches + 4 * self.noise_fetches + 23 * self.pixels


class RtInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("num_cus", C.c_int32), ("samples_per_launch", C.c_uint32), ("launches_in_flight", C.c_uint16), ("frames_in_flight", C.c_uint16),
                ("light_record_budget_bytes", C.c_uint64), ("light_record_bytes", C.c_uint64), ("device_bytes", C.c_uint64)]


class RtTiming(C.Structure):
    _fields_ = [("frame_ms", C.c_float), ("trace_ms", C.c_float), ("shade_ms", C.c_float),
                ("trace_launches", C.c_uint32), ("other_launches", C.c_uint32), ("rays_traced", C.c_uint64)]


class RtVoxelEdit(C.Structure):
    """rt_edit_voxels record (ABI 1.3, additive): one edited voxel, 16 bytes."""
    _fields_ = [("x", C.c_uint16), ("y", C.c_uint16), ("z", C.c_uint16), ("solid", C.c_uint16), ("material", C.c_uint32),
                ("reserved", C.c_uint32)]


assert C.sizeof(RtVoxelEdit) == 16


RT_SHAPE_BOX, RT_SHAPE_SPHERE = 0, 1                # RtShapeEdit.kind (ABI 1.3, additive: shape edits)
RT_WHERE_ALL, RT_WHERE_SOLID, RT_WHERE_AIR = 0, 1, 2   # RtShapeEdit.where


class RtShapeEdit(C.Structure):
    """rt_edit_shapes record (ABI 1.3, additive): one box or sphere, 32 bytes; `reserved` must be 0."""
    _fields_ = [("a", C.c_int32 * 3), ("material", C.c_uint32), ("b", C.c_int32 * 3), ("kind", C.c_uint8), ("where", C.c_uint8),
                ("solid", C.c_uint8), ("reserved", C.c_uint8)]


assert C.sizeof(RtShapeEdit) == 32


RT_STAMP_ABSENT, RT_STAMP_AIR, RT_STAMP_SOLID = 0, 1, 2   # a stamp voxel's state (ABI 1.3, additive: voxel stamps)
RT_STAMP_SKIP_AIR = 0x1                                    # rt_stamp_capture flag: unoccupied voxels become ABSENT, not AIR


class RtStampPlace(C.Structure):
    """rt_edit_stamps record (ABI 1.3, additive): one placement of a stamp, 32 bytes; the reserved fields must be 0."""
    _fields_ = [("at", C.c_int32 * 3), ("stamp", C.c_uint32), ("orient", C.c_uint8), ("where", C.c_uint8), ("reserved0", C.c_uint8 * 2),
                ("reserved", C.c_uint32 * 3)]


assert C.sizeof(RtStampPlace) == 32


RT_HIT_AIR, RT_HIT_SOLID, RT_HIT_LIMIT = 0, 1, 2   # RtRayHit.kind (ABI 1.3, additive: ray queries)


class RtRay(C.Structure):
    """rt_trace_rays input (ABI 1.3, additive): 32 bytes; the reserved words are ignored."""
    _fields_ = [("origin", C.c_float * 3), ("reserved0", C.c_uint32), ("direction", C.c_float * 3), ("reserved1", C.c_uint32)]


class RtRayHit(C.Structure):
    """rt_trace_rays / rt_pick_pixels result (ABI 1.3, additive): 48 bytes."""
    _fields_ = [("position", C.c_float * 3), ("distance", C.c_float), ("texel", C.c_int32 * 3), ("material", C.c_uint32),
                ("normal", C.c_uint32), ("kind", C.c_uint32), ("iterations", C.c_uint32), ("border_fetches", C.c_uint32)]


assert C.sizeof(RtRay) == 32 and C.sizeof(RtRayHit) == 48


RT_PROBE_SPHERE = 6   # RtLightProbe.normal: no hemisphere offset (ABI 1.3, additive: light probes)


class RtLightProbe(C.Structure):
    """rt_probe_light input (ABI 1.3, additive): 32 bytes; `reserved` must be 0."""
    _fields_ = [("position", C.c_float * 3), ("normal", C.c_uint32), ("cell", C.c_uint16 * 2), ("reserved", C.c_uint32 * 3)]


class RtProbeLight(C.Structure):
    """rt_probe_light result (ABI 1.3, additive): 16 bytes."""
    _fields_ = [("light", C.c_float * 3), ("sun_samples", C.c_uint32)]


assert C.sizeof(RtLightProbe) == 32 and C.sizeof(RtProbeLight) == 16


RT_SWEEP_FREE, RT_SWEEP_BLOCKED, RT_SWEEP_EMBEDDED, RT_SWEEP_INVALID = 0, 1, 2, 3   # RtSweepHit.kind (ABI 1.3, additive: box sweeps)


class RtBoxSweep(C.Structure):
    """rt_sweep_boxes input (ABI 1.3, additive): 48 bytes; the reserved words are ignored."""
    _fields_ = [("lo", C.c_float * 3), ("reserved0", C.c_uint32), ("hi", C.c_float * 3), ("reserved1", C.c_uint32),
                ("motion", C.c_float * 3), ("reserved2", C.c_uint32)]


class RtSweepHit(C.Structure):
    """rt_sweep_boxes result (ABI 1.3, additive): 64 bytes."""
    _fields_ = [("t", C.c_float), ("kind", C.c_uint32), ("normal", C.c_uint32), ("material", C.c_uint32),
                ("texel", C.c_int32 * 3), ("axis", C.c_uint32), ("lo", C.c_float * 3), ("reserved0", C.c_uint32),
                ("hi", C.c_float * 3), ("reserved1", C.c_uint32)]


assert C.sizeof(RtBoxSweep) == 48 and C.sizeof(RtSweepHit) == 64


class RtDrawBox(C.Structure):
    """rt_draw_boxes input (ABI 1.3, additive: entity boxes): 32 bytes."""
    _fields_ = [("lo", C.c_float * 3), ("material", C.c_uint32), ("hi", C.c_float * 3), ("emission", C.c_uint32)]


assert C.sizeof(RtDrawBox) == 32
assert (RtDrawBox.lo.offset, RtDrawBox.material.offset, RtDrawBox.hi.offset, RtDrawBox.emission.offset) == (0, 12, 16, 28)
MAX_DRAW_BOXES = 4096   # rt_draw_boxes: boxes per call


class RtParticle(C.Structure):
    """rt_draw_particles input (ABI 1.3, additive: particles): 32 bytes; `reserved` must be 0."""
    _fields_ = [("center", C.c_float * 3), ("half", C.c_float), ("material", C.c_uint32), ("emission", C.c_uint32), ("light", C.c_uint32),
                ("reserved", C.c_uint32)]


assert C.sizeof(RtParticle) == 32
assert (RtParticle.center.offset, RtParticle.half.offset, RtParticle.material.offset, RtParticle.emission.offset, RtParticle.light.offset,
        RtParticle.reserved.offset) == (0, 12, 16, 20, 24, 28)
MAX_PARTICLES = 1 << 20         # rt_draw_particles: particles per call
MAX_PARTICLE_LIGHTS = 1 << 20   # ... and light records per call
PARTICLE_DTYPE = np.dtype(RtParticle)   # the numpy view of the record (render.make_particles builds arrays of it)

# rt_step_particles (ABI 1.3, additive: particle simulation): RtParticleState.flags
RT_PARTICLE_DIE, RT_PARTICLE_STICK, RT_PARTICLE_SLIDE, RT_PARTICLE_BOUNCE = 0, 1, 2, 3   # the response to contact, flags & RT_PSTATE_RESPONSE
RT_PSTATE_RESPONSE = 0x3
RT_PSTATE_DEAD = 0x100        # inactive: copied through, not drawn
RT_PSTATE_INVALID = 0x200     # set by the device on a record outside the domain; inactive
RT_PSTATE_CONTACT = 0x70000   # output: bit 16 + a set iff axis a blocked a sub-sweep this tick


class RtParticleState(C.Structure):
    """rt_step_particles' state of one particle: 64 bytes; `reserved` must be 0."""
    _fields_ = [("lo", C.c_float * 3), ("life", C.c_float), ("hi", C.c_float * 3), ("flags", C.c_uint32), ("velocity", C.c_float * 3),
                ("light", C.c_uint32), ("material", C.c_uint32), ("emission", C.c_uint32), ("half", C.c_float), ("reserved", C.c_uint32)]


class RtParticleStep(C.Structure):
    """rt_step_particles' parameters of one call: 48 bytes."""
    _fields_ = [("dt", C.c_float), ("accel", C.c_float * 3), ("damping", C.c_float), ("restitution", C.c_float), ("friction", C.c_float),
                ("rest_speed", C.c_float), ("lr", C.c_int32 * 3), ("sweeps", C.c_uint32)]


assert C.sizeof(RtParticleState) == 64 and C.sizeof(RtParticleStep) == 48
PARTICLE_STATE_DTYPE = np.dtype(RtParticleState)   # the numpy view of the state (render.make_particle_states builds arrays of it)


class RtParticleEmit(C.Structure):
    """rt_emit_particles' emitter (ABI 1.3, additive: particle emitters): 96 bytes; the reserved bytes and words must be 0."""
    _fields_ = [("a", C.c_int32 * 3), ("seed", C.c_uint32), ("b", C.c_int32 * 3), ("kind", C.c_uint8), ("response", C.c_uint8),
                ("reserved0", C.c_uint8 * 2), ("origin", C.c_float * 3), ("speed", C.c_float), ("drift", C.c_float * 3), ("spread", C.c_float),
                ("half", C.c_float), ("life_min", C.c_float), ("life_span", C.c_float), ("density", C.c_uint32), ("light", C.c_uint32),
                ("emission", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class RtEmitCursor(C.Structure):
    """rt_emit_particles' ring cursor: 16 bytes; `reserved` is left as it is."""
    _fields_ = [("next", C.c_uint32), ("emitted", C.c_uint32), ("dropped", C.c_uint32), ("reserved", C.c_uint32)]


assert C.sizeof(RtParticleEmit) == 96 and C.sizeof(RtEmitCursor) == 16
assert (RtParticleEmit.seed.offset, RtParticleEmit.b.offset, RtParticleEmit.kind.offset, RtParticleEmit.response.offset, RtParticleEmit.origin.offset,
        RtParticleEmit.drift.offset, RtParticleEmit.half.offset, RtParticleEmit.density.offset, RtParticleEmit.light.offset,
        RtParticleEmit.reserved.offset) == (12, 16, 28, 29, 32, 48, 64, 76, 80, 88)
EMIT_DTYPE = np.dtype(RtParticleEmit)          # the numpy view of an emitter (render.make_particle_emitters builds arrays of it)
EMIT_CURSOR_DTYPE = np.dtype(RtEmitCursor)     # ... and of the cursor
MAX_EMITTERS = 256                             # rt_emit_particles: emitters per call
MAX_EMIT_CAPACITY = 1 << 20                    # ... and slots of the ring


class RtParticleDeposit(C.Structure):
    """rt_deposit_particles' parameters (ABI 1.3, additive: particle deposits): 48 bytes; the reserved words must be 0."""
    _fields_ = [("lo", C.c_int32 * 3), ("max_speed", C.c_float), ("hi", C.c_int32 * 3), ("reserved0", C.c_uint32), ("lr", C.c_int32 * 3),
                ("reserved1", C.c_uint32)]


class RtDepositCount(C.Structure):
    """rt_deposit_particles' counters: 16 bytes, added to by every call."""
    _fields_ = [("deposited", C.c_uint32), ("voxels", C.c_uint32), ("occupied", C.c_uint32), ("outside", C.c_uint32)]


assert C.sizeof(RtParticleDeposit) == 48 and C.sizeof(RtDepositCount) == 16
assert (RtParticleDeposit.max_speed.offset, RtParticleDeposit.hi.offset, RtParticleDeposit.reserved0.offset, RtParticleDeposit.lr.offset,
        RtParticleDeposit.reserved1.offset) == (12, 16, 28, 32, 44)
DEPOSIT_DTYPE = np.dtype(RtParticleDeposit)        # the numpy view of the parameters
DEPOSIT_COUNT_DTYPE = np.dtype(RtDepositCount)     # ... and of the counters
MAX_DEPOSIT_TEXELS = 1 << 24                       # rt_deposit_particles: texels of the clipped box


def make_particle_deposit(lo, hi, max_speed=0.0, lr=(0, 0, 0)):
    """An RtParticleDeposit: the box `lo`..`hi` of texels (inclusive, as a box shape's a and b), the rest threshold `max_speed` in units
    per second and the window `lr`.  Refuses what the calls refuse without knowing R: a box with lo > hi, a non-finite or negative
    max_speed.  The box's range and the window's bound are judged by the call (they need R)."""
    if len(lo) != 3 or len(hi) != 3 or len(lr) != 3:
        raise ValueError("lo, hi and lr have three components")
    p = RtParticleDeposit()
    for k in range(3):
        p.lo[k], p.hi[k], p.lr[k] = int(lo[k]), int(hi[k]), int(lr[k])
        if p.lo[k] > p.hi[k]:
            raise ValueError("the box needs lo <= hi on every axis")
    p.max_speed = float(max_speed)
    if not (p.max_speed >= 0.0 and p.max_speed != float("inf")):
        raise ValueError("max_speed must be finite and not negative")
    return p


class RtVoxelSettle(C.Structure):
    """rt_settle_voxels' parameters (ABI 1.3, additive: voxel settling): 48 bytes; the reserved bytes and word must be 0."""
    _fields_ = [("lo", C.c_int32 * 3), ("max_fall", C.c_uint32), ("hi", C.c_int32 * 3), ("air_material", C.c_uint32), ("loose_mask", C.c_uint32),
                ("loose_value", C.c_uint32), ("axis", C.c_uint8), ("toward", C.c_uint8), ("reserved0", C.c_uint8 * 2), ("reserved1", C.c_uint32)]


class RtSettleCount(C.Structure):
    """rt_settle_voxels' counters: 16 bytes, added to by every call."""
    _fields_ = [("moved", C.c_uint32), ("falling", C.c_uint32), ("distance", C.c_uint32), ("chunks", C.c_uint32)]


assert C.sizeof(RtVoxelSettle) == 48 and C.sizeof(RtSettleCount) == 16
assert (RtVoxelSettle.max_fall.offset, RtVoxelSettle.hi.offset, RtVoxelSettle.air_material.offset, RtVoxelSettle.loose_mask.offset,
        RtVoxelSettle.loose_value.offset, RtVoxelSettle.axis.offset, RtVoxelSettle.toward.offset, RtVoxelSettle.reserved0.offset,
        RtVoxelSettle.reserved1.offset) == (12, 16, 28, 32, 36, 40, 41, 42, 44)
SETTLE_DTYPE = np.dtype(RtVoxelSettle)             # the numpy view of the parameters
SETTLE_COUNT_DTYPE = np.dtype(RtSettleCount)       # ... and of the counters
SETTLE_UNLIMITED = 0xFFFFFFFF                      # RtVoxelSettle.max_fall: until the voxel rests


def make_voxel_settle(lo, hi, max_fall=SETTLE_UNLIMITED, air_material=0, loose_mask=0, loose_value=0, axis=2, toward=0):
    """An RtVoxelSettle: the box `lo`..`hi` of texels (inclusive, as a box shape's a and b), the cells a voxel may fall in this call,
    the word left in vacated cells, the mask test that makes an occupied voxel loose (0, 0: every one) and the fall direction (the
    terrain's down is axis 2 towards 0).  Refuses what the calls refuse without knowing R: a box with lo > hi, axis > 2, toward > 1,
    max_fall == 0, a loose_value bit outside loose_mask.  The box's range is judged by the call (it needs R)."""
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("lo and hi have three components")
    p = RtVoxelSettle()
    for k in range(3):
        p.lo[k], p.hi[k] = int(lo[k]), int(hi[k])
        if p.lo[k] > p.hi[k]:
            raise ValueError("the box needs lo <= hi on every axis")
    if int(axis) not in (0, 1, 2) or int(toward) not in (0, 1):
        raise ValueError("axis is 0, 1 or 2 and toward 0 or 1")
    if not 1 <= int(max_fall) <= SETTLE_UNLIMITED:
        raise ValueError("max_fall is 1..0xFFFFFFFF")
    if int(loose_value) & ~int(loose_mask):
        raise ValueError("loose_value has a bit outside loose_mask")
    p.max_fall, p.air_material, p.loose_mask, p.loose_value = int(max_fall), int(air_material), int(loose_mask), int(loose_value)
    p.axis, p.toward = int(axis), int(toward)
    return p


RT_DETACH_CARVE, RT_DETACH_CAPTURE, RT_DETACH_ANCHOR_MATERIAL = 0x1, 0x2, 0x4   # RtVoxelDetach.flags (ABI 1.3, additive: voxel detachment)


class RtVoxelDetach(C.Structure):
    """rt_detach_voxels' parameters (ABI 1.3, additive: voxel detachment): 48 bytes; the reserved bytes must be 0."""
    _fields_ = [("lo", C.c_int32 * 3), ("flags", C.c_uint32), ("hi", C.c_int32 * 3), ("air_material", C.c_uint32), ("anchor_mask", C.c_uint32),
                ("anchor_value", C.c_uint32), ("max_passes", C.c_uint32), ("anchor_faces", C.c_uint8), ("reserved0", C.c_uint8 * 3)]


class RtDetachResult(C.Structure):
    """rt_detach_voxels' result: 48 bytes; the counters are added to, the bounds merged (min into lo, max into hi)."""
    _fields_ = [("detached", C.c_uint32), ("supported", C.c_uint32), ("passes", C.c_uint32), ("unconverged", C.c_uint32), ("lo", C.c_int32 * 3),
                ("chunks", C.c_uint32), ("hi", C.c_int32 * 3), ("reserved", C.c_uint32)]


assert C.sizeof(RtVoxelDetach) == 48 and C.sizeof(RtDetachResult) == 48
assert (RtVoxelDetach.flags.offset, RtVoxelDetach.hi.offset, RtVoxelDetach.air_material.offset, RtVoxelDetach.anchor_mask.offset,
        RtVoxelDetach.anchor_value.offset, RtVoxelDetach.max_passes.offset, RtVoxelDetach.anchor_faces.offset,
        RtVoxelDetach.reserved0.offset) == (12, 16, 28, 32, 36, 40, 44, 45)
assert (RtDetachResult.unconverged.offset, RtDetachResult.lo.offset, RtDetachResult.chunks.offset, RtDetachResult.hi.offset,
        RtDetachResult.reserved.offset) == (12, 16, 28, 32, 44)
DETACH_DTYPE = np.dtype(RtVoxelDetach)             # the numpy view of the parameters
DETACH_RESULT_DTYPE = np.dtype(RtDetachResult)     # ... and of the result
DETACH_MAX_PASSES = 256


def make_voxel_detach(lo, hi, flags=RT_DETACH_CARVE | RT_DETACH_CAPTURE, anchor_faces=0x10, air_material=0, anchor_mask=0, anchor_value=0,
                      max_passes=DETACH_MAX_PASSES):
    """An RtVoxelDetach: the box `lo`..`hi` of texels (inclusive, as a box shape's a and b), the RT_DETACH_* flags, the faces of the
    clipped box that anchor (bit 2k the low face of axis k, bit 2k + 1 the high one; the default is the low z face: the ground), the
    word left in carved cells, the mask test of anchoring materials and the pass limit.  Refuses what the calls refuse without
    knowing R: a box with lo > hi, an unknown flag, anchor_faces above 63, max_passes outside 1..256, an anchor_value bit outside
    anchor_mask, a mask or value without RT_DETACH_ANCHOR_MATERIAL.  The box's range and extent are judged by the call (it needs R)."""
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("lo and hi have three components")
    p = RtVoxelDetach()
    for k in range(3):
        p.lo[k], p.hi[k] = int(lo[k]), int(hi[k])
        if p.lo[k] > p.hi[k]:
            raise ValueError("the box needs lo <= hi on every axis")
    if int(flags) & ~(RT_DETACH_CARVE | RT_DETACH_CAPTURE | RT_DETACH_ANCHOR_MATERIAL):
        raise ValueError("flags holds an unknown bit")
    if not 0 <= int(anchor_faces) <= 63:
        raise ValueError("anchor_faces is 0..63")
    if not 1 <= int(max_passes) <= DETACH_MAX_PASSES:
        raise ValueError("max_passes is 1..256")
    if int(anchor_value) & ~int(anchor_mask):
        raise ValueError("anchor_value has a bit outside anchor_mask")
    if not int(flags) & RT_DETACH_ANCHOR_MATERIAL and (int(anchor_mask) or int(anchor_value)):
        raise ValueError("anchor_mask and anchor_value need RT_DETACH_ANCHOR_MATERIAL")
    p.flags, p.air_material, p.anchor_mask, p.anchor_value = int(flags), int(air_material), int(anchor_mask), int(anchor_value)
    p.max_passes, p.anchor_faces = int(max_passes), int(anchor_faces)
    return p


class RtVoxelFlow(C.Structure):
    """rt_flow_voxels' parameters (ABI 1.3, additive: fluid flow): 64 bytes; the reserved bytes and words must be 0."""
    _fields_ = [("lo", C.c_int32 * 3), ("ticks", C.c_uint32), ("hi", C.c_int32 * 3), ("air_material", C.c_uint32), ("fluid_mask", C.c_uint32),
                ("fluid_value", C.c_uint32), ("fluid_word", C.c_uint32), ("reserved0", C.c_uint32), ("level_shift", C.c_uint8), ("max_level", C.c_uint8),
                ("reserved1", C.c_uint8 * 2), ("reserved2", C.c_uint32 * 3)]


class RtFlowCount(C.Structure):
    """rt_flow_voxels' counters: 32 bytes, added to by every call; reserved is never written."""
    _fields_ = [("wetted", C.c_uint32), ("dried", C.c_uint32), ("changed", C.c_uint32), ("active", C.c_uint32), ("chunks", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


assert C.sizeof(RtVoxelFlow) == 64 and C.sizeof(RtFlowCount) == 32
assert (RtVoxelFlow.ticks.offset, RtVoxelFlow.hi.offset, RtVoxelFlow.air_material.offset, RtVoxelFlow.fluid_mask.offset, RtVoxelFlow.fluid_value.offset,
        RtVoxelFlow.fluid_word.offset, RtVoxelFlow.reserved0.offset, RtVoxelFlow.level_shift.offset, RtVoxelFlow.max_level.offset,
        RtVoxelFlow.reserved1.offset, RtVoxelFlow.reserved2.offset) == (12, 16, 28, 32, 36, 40, 44, 48, 49, 50, 52)
FLOW_DTYPE = np.dtype(RtVoxelFlow)                 # the numpy view of the parameters
FLOW_COUNT_DTYPE = np.dtype(RtFlowCount)           # ... and of the counters
FLOW_MAX_TICKS, FLOW_MAX_LEVEL, FLOW_MAX_SHIFT, FLOW_SOURCE = 256, 13, 28, 15   # ticks per call; max_level; level_shift; the level value of a source


def make_voxel_flow(lo, hi, fluid_mask, fluid_value, fluid_word=None, ticks=1, air_material=0, level_shift=0, max_level=7):
    """An RtVoxelFlow: the box `lo`..`hi` of texels (inclusive, as a box shape's a and b), the mask test that makes an occupied voxel
    this fluid, the word a newly wetted cell gets (None: fluid_value), the ticks of the call, the word left in dried cells, where the
    4-bit level field sits in a word and the strength next to a source.  Refuses what the calls refuse without knowing R: a box with
    lo > hi, ticks outside 1..256, level_shift above 28, max_level outside 1..13, a zero mask, a mask or word that meets the level
    field, a value outside the mask, a word that fails the test.  The box's range and extent are judged by the call (it needs R)."""
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("lo and hi have three components")
    p = RtVoxelFlow()
    for k in range(3):
        p.lo[k], p.hi[k] = int(lo[k]), int(hi[k])
        if p.lo[k] > p.hi[k]:
            raise ValueError("the box needs lo <= hi on every axis")
    fluid_word = fluid_value if fluid_word is None else fluid_word
    if not 1 <= int(ticks) <= FLOW_MAX_TICKS:
        raise ValueError("ticks is 1..256")
    if not 0 <= int(level_shift) <= FLOW_MAX_SHIFT or not 1 <= int(max_level) <= FLOW_MAX_LEVEL:
        raise ValueError("level_shift is 0..28 and max_level 1..13")
    field = 0xF << int(level_shift)
    if int(fluid_mask) == 0 or int(fluid_mask) & field or int(fluid_word) & field:
        raise ValueError("fluid_mask is not 0, and neither it nor fluid_word meets the level field")
    if int(fluid_value) & ~int(fluid_mask) or int(fluid_word) & int(fluid_mask) != int(fluid_value):
        raise ValueError("fluid_value lies inside fluid_mask and fluid_word passes the fluid test")
    p.ticks, p.air_material, p.fluid_mask, p.fluid_value, p.fluid_word = int(ticks), int(air_material), int(fluid_mask), int(fluid_value), int(fluid_word)
    p.level_shift, p.max_level = int(level_shift), int(max_level)
    return p


RT_NAV_UNREACHED, RT_NAV_NO_MOVE = 0xFFFF, 0xFF   # dist / move of a cell nothing leads from (ABI 1.3, additive: navigation fields)


class RtNavBuild(C.Structure):
    """rt_nav_build's parameters (ABI 1.3, additive: navigation fields): 32 bytes; the reserved words must be 0."""
    _fields_ = [("lo", C.c_int32 * 3), ("max_dist", C.c_uint32), ("height", C.c_uint8), ("max_climb", C.c_uint8), ("max_drop", C.c_uint8),
                ("goal_snap", C.c_uint8), ("reserved", C.c_uint32 * 3)]


class RtNavGoal(C.Structure):
    """One goal of rt_nav_build: 16 bytes, a texel."""
    _fields_ = [("cell", C.c_int32 * 3), ("reserved", C.c_uint32)]


class RtNavResult(C.Structure):
    """rt_nav_build's result: 32 bytes; the counters are added to, `levels` merged by maximum."""
    _fields_ = [("standable", C.c_uint32), ("reached", C.c_uint32), ("levels", C.c_uint32), ("truncated", C.c_uint32),
                ("goals_used", C.c_uint32), ("goals_dropped", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class RtNavAgent(C.Structure):
    """rt_nav_sample input: 16 bytes; the foot point, how far to look down (0..8) and up (0..2) for a reached cell."""
    _fields_ = [("pos", C.c_float * 3), ("snap_down", C.c_uint8), ("snap_up", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class RtNavStep(C.Structure):
    """rt_nav_sample output: 32 bytes."""
    _fields_ = [("cell", C.c_int32 * 3), ("dist", C.c_uint32), ("next", C.c_int32 * 3), ("move", C.c_uint32)]


assert (C.sizeof(RtNavBuild), C.sizeof(RtNavGoal), C.sizeof(RtNavResult), C.sizeof(RtNavAgent), C.sizeof(RtNavStep)) == (32, 16, 32, 16, 32)
assert (RtNavBuild.max_dist.offset, RtNavBuild.height.offset, RtNavBuild.max_climb.offset, RtNavBuild.max_drop.offset,
        RtNavBuild.goal_snap.offset, RtNavBuild.reserved.offset) == (12, 16, 17, 18, 19, 20)
assert (RtNavResult.levels.offset, RtNavResult.truncated.offset, RtNavResult.goals_used.offset, RtNavResult.goals_dropped.offset,
        RtNavResult.reserved.offset) == (8, 12, 16, 20, 24)
assert (RtNavAgent.snap_down.offset, RtNavAgent.snap_up.offset, RtNavAgent.reserved.offset) == (12, 13, 14)
assert (RtNavStep.dist.offset, RtNavStep.next.offset, RtNavStep.move.offset) == (12, 16, 28)
NAV_GOAL_DTYPE = np.dtype(RtNavGoal)       # the numpy views of the records
NAV_RESULT_DTYPE = np.dtype(RtNavResult)
NAV_AGENT_DTYPE = np.dtype(RtNavAgent)
NAV_STEP_DTYPE = np.dtype(RtNavStep)
MAX_NAV_FIELDS, MAX_NAV_EXTENT, MAX_NAV_DIST, MAX_NAV_GOALS, MAX_NAV_AGENTS = 64, 256, 4096, 4096, 1 << 20


def make_nav_build(lo, max_dist, height=2, max_climb=1, max_drop=3, goal_snap=0):
    """An RtNavBuild: the box's low corner `lo` in texels (its extent is the field's), the largest distance written, the walker's
    height in cells, how far it steps up and drops, and how far below a goal record its goal cell may lie.  Refuses what the call
    refuses without knowing R or the field: a parameter outside its range.  The box is judged by the call."""
    if len(lo) != 3:
        raise ValueError("lo has three components")
    for name, v, a, b in (("max_dist", max_dist, 1, MAX_NAV_DIST), ("height", height, 1, 4), ("max_climb", max_climb, 0, 2),
                          ("max_drop", max_drop, 0, 8), ("goal_snap", goal_snap, 0, 8)):
        if not a <= int(v) <= b:
            raise ValueError("%s is %d..%d" % (name, a, b))
    p = RtNavBuild()
    for k in range(3):
        p.lo[k] = int(lo[k])
    p.max_dist, p.height, p.max_climb, p.max_drop, p.goal_snap = int(max_dist), int(height), int(max_climb), int(max_drop), int(goal_snap)
    return p


def make_nav_goals(cells):
    """NAV_GOAL_DTYPE records from int[N, 3] texels (or ready records)."""
    if isinstance(cells, np.ndarray) and cells.dtype == NAV_GOAL_DTYPE:
        return np.ascontiguousarray(cells).reshape(-1)
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    out = np.zeros(len(cells), dtype=NAV_GOAL_DTYPE)
    out["cell"] = cells
    return out


def make_nav_agents(pos, snap_down=1, snap_up=1):
    """NAV_AGENT_DTYPE records from float[N, 3] foot points (or ready records); snap_down / snap_up are scalars or arrays of N."""
    if isinstance(pos, np.ndarray) and pos.dtype == NAV_AGENT_DTYPE:
        return np.ascontiguousarray(pos).reshape(-1)
    pos = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(len(pos), dtype=NAV_AGENT_DTYPE)
    out["pos"] = pos
    out["snap_down"] = snap_down
    out["snap_up"] = snap_up
    return out


class RtDrawStamp(C.Structure):
    """rt_draw_stamps input (ABI 1.3, additive: voxel-model entities): 32 bytes; the reserved fields must be 0."""
    _fields_ = [("origin", C.c_float * 3), ("scale", C.c_float), ("stamp", C.c_uint32), ("orient", C.c_uint8), ("reserved0", C.c_uint8 * 3),
                ("emission", C.c_uint32), ("reserved", C.c_uint32)]


assert C.sizeof(RtDrawStamp) == 32
assert (RtDrawStamp.origin.offset, RtDrawStamp.scale.offset, RtDrawStamp.stamp.offset, RtDrawStamp.orient.offset,
        RtDrawStamp.emission.offset, RtDrawStamp.reserved.offset) == (0, 12, 16, 20, 24, 28)
MAX_DRAW_STAMPS = 4096   # rt_draw_stamps: models per call


RT_ENTITY_NONE, RT_ENTITY_BOX, RT_ENTITY_MODEL = 0, 1, 2   # RtEntityHit.kind (ABI 1.3, additive: entity queries)


class RtEntityHit(C.Structure):
    """rt_trace_entities / rt_pick_entities result (ABI 1.3, additive): 48 bytes."""
    _fields_ = [("position", C.c_float * 3), ("t", C.c_float), ("kind", C.c_uint32), ("index", C.c_uint32), ("normal", C.c_uint32),
                ("material", C.c_uint32), ("cell", C.c_int32 * 3), ("voxel", C.c_uint32)]


assert C.sizeof(RtEntityHit) == 48
assert (RtEntityHit.t.offset, RtEntityHit.kind.offset, RtEntityHit.material.offset, RtEntityHit.cell.offset, RtEntityHit.voxel.offset) == (12, 16, 28, 32, 44)
MAX_ENTITY_RAYS = 1 << 24   # rt_trace_entities / rt_pick_entities: rays or pixels per call


class RtEntitySweepHit(C.Structure):
    """rt_sweep_entities result (ABI 1.3, additive: entity sweeps): 80 bytes."""
    _fields_ = [("t", C.c_float), ("kind", C.c_uint32), ("normal", C.c_uint32), ("material", C.c_uint32),
                ("entity", C.c_uint32), ("index", C.c_uint32), ("axis", C.c_uint32), ("voxel", C.c_uint32),
                ("cell", C.c_int32 * 3), ("reserved0", C.c_uint32), ("lo", C.c_float * 3), ("reserved1", C.c_uint32),
                ("hi", C.c_float * 3), ("reserved2", C.c_uint32)]


assert C.sizeof(RtEntitySweepHit) == 80
assert (RtEntitySweepHit.entity.offset, RtEntitySweepHit.voxel.offset, RtEntitySweepHit.cell.offset, RtEntitySweepHit.lo.offset,
        RtEntitySweepHit.hi.offset) == (16, 28, 32, 48, 64)
ENTITY_SWEEP_HIT_DTYPE = np.dtype(RtEntitySweepHit)   # the numpy view of the record
MAX_ENTITY_SWEEPS = 1 << 24   # rt_sweep_entities: sweeps per call


class RtPointLight(C.Structure):
    """rt_add_lights input (ABI 1.3, additive: point lights): 32 bytes; `reserved` must be 0."""
    _fields_ = [("position", C.c_float * 3), ("radius", C.c_float), ("color", C.c_float * 3), ("reserved", C.c_uint32)]


assert C.sizeof(RtPointLight) == 32
assert (RtPointLight.position.offset, RtPointLight.radius.offset, RtPointLight.color.offset, RtPointLight.reserved.offset) == (0, 12, 16, 28)
MAX_POINT_LIGHTS = 1024   # rt_add_lights: lights per call


class RtDenoiseParams(C.Structure):
    """rt_denoise_history / rt_denoise_planes_counted parameters (ABI 1.3, additive): 48 bytes; `reserved` must be 0."""
    _fields_ = [("struct_size", C.c_uint32), ("faithful", C.c_int32), ("weight_by_count", C.c_int32), ("settle", C.c_uint32 * 6),
                ("reserved", C.c_uint32 * 3)]


assert C.sizeof(RtDenoiseParams) == 48
