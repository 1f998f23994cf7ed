"""Python binding of the ray-trace path.

Two layers, both thin ctypes wrappers (all logic lives in the native libraries):

* `Context`  — the C ABI of include/rt_abi.h, one object per GPU context (rt_create ... rt_destroy).
* `Camera`, `Game`, `Pipeline`, `create_instance` — the C++ host mirror of the reference's public `render` API
  (src/render/mod.rs:20-43, src/render/pipeline/pipeline.rs:134-255, src/game/mod.rs:37-58), so that tests read
  like a user of the reference: `game = Game(); pipeline = create_instance(cfg, game); pipeline.draw_frame(game)`.
"""
import ctypes as C
import math

import numpy as np

from . import _lib, abi
from .abi import (BUFFER_FORMATS, BUFFER_NAMES, MAX_ENTITY_SWEEPS, MAX_DRAW_BOXES, MAX_DRAW_STAMPS, MAX_ENTITY_RAYS, MAX_PARTICLE_LIGHTS, MAX_PARTICLES, MAX_POINT_LIGHTS, RT_BUF_COUNT, RT_BUF_FINAL_BGRA8, RT_KERNEL_DEFAULT, RT_SHAPE_BOX, RT_SHAPE_SPHERE,
                  RT_SWEEP_BLOCKED, RT_SWEEP_FREE, RT_WHERE_ALL, RtBoxSweep, RtConfig, RtCounters, RtDenoiseParams, RtDrawBox, RtDrawStamp, RtEntityHit, RtInfo, RtLightProbe,
                  RtPointLight, RtProbeLight, RtRayHit, RtShapeEdit, RtStampPlace, RtSweepHit, RtTiming, RtUniforms, RtVoxelEdit)


class RtError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("rt error %d: %s" % (code, message))
        self.code = code


def make_config(width, height, spp=1, depth=2, device=0, tile_rank=0, tile_world=1, kernel=RT_KERNEL_DEFAULT, flags=0,
                region=256, history_cap=0, edit_radius=0, stream_history=0):
    cfg = RtConfig()
    cfg.struct_size = C.sizeof(RtConfig)
    cfg.width, cfg.height, cfg.region = int(width), int(height), int(region)
    cfg.spp, cfg.depth, cfg.device = int(spp), int(depth), int(device)
    cfg.tile_rank, cfg.tile_world = int(tile_rank), int(tile_world)
    cfg.kernel, cfg.flags = int(kernel), int(flags)
    cfg.history_cap = int(history_cap)   # RT_FLAG_REPROJECT: 0 = the default (32)
    cfg.edit_radius = int(edit_radius)   # RT_FLAG_REPROJECT: 0 = an edit restarts the history; 1..64 = only near the edit
    cfg.stream_history = int(stream_history)   # RT_FLAG_REPROJECT: 0 = a slab restarts the history; 1 = only near what left or arrived
    return cfg


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _ptr_or_none(a):
    """The host array's address, or NULL for an empty one (the library takes NULL with a count of 0)."""
    return _p(a) if a.size else None


def _dp(t):
    """A device tensor's address (NULL for None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _lr3(v):
    """An int32[3] argument: a render offset `lr`, a texel, an extent."""
    return (C.c_int32 * 3)(*[int(x) for x in v])


def _records(x, dtype):
    """Host data as the library reads it: a contiguous flat array of `dtype`; None is the empty array."""
    return np.zeros(0, dtype=dtype) if x is None else np.ascontiguousarray(x, dtype=dtype).reshape(-1)


def _rows(rows, dtype):
    """A ready array of `dtype` records, or a sequence of single rows (box_shape, stamp_place), as contiguous records."""
    if not (isinstance(rows, np.ndarray) and rows.dtype == dtype):
        rows = np.array([np.asarray(s, dtype=dtype) for s in rows], dtype=dtype)
    return np.ascontiguousarray(rows).reshape(-1)


def _entity_records(boxes, models):
    """The entity calls' host records: contiguous DRAW_BOX_DTYPE and DRAW_STAMP_DTYPE arrays (empty for None)."""
    return _records(boxes, DRAW_BOX_DTYPE), _records(models, DRAW_STAMP_DTYPE)


def _face_lights(face_lights, n, what):
    """The PROBE_LIGHT_DTYPE records that light `n` entities' faces: six per entity, or a ValueError."""
    lights = _records(face_lights, PROBE_LIGHT_DTYPE)
    if lights.size != 6 * n:
        raise ValueError("face_lights must hold six records per %s" % what)
    return lights


def _rays(origins, directions):
    """float32[N, 8] RtRay rows (origin, pad, direction, pad) from float[N, 3] origins and directions."""
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("origins and directions must have the same shape [N, 3]")
    rays = np.zeros((o.shape[0], 8), dtype=np.float32)
    rays[:, 0:3], rays[:, 4:7] = o, d
    return rays


def _pick_result(hit, adjacent, world, **more):
    """What Pipeline.pick and pick_entity return: the world's hit record, its fields as Python values, and the two texels."""
    h = hit[0]
    return dict(more, hit=h, texel=tuple(int(v) for v in h["texel"]), normal=int(h["normal"]), kind=int(h["kind"]),
                adjacent=tuple(adjacent[:]), world=tuple(world[:]))


# The measured settle thresholds of rt_denoise_history (DESIGN.md "History-aware denoise"): the size-1 dispatch filters everybody,
# pixels with 16 / 8 / 4 / 4 / 2 samples or more sit out the dispatches of size 2 / 4 / 8 / 8 / 16, taps are not weighted by their
# counts.  On the measurement scene this lowers the error against a converged frame over all surface pixels and over those with 8
# samples or more, in both bindings, and leaves fresh pixels where plain rt_denoise puts them; count weighting lowers the error of
# old pixels further but raises that of fresh ones, so it is offered and not part of the preset.
HISTORY_DENOISE_PRESET = dict(weight_by_count=False, settle=(0, 16, 8, 4, 4, 2))


def denoise_params(faithful=True, weight_by_count=False, settle=(0, 0, 0, 0, 0, 0)):
    """An RtDenoiseParams block (include/rt_abi.h); the defaults are the neutral parameters, which give rt_denoise's result."""
    p = RtDenoiseParams()
    p.struct_size = C.sizeof(RtDenoiseParams)
    p.faithful = 1 if faithful else 0
    p.weight_by_count = 1 if weight_by_count else 0
    settle = tuple(int(v) for v in settle)
    if len(settle) != 6:
        raise ValueError("settle holds one threshold per dispatch: six")
    for i, v in enumerate(settle):
        p.settle[i] = v
    return p


# numpy views of the ABI's records: each layout is written once, as the ctypes struct in abi.py (tests/test_record_layouts.py pins them)
HIT_DTYPE = np.dtype(RtRayHit)
PROBE_DTYPE, PROBE_LIGHT_DTYPE = np.dtype(RtLightProbe), np.dtype(RtProbeLight)
SWEEP_DTYPE, SWEEP_HIT_DTYPE = np.dtype(RtBoxSweep), np.dtype(RtSweepHit)
DRAW_BOX_DTYPE = np.dtype(RtDrawBox)
DRAW_STAMP_DTYPE = np.dtype(RtDrawStamp)
ENTITY_HIT_DTYPE = np.dtype(RtEntityHit)
POINT_LIGHT_DTYPE = np.dtype(RtPointLight)
SHAPE_DTYPE = np.dtype(RtShapeEdit)
STAMP_PLACE_DTYPE = np.dtype(RtStampPlace)
VOXEL_EDIT_DTYPE = np.dtype(RtVoxelEdit)


def box_shape(lo, hi, material=0, solid=True, where=RT_WHERE_ALL):
    """One RtShapeEdit row: the box of texels lo..hi (x, y, z), both corners inclusive."""
    s = np.zeros((), dtype=SHAPE_DTYPE)
    s["a"], s["b"] = [int(v) for v in lo], [int(v) for v in hi]
    s["material"], s["kind"], s["where"], s["solid"] = int(material) & 0xFFFFFFFF, RT_SHAPE_BOX, int(where), 1 if solid else 0
    return s


def sphere_shape(centre, radius, material=0, solid=True, where=RT_WHERE_ALL):
    """One RtShapeEdit row: the sphere of `radius` texels round `centre`, in texel coordinates with a voxel's centre at x + 0.5 —
    both in half texels at most (centre (10.5, 10.5, 10.5), radius 3.5: the sphere round voxel (10, 10, 10))."""
    c2 = [2.0 * float(v) for v in centre]
    d = 2.0 * float(radius)
    if any(v != math.floor(v) for v in c2) or d != math.floor(d) or d < 0:
        raise ValueError("a sphere's centre and radius are whole or half texels")
    s = np.zeros((), dtype=SHAPE_DTYPE)
    s["a"], s["b"] = [int(v) for v in c2], [int(d) * int(d), 0, 0]
    s["material"], s["kind"], s["where"], s["solid"] = int(material) & 0xFFFFFFFF, RT_SHAPE_SPHERE, int(where), 1 if solid else 0
    return s


def stamp_place(stamp, at, orient=0, where=RT_WHERE_ALL):
    """One RtStampPlace row: stamp `stamp` with the low corner of its oriented box at texel `at` (x, y, z); orient = p << 3 | f."""
    s = np.zeros((), dtype=STAMP_PLACE_DTYPE)
    s["at"], s["stamp"], s["orient"], s["where"] = [int(v) for v in at], int(stamp), int(orient), int(where)
    return s


# Texel step from a hit voxel to the empty neighbour in front of the face the ray crossed, per normal code (raytrace.comp:89-93): an
# even code means the ray travelled towards -axis, so it came from +axis.
FACE_STEP = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=np.int64)


def adjacent_texel(texel, normal, region=256):
    """Texel in front of face `normal` of `texel` (where a placed block goes), wrapped mod R."""
    t = np.asarray(texel, dtype=np.int64)
    return (t + FACE_STEP[np.asarray(normal, dtype=np.int64)]) % int(region)


def texel_to_world(texel, lr=(0, 0, 0), region=256):
    """World coordinate of `texel` inside the window the region covers for render offset `lr`: texel = world + R/2 (mod R) and
    lr - R/2 <= world < lr + R/2 (raytrace.comp:104-105,138-145)."""
    t = np.asarray(texel, dtype=np.int64)
    lr = np.asarray(lr, dtype=np.int64)
    R = int(region)
    return lr - R // 2 + (t - lr) % R


def row_from_bottom(y_from_top, height):
    """Frame row of a screen row counted from the top: the planes' row 0 is the bottom of the view."""
    return int(height) - 1 - np.asarray(y_from_top)


class Context:
    """Owns one RtContext*.  Use as a context manager or call destroy()."""

    def __init__(self, cfg=None, handle=None, owned=True):
        self._lib = _lib.amd()
        self._owned = owned
        if handle is not None:
            self._h = C.c_void_p(handle)
            self.cfg = cfg
            return
        h = C.c_void_p()
        rc = self._lib.rt_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise RtError(rc, self._lib.rt_last_error(None).decode())
        self._h = h
        self.cfg = cfg

    # -- lifecycle ---------------------------------------------------------------------------------------
    def destroy(self):
        self._retire_staging_views()
        if self._h and self._owned:
            self._lib.rt_destroy(self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise RtError(rc, self._lib.rt_last_error(self._h).decode())

    @property
    def handle(self):
        return self._h

    @property
    def _device(self):
        return self.cfg.device if self.cfg is not None else 0

    @property
    def _region(self):
        return self.cfg.region if self.cfg is not None else 256

    # -- uploads -----------------------------------------------------------------------------------------
    def upload_world(self, materials, minefield):
        materials, minefield = _records(materials, np.uint32), _records(minefield, np.uint8)
        n = self._region ** 3
        if materials.size != n or minefield.size != n:
            raise ValueError("world arrays must hold region^3 voxels")
        self._check(self._lib.rt_upload_world(self._h, _p(materials), _p(minefield)))

    def slice_staging(self):
        """rt_slice_staging: (materials u32[16 R^2], minefield u8[16 R^2]) views of the library's pinned slab staging — fill them
        and pass them to upload_slice to skip the copy into the staging buffer.  The memory belongs to the context: the views are
        writable from this call until the next upload_slice (which hands the buffer to the device and makes them read-only: there
        are two staging sets, ask again for every slab) and dead after destroy() — do not keep them."""
        pm, pf = C.c_void_p(), C.c_void_p()
        self._check(self._lib.rt_slice_staging(self._h, C.byref(pm), C.byref(pf)))
        n = 16 * self._region ** 2
        mats = np.ctypeslib.as_array(C.cast(pm, C.POINTER(C.c_uint32)), shape=(n,))
        mine = np.ctypeslib.as_array(C.cast(pf, C.POINTER(C.c_uint8)), shape=(n,))
        self._staging_views = (mats, mine)
        return mats, mine

    def _retire_staging_views(self):
        for v in getattr(self, "_staging_views", None) or ():
            v.flags.writeable = False       # a write after the hand-over would race with the host-to-device copy
        self._staging_views = None

    def upload_slice(self, axis, texel_offset, materials, minefield):
        materials, minefield = _records(materials, np.uint32), _records(minefield, np.uint8)
        n = 16 * self._region ** 2
        if materials.size != n or minefield.size != n:
            raise ValueError("slice arrays must hold 16*region*region voxels")
        try:
            self._check(self._lib.rt_upload_slice(self._h, int(axis), int(texel_offset), _p(materials), _p(minefield)))
        finally:
            self._retire_staging_views()

    def edit_voxels(self, xyz, materials, solid):
        """rt_edit_voxels: xyz int[N, 3] texel coordinates (x, y, z), materials u32[N] packed words, solid bool/int[N].  Later rows
        win over earlier rows for the same voxel; the touched 64^3 chunks get pack_into's minefield (see include/rt_abi.h)."""
        xyz = np.asarray(xyz).reshape(-1, 3)
        materials = np.asarray(materials, dtype=np.uint32).reshape(-1)
        solid = np.asarray(solid).reshape(-1)
        n = xyz.shape[0]
        if materials.size != n or solid.size != n:
            raise ValueError("xyz, materials and solid must describe the same number of edits")
        if n and (xyz.min() < 0 or xyz.max() > 0xFFFF):
            raise ValueError("coordinates must fit uint16 (the library checks them against the region)")
        recs = np.zeros(n, dtype=VOXEL_EDIT_DTYPE)
        recs["x"], recs["y"], recs["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        recs["solid"] = solid != 0
        recs["material"] = materials
        self.edit_records(recs)

    def edit_records(self, recs):
        """rt_edit_voxels on a ready array of RtVoxelEdit records (numpy structured array of 16-byte rows, reserved included)."""
        recs = np.ascontiguousarray(recs)
        assert recs.dtype.itemsize == VOXEL_EDIT_DTYPE.itemsize
        self._check(self._lib.rt_edit_voxels(self._h, recs.ctypes.data_as(C.POINTER(RtVoxelEdit)), int(recs.size)))

    def edit_shapes(self, shapes):
        """rt_edit_shapes: a sequence of box_shape / sphere_shape rows, or a ready SHAPE_DTYPE array (32-byte RtShapeEdit rows),
        applied in order on the device; every 64^3 chunk that meets a shape's bounding box is rebuilt (see include/rt_abi.h)."""
        shapes = _rows(shapes, SHAPE_DTYPE)
        self._check(self._lib.rt_edit_shapes(self._h, shapes.ctypes.data_as(C.POINTER(RtShapeEdit)), int(shapes.size)))

    def stamp_create(self, materials, state):
        """rt_stamp_create: a stamp from materials u32[ez, ey, ex] and state u8[ez, ey, ex] (0 absent, 1 air, 2 solid); returns its id."""
        materials = np.ascontiguousarray(materials, dtype=np.uint32)
        state = np.ascontiguousarray(state, dtype=np.uint8)
        if materials.ndim != 3 or materials.shape != state.shape:
            raise ValueError("materials and state are [ez, ey, ex] arrays of one shape")
        out = C.c_uint32(0)
        self._check(self._lib.rt_stamp_create(self._h, _lr3(materials.shape[::-1]), _p(materials), _p(state), C.byref(out)))
        return out.value

    def stamp_capture(self, lo, extent, flags=0):
        """rt_stamp_capture: a stamp from the resident region's box at texel `lo` (x, y, z) of `extent` (ex, ey, ez), copied on the
        device in stream order; RT_STAMP_SKIP_AIR leaves the unoccupied voxels out of it.  Returns its id."""
        out = C.c_uint32(0)
        self._check(self._lib.rt_stamp_capture(self._h, _lr3(lo), _lr3(extent), int(flags), C.byref(out)))
        return out.value

    def stamp_info(self, stamp):
        """rt_stamp_info: the stamp's extent (ex, ey, ez)."""
        ext = (C.c_int32 * 3)()
        self._check(self._lib.rt_stamp_info(self._h, int(stamp), ext))
        return tuple(ext)

    def stamp_read(self, stamp):
        """rt_stamp_read: (materials u32[ez, ey, ex], state u8[ez, ey, ex]) of the stamp.  Synchronises."""
        ex, ey, ez = self.stamp_info(stamp)
        mats = np.empty((ez, ey, ex), dtype=np.uint32)
        state = np.empty((ez, ey, ex), dtype=np.uint8)
        self._check(self._lib.rt_stamp_read(self._h, int(stamp), _p(mats), _p(state)))
        return mats, state

    def stamp_destroy(self, stamp):
        """rt_stamp_destroy: the id is invalid afterwards; placements already enqueued still read the stamp."""
        self._check(self._lib.rt_stamp_destroy(self._h, int(stamp)))

    def edit_stamps(self, places):
        """rt_edit_stamps: a sequence of stamp_place rows, or a ready STAMP_PLACE_DTYPE array (32-byte RtStampPlace rows), pasted in
        order on the device; every 64^3 chunk that meets a placement's bounding box is rebuilt (see include/rt_abi.h)."""
        places = _rows(places, STAMP_PLACE_DTYPE)
        self._check(self._lib.rt_edit_stamps(self._h, places.ctypes.data_as(C.POINTER(RtStampPlace)), int(places.size)))

    def read_box(self, origin, extent):
        """rt_read_box: (materials u32[ez, ey, ex], minefield u8[ez, ey, ex]) of the resident region's box at texel `origin` (x, y, z)
        of `extent` (ex, ey, ez).  Synchronises."""
        x0, y0, z0 = (int(v) for v in origin)
        ex, ey, ez = (int(v) for v in extent)
        shape = (max(ez, 0), max(ey, 0), max(ex, 0))
        mats = np.empty(shape, dtype=np.uint32)
        mine = np.empty(shape, dtype=np.uint8)
        self._check(self._lib.rt_read_box(self._h, x0, y0, z0, ex, ey, ez, _p(mats), _p(mine)))
        return mats, mine

    def generate_world(self, seed, window_lo=None):
        """rt_generate_world: the procedural world of `seed` generated on the device into the whole region — the window
        [lo, lo + R) on every axis, window_lo None = (-R/2, -R/2, -R/2), i.e. world.generate_region(seed, R); any other window
        (multiples of 16) equals world.toroidal_region(lo + R/2, seed, R).  Asynchronous; makes the world resident."""
        lo = None if window_lo is None else (C.c_int64 * 3)(*[int(v) for v in window_lo])
        self._check(self._lib.rt_generate_world(self._h, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), lo))

    def generate_slice(self, seed, axis, window_lo):
        """rt_generate_slice: one 16-thick slab generated on the device — [lo[axis], lo[axis] + 16) along `axis`, [lo, lo + R)
        along the other two, every voxel at texel (v + R/2) mod R (world.slice_window turns a streamer's request into it)."""
        lo = (C.c_int64 * 3)(*[int(v) for v in window_lo])
        self._check(self._lib.rt_generate_slice(self._h, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(axis), lo))

    def upload_noise(self, rgba8):
        rgba8 = _records(rgba8, np.uint8)
        if rgba8.size != 512 * 512 * 4:
            raise ValueError("noise must be 512x512 RGBA8")
        self._check(self._lib.rt_upload_noise(self._h, _p(rgba8)))

    # -- ray queries -------------------------------------------------------------------------------------
    def trace_rays(self, origins, directions, lr=(0, 0, 0)):
        """rt_trace_rays: float[N, 3] origins and directions -> numpy array of HIT_DTYPE (RtRayHit) per ray.  Synchronous."""
        rays = _rays(origins, directions)
        hits = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
        self._check(self._lib.rt_trace_rays(self._h, _p(rays), rays.shape[0], _lr3(lr), _p(hits)))
        return hits

    def trace_rays_async(self, rays, hits, lr=(0, 0, 0)):
        """rt_trace_rays_async on torch device tensors: `rays` float32[N, 8] (origin, pad, direction, pad per row), `hits` any
        contiguous tensor of N * 48 bytes (e.g. uint8[N, 48] or int32[N, 12]).  Enqueued: valid after sync(), or in the order of a
        stream given to set_stream().  `rays` must be complete on the device when the call is made (the query is not ordered
        after the caller's stream unless that stream was given to set_stream())."""
        n = check_query_tensors(rays, hits, self._device)
        self._check(self._lib.rt_trace_rays_async(self._h, _dp(rays), n, _lr3(lr), _dp(hits)))

    def pick_pixels(self, uniforms, xy):
        """rt_pick_pixels: int[N, 2] whole-frame pixels (x, y), row 0 = bottom, of the camera in `uniforms` -> HIT_DTYPE[N]."""
        xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
        hits = np.zeros(xy.shape[0], dtype=HIT_DTYPE)
        self._check(self._lib.rt_pick_pixels(self._h, C.byref(uniforms), _p(xy), int(xy.shape[0]), _p(hits)))
        return hits

    # -- entity queries ----------------------------------------------------------------------------------
    def trace_entities(self, origins, directions, lr=(0, 0, 0), boxes=None, models=None):
        """rt_trace_entities: float[N, 3] origins and directions against the resident world and the drawn `boxes` (DRAW_BOX_DTYPE[B]) and
        `models` (DRAW_STAMP_DTYPE[M]) -> (world_hits HIT_DTYPE[N], entity_hits ENTITY_HIT_DTYPE[N]).  Synchronous; an invalid record
        fails the whole call (RtError, INVALID_ARG).  Rays that lie together should follow each other: a wave of 64 culls as one."""
        rays = _rays(origins, directions)
        boxes, models = _entity_records(boxes, models)
        world = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
        hits = np.zeros(rays.shape[0], dtype=ENTITY_HIT_DTYPE)
        self._check(self._lib.rt_trace_entities(self._h, _p(rays), rays.shape[0], _lr3(lr), _ptr_or_none(boxes), boxes.size,
                                                _ptr_or_none(models), models.size, _p(world), _p(hits)))
        return world, hits

    def pick_entities(self, uniforms, xy, boxes=None, models=None):
        """rt_pick_entities: int[N, 2] whole-frame pixels (x, y), row 0 = bottom, of the camera in `uniforms` -> (world_hits HIT_DTYPE[N]
        as pick_pixels gives them, entity_hits ENTITY_HIT_DTYPE[N]): kind != RT_ENTITY_NONE where rt_draw_boxes / rt_draw_stamps with the
        same records draw an entity into that pixel."""
        xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
        boxes, models = _entity_records(boxes, models)
        world = np.zeros(xy.shape[0], dtype=HIT_DTYPE)
        hits = np.zeros(xy.shape[0], dtype=ENTITY_HIT_DTYPE)
        self._check(self._lib.rt_pick_entities(self._h, C.byref(uniforms), _p(xy), xy.shape[0], _ptr_or_none(boxes), boxes.size,
                                               _ptr_or_none(models), models.size, _p(world), _p(hits)))
        return world, hits

    def trace_entities_async(self, rays, boxes, models, world_hits, entity_hits, lr=(0, 0, 0)):
        """rt_trace_entities_async on torch device tensors: `rays` float32[N, 8] as for trace_rays_async, `boxes` any contiguous tensor of
        B * 32 bytes (RtDrawBox rows) or None, `world_hits` any contiguous tensor of N * 48 bytes or None, `entity_hits` likewise (not
        None); `models` host records as for draw_stamps_async (free again on return).  Enqueued: valid after sync(), or in the order of
        a stream given to set_stream().  An invalid box is skipped on the device, an invalid model fails the call."""
        n, nb = check_entity_query_tensors(rays, boxes, world_hits, entity_hits, self._device)
        models = _records(models, DRAW_STAMP_DTYPE)
        self._check(self._lib.rt_trace_entities_async(self._h, _dp(rays), n, _lr3(lr), _dp(boxes) if nb else None, nb,
                                                      _ptr_or_none(models), models.size, _dp(world_hits), _dp(entity_hits)))

    # -- light probes ------------------------------------------------------------------------------------
    def probe_light(self, uniforms, positions, normals, cells, samples, depth):
        """rt_probe_light: float[N, 3] positions, int[N] normal codes (0..5, or RT_PROBE_SPHERE), int[N, 2] noise cells ->
        numpy array of PROBE_LIGHT_DTYPE (RtProbeLight) per probe: the mean light of `samples` paths of `depth` levels from each
        surface under the sun_angle, seed and lr of `uniforms`.  Synchronous."""
        return self.probe_records(uniforms, make_probes(positions, normals, cells), samples, depth)

    def probe_records(self, uniforms, probes, samples, depth):
        """rt_probe_light on a ready array of RtLightProbe records (numpy PROBE_DTYPE rows, reserved included)."""
        probes = np.ascontiguousarray(probes)
        assert probes.dtype.itemsize == PROBE_DTYPE.itemsize
        out = np.zeros(probes.size, dtype=PROBE_LIGHT_DTYPE)
        self._check(self._lib.rt_probe_light(self._h, C.byref(uniforms), _p(probes), int(probes.size), int(samples), int(depth), _p(out)))
        return out

    def probe_light_async(self, uniforms, probes, out, samples, depth):
        """rt_probe_light_async on torch device tensors: `probes` any contiguous tensor of N * 32 bytes (RtLightProbe rows, e.g.
        uint8[N, 32] from make_probes), `out` any contiguous tensor of N * 16 bytes (e.g. float32[N, 4]: light rgb, then the bits of
        sun_samples).  Enqueued: valid after sync(), or in the order of a stream given to set_stream().  `probes` must be complete
        on the device when the call is made."""
        n = check_probe_tensors(probes, out, self._device)
        self._check(self._lib.rt_probe_light_async(self._h, C.byref(uniforms), _dp(probes), n, int(samples), int(depth), _dp(out)))

    # -- box sweeps --------------------------------------------------------------------------------------
    def sweep_boxes(self, sweeps, lr=(0, 0, 0)):
        """rt_sweep_boxes: `sweeps` float[N, 3, 3] (lo, hi, motion per row) or SWEEP_DTYPE[N] records -> numpy array of SWEEP_HIT_DTYPE
        (RtSweepHit) per sweep.  Synchronous; a record outside the validated domain fails the whole call (RtError, INVALID_ARG)."""
        recs = make_sweeps(sweeps)
        hits = np.zeros(recs.size, dtype=SWEEP_HIT_DTYPE)
        self._check(self._lib.rt_sweep_boxes(self._h, _p(recs), recs.size, _lr3(lr), _p(hits)))
        return hits

    def sweep_boxes_async(self, sweeps, hits, lr=(0, 0, 0)):
        """rt_sweep_boxes_async on torch device tensors: `sweeps` any contiguous tensor of N * 48 bytes (RtBoxSweep rows, e.g.
        float32[N, 12]), `hits` any contiguous tensor of N * 64 bytes.  Enqueued: valid after sync(), or in the order of a stream
        given to set_stream().  `sweeps` must be complete on the device when the call is made.  A record outside the validated
        domain gets kind RT_SWEEP_INVALID."""
        n = check_sweep_tensors(sweeps, hits, self._device)
        self._check(self._lib.rt_sweep_boxes_async(self._h, _dp(sweeps), n, _lr3(lr), _dp(hits)))

    def move_and_slide(self, lo, hi, motion, lr=(0, 0, 0), iterations=3):
        """The character-controller loop over rt_sweep_boxes: sweep; on BLOCKED take the returned box, zero the blocked axis of
        motion * (1 - t) and sweep again; stop on FREE, on a zero remainder or after `iterations` sweeps (an EMBEDDED start stops at
        once, where it is).  Returns (lo, hi, hits): the final box as float32[3] arrays and the list of SWEEP_HIT_DTYPE records."""
        lo, hi, m = (np.asarray(v, dtype=np.float32).reshape(3).copy() for v in (lo, hi, motion))
        hits = []
        for _ in range(int(iterations)):
            h = self.sweep_boxes(np.stack([lo, hi, m])[None], lr)[0]
            hits.append(h)
            if h["kind"] not in (RT_SWEEP_FREE, RT_SWEEP_BLOCKED):
                break
            lo, hi = h["lo"].copy(), h["hi"].copy()
            if h["kind"] == RT_SWEEP_FREE:
                break
            m = m * (np.float32(1.0) - h["t"])
            m[int(h["axis"])] = 0
            if not m.any():
                break
        return lo, hi, hits

    # -- entity sweeps -----------------------------------------------------------------------------------
    def sweep_entities(self, sweeps, lr=(0, 0, 0), boxes=None, models=None, world=True):
        """rt_sweep_entities: `sweeps` as for sweep_boxes (SWEEP_DTYPE records carry the self exemption: reserved0 = 1 + the index of
        the box a sweep ignores, reserved1 likewise for models) against the resident world and the drawn `boxes` (DRAW_BOX_DTYPE[B]) and
        `models` (DRAW_STAMP_DTYPE[M]) -> (world_hits SWEEP_HIT_DTYPE[N] — what sweep_boxes returns; None with world=False —,
        entity_hits abi.ENTITY_SWEEP_HIT_DTYPE[N]).  Synchronous; an invalid record fails the whole call (RtError, INVALID_ARG)."""
        recs = make_sweeps(sweeps)
        boxes, models = _entity_records(boxes, models)
        world_hits = np.zeros(recs.size, dtype=SWEEP_HIT_DTYPE) if world else None
        hits = np.zeros(recs.size, dtype=abi.ENTITY_SWEEP_HIT_DTYPE)
        self._check(self._lib.rt_sweep_entities(self._h, _p(recs), recs.size, _lr3(lr), _ptr_or_none(boxes), boxes.size, _ptr_or_none(models),
                                                models.size, _p(world_hits) if world else None, _p(hits)))
        return world_hits, hits

    def sweep_entities_async(self, sweeps, boxes, models, world_hits, entity_hits, lr=(0, 0, 0)):
        """rt_sweep_entities_async on torch device tensors: `sweeps` any contiguous tensor of N * 48 bytes (RtBoxSweep rows), `boxes` any
        contiguous tensor of B * 32 bytes (RtDrawBox rows) or None, `world_hits` any contiguous tensor of N * 64 bytes or None,
        `entity_hits` any contiguous tensor of N * 80 bytes; `models` host records as for draw_stamps_async (free again on return).
        Enqueued: valid after sync(), or in the order of a stream given to set_stream().  A sweep outside the domain gets kind
        RT_SWEEP_INVALID, an invalid box is skipped on the device, an invalid model fails the call."""
        n, nb = entity_sweep_tensor_counts(sweeps, boxes, world_hits, entity_hits, self._device)
        models = _records(models, DRAW_STAMP_DTYPE)
        self._check(self._lib.rt_sweep_entities_async(self._h, _dp(sweeps), n, _lr3(lr), _dp(boxes) if nb else None, nb,
                                                      _ptr_or_none(models), models.size, _dp(world_hits), _dp(entity_hits)))

    def move_box_entities(self, lo, hi, motion, lr=(0, 0, 0), boxes=None, models=None, self_box=None, self_model=None, iterations=3):
        """move_and_slide's character-controller loop over rt_sweep_entities: sweep; take the combined box; when the world or an
        entity blocked, zero the blocked axis of motion * (1 - t) and sweep again.  It stops on a free sweep, on a zero remainder,
        after `iterations` sweeps, and at once — where it is — on a start embedded in the world or in an entity (entities move: the
        host resolves that) or outside the domain.  `self_box` / `self_model`: the index of the mover's own record in `boxes` /
        `models`, which the sweeps ignore.  Returns (lo, hi, hits): the final box and the list of (world_hit, entity_hit) records."""
        lo, hi, m = (np.asarray(v, dtype=np.float32).reshape(3).copy() for v in (lo, hi, motion))
        hits = []
        for _ in range(int(iterations)):
            rec = np.zeros(1, dtype=SWEEP_DTYPE)
            rec["lo"], rec["hi"], rec["motion"] = lo, hi, m
            rec["reserved0"] = 0 if self_box is None else int(self_box) + 1
            rec["reserved1"] = 0 if self_model is None else int(self_model) + 1
            world, ent = self.sweep_entities(rec, lr, boxes, models)
            w, e = world[0], ent[0]
            hits.append((w, e))
            if e["kind"] not in (RT_SWEEP_FREE, RT_SWEEP_BLOCKED) or w["kind"] not in (RT_SWEEP_FREE, RT_SWEEP_BLOCKED):
                break
            lo, hi = e["lo"].copy(), e["hi"].copy()
            stop = e if e["kind"] == RT_SWEEP_BLOCKED else w   # (a reported entity block came first: t_e < W.t)
            if stop["kind"] == RT_SWEEP_FREE:
                break
            m = m * (np.float32(1.0) - stop["t"])
            m[int(stop["axis"])] = 0
            if not m.any():
                break
        return lo, hi, hits

    # -- entity boxes ------------------------------------------------------------------------------------
    def draw_boxes(self, uniforms, boxes, face_lights):
        """rt_draw_boxes: `boxes` DRAW_BOX_DTYPE[N] records (make_draw_boxes) and `face_lights` PROBE_LIGHT_DTYPE[6 N] records (what
        probe_records returns for face_probes(boxes, ...)), composited by depth into the planes of the frame drawn last under the camera
        of `uniforms`.  Synchronous; an invalid box fails the whole call (RtError, INVALID_ARG)."""
        boxes = _records(boxes, DRAW_BOX_DTYPE)
        lights = _face_lights(face_lights, boxes.size, "box")
        self._check(self._lib.rt_draw_boxes(self._h, C.byref(uniforms), _ptr_or_none(boxes), _ptr_or_none(lights), boxes.size))

    def draw_boxes_async(self, uniforms, boxes, face_lights):
        """rt_draw_boxes_async on torch device tensors: `boxes` any contiguous tensor of N * 32 bytes (RtDrawBox rows), `face_lights` any
        contiguous tensor of 6 N * 16 bytes (e.g. the `out` of probe_light_async).  Enqueued behind the frame drawn last and the queries
        enqueued so far; an invalid box is skipped on the device."""
        n = check_draw_box_tensors(boxes, face_lights, self._device)
        self._check(self._lib.rt_draw_boxes_async(self._h, C.byref(uniforms), _dp(boxes), _dp(face_lights), n))

    # -- particles ---------------------------------------------------------------------------------------
    def draw_particles(self, uniforms, particles, lights):
        """rt_draw_particles: `particles` abi.PARTICLE_DTYPE[N] records (make_particles), each the cube center -+ half lit on all faces by
        `lights`[particle.light] (PROBE_LIGHT_DTYPE[L] records, what probe_records returns), composited by depth into the planes of the
        frame drawn last under the camera of `uniforms`, exactly as draw_boxes composites the derived boxes.  Synchronous; an invalid
        record fails the whole call (RtError, INVALID_ARG)."""
        particles = _records(particles, abi.PARTICLE_DTYPE)
        lights = _records(lights, PROBE_LIGHT_DTYPE)
        self._check(self._lib.rt_draw_particles(self._h, C.byref(uniforms), _ptr_or_none(particles), particles.size, _ptr_or_none(lights), lights.size))

    def draw_particles_async(self, uniforms, particles, lights):
        """rt_draw_particles_async on torch device tensors: `particles` any contiguous tensor of N * 32 bytes (RtParticle rows), `lights`
        any contiguous tensor of L * 16 bytes (e.g. the `out` of probe_light_async).  Enqueued behind the frame drawn last and the
        queries enqueued so far; an invalid record is skipped on the device."""
        n, nlights = particle_tensor_counts(particles, lights, self._device)
        self._check(self._lib.rt_draw_particles_async(self._h, C.byref(uniforms), _dp(particles), n, _dp(lights), nlights))

    # -- particle simulation ------------------------------------------------------------------------------
    def step_particles(self, params, states):
        """rt_step_particles: one tick of `states` (abi.PARTICLE_STATE_DTYPE[N] records, make_particle_states) under `params` (an
        abi.RtParticleStep, make_particle_step) against the resident world -> (states, particles): the next states and the
        abi.PARTICLE_DTYPE[N] draw records, as new arrays.  Synchronous; an active invalid record fails the whole call (RtError,
        INVALID_ARG)."""
        states = _records(states, abi.PARTICLE_STATE_DTYPE)
        out = np.zeros(states.size, dtype=abi.PARTICLE_STATE_DTYPE)
        draw = np.zeros(states.size, dtype=abi.PARTICLE_DTYPE)
        self._check(self._lib.rt_step_particles(self._h, C.byref(params), _ptr_or_none(states), _ptr_or_none(out), _ptr_or_none(draw), states.size))
        return out, draw

    def step_particles_async(self, params, states_in, states_out, draw=None):
        """rt_step_particles_async on torch device tensors: `states_in` and `states_out` any contiguous tensors of N * 64 bytes
        (RtParticleState rows; the same tensor steps in place), `draw` a contiguous tensor of N * 32 bytes (RtParticle rows, what
        draw_particles_async takes) or None.  Enqueued: valid after sync(), or in the order of a stream given to set_stream().
        `states_in` must be complete on the device when the call is made.  An active invalid record gets RT_PSTATE_INVALID."""
        n = particle_step_tensor_count(states_in, states_out, draw, self._device)
        self._check(self._lib.rt_step_particles_async(self._h, C.byref(params), _dp(states_in), _dp(states_out), _dp(draw), n))

    # -- particle emitters --------------------------------------------------------------------------------
    def emit_particles(self, emitters, lr, states, max_emit, cursor):
        """rt_emit_particles: one particle per occupied voxel that `emitters` (abi.EMIT_DTYPE records, make_particle_emitters) select,
        written into the ring `states` (abi.PARTICLE_STATE_DTYPE[capacity]) from the slot `cursor` (an abi.EMIT_CURSOR_DTYPE record,
        an abi.RtEmitCursor or (next, emitted, dropped)) points at, at most `max_emit` of them -> (states, cursor): the ring after the
        call and the cursor as an abi.EMIT_CURSOR_DTYPE record, both new.  Synchronous; an invalid emitter fails the whole call
        (RtError, INVALID_ARG)."""
        emitters = _records(emitters, abi.EMIT_DTYPE)
        ring = _records(states, abi.PARTICLE_STATE_DTYPE).copy()
        cur = emit_cursor(cursor)
        self._check(self._lib.rt_emit_particles(self._h, _ptr_or_none(emitters), emitters.size, _lr3(lr), _ptr_or_none(ring), ring.size,
                                                int(max_emit), _p(cur)))
        return ring, cur[0]

    def emit_particles_async(self, emitters, lr, states_t, max_emit, cursor_t):
        """rt_emit_particles_async on torch device tensors: `states_t` any contiguous tensor of capacity * 64 bytes (RtParticleState
        rows: the ring), `cursor_t` one of 16 bytes (RtEmitCursor); `emitters` host records as for emit_particles.  Enqueued: valid
        after sync(), or in the order of a stream given to set_stream(); a second call chains on the device's cursor."""
        emitters = _records(emitters, abi.EMIT_DTYPE)
        capacity = emit_tensor_capacity(states_t, cursor_t, self._device)
        self._check(self._lib.rt_emit_particles_async(self._h, _ptr_or_none(emitters), emitters.size, _lr3(lr), _dp(states_t), capacity,
                                                      int(max_emit), _dp(cursor_t)))

    # -- particle deposits --------------------------------------------------------------------------------
    def deposit_particles(self, params, states, draw=None, counts=None):
        """rt_deposit_particles: the resting particles of `states` (abi.PARTICLE_STATE_DTYPE[N]) whose centre voxel lies in the box of
        `params` (an abi.RtParticleDeposit, abi.make_particle_deposit) become voxels of the resident world -> (states, draw, counts):
        the states with DEAD set on what was deposited, the abi.PARTICLE_DTYPE[N] draw records with those records' half cleared (None
        when `draw` is None) and the abi.DEPOSIT_COUNT_DTYPE record `counts` (None starts from zeros) added to, all new arrays.
        Synchronous for the arrays; the world change is stream-ordered."""
        states = _records(states, abi.PARTICLE_STATE_DTYPE).copy()
        if draw is not None:
            draw = _records(draw, abi.PARTICLE_DTYPE).copy()
            if draw.size != states.size:
                raise ValueError("draw must hold one record per state")
        cnt = deposit_counts(counts)
        self._check(self._lib.rt_deposit_particles(self._h, C.byref(params), _ptr_or_none(states), None if draw is None else _ptr_or_none(draw),
                                                   states.size, _p(cnt)))
        return states, draw, cnt[0]

    def deposit_particles_async(self, params, states_t, draw_t=None, counts_t=None):
        """rt_deposit_particles_async on torch device tensors: `states_t` any contiguous tensor of N * 64 bytes (RtParticleState rows,
        updated in place), `draw_t` one of N * 32 bytes (RtParticle rows) or None, `counts_t` one of 16 bytes (RtDepositCount, added
        to) or None.  Enqueued behind the steps and queries already enqueued: valid after sync(), or in the order of a stream given
        to set_stream()."""
        n = deposit_tensor_count(states_t, draw_t, counts_t, self._device)
        self._check(self._lib.rt_deposit_particles_async(self._h, C.byref(params), _dp(states_t), _dp(draw_t), n, _dp(counts_t)))

    # -- voxel settling -----------------------------------------------------------------------------------
    def settle_voxels(self, params, counts=None):
        """rt_settle_voxels: the loose voxels in the box of `params` (an abi.RtVoxelSettle, abi.make_voxel_settle) fall along its axis
        -> the abi.SETTLE_COUNT_DTYPE record `counts` (None starts from zeros) added to, a new record.  Synchronous for the counts;
        the world change is stream-ordered."""
        cnt = settle_counts(counts)
        self._check(self._lib.rt_settle_voxels(self._h, C.byref(params), _p(cnt)))
        return cnt[0]

    def settle_voxels_async(self, params, counts_t=None):
        """rt_settle_voxels_async: `counts_t` a contiguous torch device tensor of 16 bytes (RtSettleCount, added to) or None.
        Enqueued: valid after sync(), or in the order of a stream given to set_stream()."""
        if counts_t is not None:
            _device_tensors(self._device, ("counts", counts_t))
            if _nbytes(counts_t) != abi.SETTLE_COUNT_DTYPE.itemsize:
                raise ValueError("counts must be a contiguous tensor of 16 bytes (one RtSettleCount)")
        self._check(self._lib.rt_settle_voxels_async(self._h, C.byref(params), _dp(counts_t)))

    # -- voxel detachment ---------------------------------------------------------------------------------
    def detach_voxels(self, params, result=None):
        """rt_detach_voxels: the occupied voxels in the box of `params` (an abi.RtVoxelDetach, abi.make_voxel_detach) that nothing joins
        to an anchor are counted, with RT_DETACH_CARVE carved and with RT_DETACH_CAPTURE written into a new stamp -> (the
        abi.DETACH_RESULT_DTYPE record `result` added to and merged, a new record; None starts from detach_result(); the stamp's id,
        None without RT_DETACH_CAPTURE, 0 for an empty clipped box).  Synchronous for the result; a world change is stream-ordered."""
        res = detach_result(result)
        out = C.c_uint32(0)
        self._check(self._lib.rt_detach_voxels(self._h, C.byref(params), _p(res), C.byref(out)))
        return res[0], (out.value if params.flags & abi.RT_DETACH_CAPTURE else None)

    def detach_voxels_async(self, params, result_t=None):
        """rt_detach_voxels_async: `result_t` a contiguous torch device tensor of 48 bytes (RtDetachResult, added to and merged) or
        None.  Enqueued: valid after sync(), or in the order of a stream given to set_stream().  Returns the stamp's id (valid at
        once), None without RT_DETACH_CAPTURE."""
        if result_t is not None:
            _device_tensors(self._device, ("result", result_t))
            if _nbytes(result_t) != abi.DETACH_RESULT_DTYPE.itemsize:
                raise ValueError("result must be a contiguous tensor of 48 bytes (one RtDetachResult)")
        out = C.c_uint32(0)
        self._check(self._lib.rt_detach_voxels_async(self._h, C.byref(params), _dp(result_t), C.byref(out)))
        return out.value if params.flags & abi.RT_DETACH_CAPTURE else None

    # -- fluid flow ---------------------------------------------------------------------------------------
    def flow_voxels(self, params, counts=None):
        """rt_flow_voxels: the fluid in the box of `params` (an abi.RtVoxelFlow, abi.make_voxel_flow) spreads, falls and dries for its
        ticks -> the abi.FLOW_COUNT_DTYPE record `counts` (None starts from zeros) added to, a new record; the host stops ticking when
        what the call added to `active` is 0.  Synchronous for the counts; the world change is stream-ordered."""
        cnt = flow_counts(counts)
        self._check(self._lib.rt_flow_voxels(self._h, C.byref(params), _p(cnt)))
        return cnt[0]

    def flow_voxels_async(self, params, counts_t=None):
        """rt_flow_voxels_async: `counts_t` a contiguous torch device tensor of 32 bytes (RtFlowCount, added to) or None.
        Enqueued: valid after sync(), or in the order of a stream given to set_stream()."""
        if counts_t is not None:
            _device_tensors(self._device, ("counts", counts_t))
            if _nbytes(counts_t) != abi.FLOW_COUNT_DTYPE.itemsize:
                raise ValueError("counts must be a contiguous tensor of 32 bytes (one RtFlowCount)")
        self._check(self._lib.rt_flow_voxels_async(self._h, C.byref(params), _dp(counts_t)))

    # -- navigation fields -------------------------------------------------------------------------------
    def nav_create(self, extent):
        """rt_nav_create: a navigation field of `extent` (ex, ey, ez) cells, each 1..256; returns its id."""
        out = C.c_uint32(0)
        self._check(self._lib.rt_nav_create(self._h, _lr3(extent), C.byref(out)))
        return out.value

    def nav_info(self, field):
        """rt_nav_info: (extent (ex, ey, ez), lo of the build enqueued last, whether there was one)."""
        ext, lo, built = (C.c_int32 * 3)(), (C.c_int32 * 3)(), C.c_uint32(0)
        self._check(self._lib.rt_nav_info(self._h, int(field), ext, lo, C.byref(built)))
        return tuple(ext), tuple(lo), bool(built.value)

    def nav_read(self, field):
        """rt_nav_read: (dist u16[ez, ey, ex], move u8[ez, ey, ex]) of the build enqueued last.  Synchronises."""
        ex, ey, ez = self.nav_info(field)[0]
        dist = np.empty((ez, ey, ex), dtype=np.uint16)
        move = np.empty((ez, ey, ex), dtype=np.uint8)
        self._check(self._lib.rt_nav_read(self._h, int(field), _p(dist), _p(move)))
        return dist, move

    def nav_destroy(self, field):
        """rt_nav_destroy: the id is invalid afterwards; waits for the builds and samples already enqueued."""
        self._check(self._lib.rt_nav_destroy(self._h, int(field)))

    def nav_build(self, field, params, goals, result=None):
        """rt_nav_build: walking distances to `goals` (int[N, 3] texels or abi.NAV_GOAL_DTYPE records) over the box of `params` (an
        abi.RtNavBuild, abi.make_nav_build) into `field` -> the abi.NAV_RESULT_DTYPE record `result` added to and merged, a new
        record; None starts from zeros.  Synchronous for the result."""
        goals = abi.make_nav_goals(goals)
        res = np.zeros(1, dtype=abi.NAV_RESULT_DTYPE)
        if result is not None:
            res[0] = np.asarray(result, dtype=abi.NAV_RESULT_DTYPE).reshape(-1)[0]
        self._check(self._lib.rt_nav_build(self._h, int(field), C.byref(params), _ptr_or_none(goals), goals.size, _p(res)))
        return res[0]

    def nav_build_async(self, field, params, goals_t, result_t=None):
        """rt_nav_build_async: `goals_t` a contiguous torch device tensor of N * 16 bytes (RtNavGoal rows) or None for no goal,
        `result_t` one of 32 bytes (RtNavResult, added to and merged) or None.  Enqueued: valid after sync(), or in the order of a
        stream given to set_stream()."""
        named = [(n, t) for n, t in (("goals", goals_t), ("result", result_t)) if t is not None]
        _device_tensors(self._device, *named)
        n = 0 if goals_t is None else record_count("goals", _nbytes(goals_t), abi.NAV_GOAL_DTYPE.itemsize, abi.MAX_NAV_GOALS, "RtNavGoal")
        if result_t is not None and _nbytes(result_t) != abi.NAV_RESULT_DTYPE.itemsize:
            raise ValueError("result must be a contiguous tensor of 32 bytes (one RtNavResult)")
        self._check(self._lib.rt_nav_build_async(self._h, int(field), C.byref(params), _dp(goals_t) if n else None, n, _dp(result_t)))

    def nav_sample(self, field, agents, snap_down=1, snap_up=1):
        """rt_nav_sample: `agents` float[N, 3] foot points (with the two snap ranges) or abi.NAV_AGENT_DTYPE records -> numpy array
        of abi.NAV_STEP_DTYPE (RtNavStep) per agent.  Synchronous."""
        recs = abi.make_nav_agents(agents, snap_down, snap_up)
        steps = np.zeros(recs.size, dtype=abi.NAV_STEP_DTYPE)
        self._check(self._lib.rt_nav_sample(self._h, int(field), _ptr_or_none(recs), recs.size, _ptr_or_none(steps)))
        return steps

    def nav_sample_async(self, field, agents_t, steps_t):
        """rt_nav_sample_async on torch device tensors: `agents_t` any contiguous tensor of N * 16 bytes (RtNavAgent rows), `steps_t`
        any contiguous tensor of N * 32 bytes.  Enqueued: valid after sync(), or in the order of a stream given to set_stream().  A
        record that cannot be read as an agent gets cell (-1, -1, -1)."""
        _device_tensors(self._device, ("agents", agents_t), ("steps", steps_t))
        n = record_count("agents", _nbytes(agents_t), abi.NAV_AGENT_DTYPE.itemsize, abi.MAX_NAV_AGENTS, "RtNavAgent")
        _holds("steps", steps_t, n, abi.NAV_STEP_DTYPE.itemsize)
        self._check(self._lib.rt_nav_sample_async(self._h, int(field), _dp(agents_t), n, _dp(steps_t)))

    # -- voxel-model entities ----------------------------------------------------------------------------
    def draw_stamps(self, uniforms, models, face_lights):
        """rt_draw_stamps: `models` DRAW_STAMP_DTYPE[N] records (make_draw_stamps) and `face_lights` PROBE_LIGHT_DTYPE[6 N] records (what
        probe_records returns for stamp_face_probes(models, extents)), composited by depth into the planes of the frame drawn last under
        the camera of `uniforms`.  Synchronous; an invalid record fails the whole call (RtError, INVALID_ARG)."""
        models = _records(models, DRAW_STAMP_DTYPE)
        lights = _face_lights(face_lights, models.size, "model")
        self._check(self._lib.rt_draw_stamps(self._h, C.byref(uniforms), _ptr_or_none(models), _ptr_or_none(lights), models.size))

    def draw_stamps_async(self, uniforms, models, face_lights):
        """rt_draw_stamps_async: `models` host records as for draw_stamps (free again on return), `face_lights` a torch device tensor:
        any contiguous tensor of 6 N * 16 bytes (e.g. the `out` of probe_light_async).  Enqueued behind the frame drawn last and the
        queries enqueued so far; an invalid record fails the whole call before anything is enqueued."""
        models = _records(models, DRAW_STAMP_DTYPE)
        check_draw_stamp_lights(models.size, face_lights, self._device)
        self._check(self._lib.rt_draw_stamps_async(self._h, C.byref(uniforms), _ptr_or_none(models), _dp(face_lights), models.size))

    # -- entity shadows ----------------------------------------------------------------------------------
    def shadow_entities(self, uniforms, boxes=None, models=None, strength=1.0):
        """rt_shadow_entities: the drawn `boxes` (DRAW_BOX_DTYPE[N]) and `models` (DRAW_STAMP_DTYPE[M]) take the sun's direct term, times
        `strength` in (0, 1], out of the two lighting planes of the frame drawn last where they shade a pixel the world leaves sunlit,
        under the camera, lr and sun angle of `uniforms`.  Synchronous; an invalid record fails the whole call (RtError, INVALID_ARG)."""
        boxes, models = _entity_records(boxes, models)
        self._check(self._lib.rt_shadow_entities(self._h, C.byref(uniforms), _ptr_or_none(boxes), boxes.size, _ptr_or_none(models), models.size,
                                                 float(strength)))

    def shadow_entities_async(self, uniforms, boxes=None, models=None, strength=1.0):
        """rt_shadow_entities_async: `boxes` a torch device tensor, any contiguous tensor of N * 32 bytes (RtDrawBox rows: what
        draw_boxes_async took), or None; `models` host records as for shadow_entities (free again on return).  Enqueued behind the frame
        drawn last; an invalid box is skipped on the device, an invalid model fails the call before anything is enqueued."""
        n = 0 if boxes is None else check_shadow_box_tensor(boxes, self._device)
        models = _records(models, DRAW_STAMP_DTYPE)
        self._check(self._lib.rt_shadow_entities_async(self._h, C.byref(uniforms), _dp(boxes) if n else None, n, _ptr_or_none(models), models.size,
                                                       float(strength)))

    # -- point lights ------------------------------------------------------------------------------------
    def add_lights(self, uniforms, lights):
        """rt_add_lights: `lights` POINT_LIGHT_DTYPE[N] records (make_point_lights) added to the two lighting planes of the frame drawn
        last under the camera and lr of `uniforms`, each through one shadow ray per pixel.  Synchronous; an invalid light fails the whole
        call (RtError, INVALID_ARG)."""
        lights = _records(lights, POINT_LIGHT_DTYPE)
        self._check(self._lib.rt_add_lights(self._h, C.byref(uniforms), _ptr_or_none(lights), lights.size))

    def add_lights_async(self, uniforms, lights):
        """rt_add_lights_async on a torch device tensor: any contiguous tensor of N * 32 bytes (RtPointLight rows).  Enqueued behind the
        frame drawn last; an invalid light is skipped on the device."""
        n = check_point_light_tensors(lights, self._device)
        self._check(self._lib.rt_add_lights_async(self._h, C.byref(uniforms), _dp(lights), n))

    def add_lights_occluded(self, uniforms, lights, boxes=None, models=None):
        """rt_add_lights_occluded: add_lights with the drawn `boxes` (DRAW_BOX_DTYPE[N]) and `models` (DRAW_STAMP_DTYPE[M]) as occluders: a
        light adds nothing at a pixel where an entity lies between the pixel's surface point and the light.  Synchronous; an invalid
        record fails the whole call (RtError, INVALID_ARG).  With no occluder the call is add_lights."""
        lights = _records(lights, POINT_LIGHT_DTYPE)
        boxes, models = _entity_records(boxes, models)
        self._check(self._lib.rt_add_lights_occluded(self._h, C.byref(uniforms), _ptr_or_none(lights), lights.size, _ptr_or_none(boxes), boxes.size,
                                                     _ptr_or_none(models), models.size))

    def add_lights_occluded_async(self, uniforms, lights, boxes=None, models=None):
        """rt_add_lights_occluded_async: `lights` a torch device tensor as for add_lights_async, `boxes` one as for shadow_entities_async
        (or None), `models` host records (free again on return).  Enqueued behind the frame drawn last; an invalid light or box is
        skipped on the device, an invalid model fails the call before anything is enqueued."""
        n = check_point_light_tensors(lights, self._device)
        nb = 0 if boxes is None else check_shadow_box_tensor(boxes, self._device)
        models = _records(models, DRAW_STAMP_DTYPE)
        self._check(self._lib.rt_add_lights_occluded_async(self._h, C.byref(uniforms), _dp(lights), n, _dp(boxes) if nb else None, nb,
                                                           _ptr_or_none(models), models.size))

    # -- frames ------------------------------------------------------------------------------------------
    def draw_frame(self, uniforms):
        self._check(self._lib.rt_draw_frame(self._h, C.byref(uniforms)))

    def sync(self):
        self._check(self._lib.rt_sync(self._h))

    def set_stream(self, stream_ptr):
        self._check(self._lib.rt_set_stream(self._h, C.c_void_p(stream_ptr)))

    def buffer_bytes(self, buffer_id):
        return int(self._lib.rt_buffer_bytes(self._h, int(buffer_id)))

    def device_ptr(self, buffer_id):
        return self._lib.rt_device_ptr(self._h, int(buffer_id))

    def tile_count(self):
        return int(self._lib.rt_tile_count(self._h))

    def tile_capacity(self):
        return int(self._lib.rt_tile_capacity(self._h))

    def readback(self, buffer_id):
        """Returns the plane as numpy: [H,W(,C)] for whole-frame contexts, [capacity*64(,C)] for tile-split ones."""
        dt, ch = BUFFER_FORMATS[buffer_id]
        nbytes = self.buffer_bytes(buffer_id)
        out = np.empty(nbytes // np.dtype(dt).itemsize, dtype=dt)
        self._check(self._lib.rt_readback(self._h, int(buffer_id), _p(out), nbytes))
        if self.cfg is not None and self.cfg.tile_world == 1:
            shape = (self.cfg.height, self.cfg.width) + ((ch,) if ch > 1 else ())
        else:
            shape = (-1,) + ((ch,) if ch > 1 else ())
        return out.reshape(shape)

    def readback_all(self):
        """The nine planes the ray-trace dispatch writes (not the finalize output)."""
        return {BUFFER_NAMES[b]: self.readback(b) for b in range(RT_BUF_FINAL_BGRA8)}

    def untile(self, buffer_id, gathered_dev_ptr, world, frame_dev_ptr):
        self._check(self._lib.rt_untile(self._h, int(buffer_id), C.c_void_p(gathered_dev_ptr), int(world),
                                        C.c_void_p(frame_dev_ptr)))

    def gbuffer_ptr(self):
        return self._lib.rt_gbuffer_ptr(self._h)

    def gbuffer_bytes(self):
        return int(self._lib.rt_gbuffer_bytes(self._h))

    def gbuffer_offset(self, buffer_id):
        """Byte offset of a reference-format plane inside the contiguous G-buffer block."""
        return int(self._lib.rt_gbuffer_offset(self._h, int(buffer_id)))

    def untile_gbuffer(self, gathered_dev_ptr, world, frame_dev_ptrs):
        """Scatter `world` gathered G-buffer blocks into six row-major planes (device pointers, None to skip)."""
        arr = (C.c_void_p * 6)(*[C.c_void_p(p) if p else None for p in frame_dev_ptrs])
        self._check(self._lib.rt_untile_gbuffer(self._h, C.c_void_p(gathered_dev_ptr), int(world), arr))

    # -- multi-GPU frame assembly (rt_gather_gbuffer) ------------------------------------------------------
    def comm_init_rank(self, unique_id):
        """ncclCommInitRank(tile_world, unique_id, tile_rank) on this context's device; returns the communicator handle."""
        comm = C.c_void_p()
        buf = (C.c_char * len(unique_id)).from_buffer_copy(bytes(unique_id))
        self._check(self._lib.rt_comm_init_rank(self._h, buf, len(unique_id), C.byref(comm)))
        return comm.value

    def gather_gbuffer(self, comm, root, frame_dev_ptrs=None, overlapped=False):
        """Every rank's six reference-format planes -> `root` over RCCL on the context's stream, un-tiled there into the six
        row-major device planes frame_dev_ptrs (root only)."""
        arr = (C.c_void_p * 6)(*[C.c_void_p(p) if p else None for p in frame_dev_ptrs]) if frame_dev_ptrs else None
        self._check(self._lib.rt_gather_gbuffer(self._h, C.c_void_p(comm) if comm else None, int(root), arr, 1 if overlapped else 0))

    def selftest(self, which=1):
        """rt_selftest: RT_SELFTEST_DENOISE_DIVISION (1) -> number of inexact quotients over the denoise division's domain;
        RT_SELFTEST_SCENE_MAPS (2) -> number of nibble-map words that differ from a rebuild from the resident minefield."""
        out = C.c_uint64(0)
        self._check(self._lib.rt_selftest(self._h, int(which), C.byref(out)))
        return int(out.value)

    def frame_ptr(self, buffer_id):
        return self._lib.rt_frame_ptr(self._h, int(buffer_id))

    def frame_readback(self, buffer_id):
        """Plane `buffer_id` of the frame rt_gather_gbuffer assembled in the library's own planes (frames_dev = NULL)."""
        dt, ch = BUFFER_FORMATS[buffer_id]
        W, H = self.cfg.width, self.cfg.height
        out = np.empty((H, W, ch) if ch > 1 else (H, W), dtype=dt)
        self._check(self._lib.rt_frame_readback(self._h, int(buffer_id), _p(out), out.nbytes))
        return out

    # -- post passes (pipeline.rs:98-123) ----------------------------------------------------------------
    def denoise(self, faithful=True):
        self._check(self._lib.rt_denoise(self._h, 1 if faithful else 0))

    def finalize(self):
        self._check(self._lib.rt_finalize(self._h))

    def denoise_planes(self, lighting_ptr, depth_ptr, normal_ptr, faithful=True):
        """The six denoise dispatches on caller-owned row-major device planes (e.g. the gathered frame on rank 0)."""
        self._check(self._lib.rt_denoise_planes(self._h, C.c_void_p(lighting_ptr), C.c_void_p(depth_ptr), C.c_void_p(normal_ptr),
                                                1 if faithful else 0))

    def denoise_history(self, params=None, faithful=True):
        """rt_denoise_history: the six denoise dispatches on the frame drawn last of an RT_FLAG_REPROJECT context, with its per-pixel
        sample counts.  `params`: an RtDenoiseParams (denoise_params); None = HISTORY_DENOISE_PRESET with `faithful`."""
        if params is None:
            params = denoise_params(faithful=faithful, **HISTORY_DENOISE_PRESET)
        self._check(self._lib.rt_denoise_history(self._h, C.byref(params)))

    def denoise_planes_counted(self, lighting_ptr, depth_ptr, normal_ptr, counts_ptr, params):
        """rt_denoise_planes_counted: the same on caller-owned row-major device planes and a u32[H, W] device plane of counts."""
        self._check(self._lib.rt_denoise_planes_counted(self._h, C.c_void_p(lighting_ptr), C.c_void_p(depth_ptr), C.c_void_p(normal_ptr),
                                                        C.c_void_p(counts_ptr), C.byref(params)))

    def finalize_planes(self, albedo_ptr, emission_ptr, fog_ptr, lighting_ptr, depth_ptr, out_ptr):
        self._check(self._lib.rt_finalize_planes(self._h, C.c_void_p(albedo_ptr), C.c_void_p(emission_ptr), C.c_void_p(fog_ptr),
                                                 C.c_void_p(lighting_ptr), C.c_void_p(depth_ptr), C.c_void_p(out_ptr)))

    # -- instrumentation ---------------------------------------------------------------------------------
    def kernel_in_use(self):
        """RtKernel the context runs (what RT_KERNEL_DEFAULT resolved to)."""
        return int(self._lib.rt_kernel_in_use(self._h))

    def counters(self):
        cn = RtCounters()
        self._check(self._lib.rt_get_counters(self._h, C.byref(cn)))
        return cn

    def reset_counters(self):
        self._check(self._lib.rt_reset_counters(self._h))

    def reset_accumulation(self):
        """rt_reset_accumulation: the next frame of an RT_FLAG_ACCUMULATE context starts its running sum from zero."""
        self._check(self._lib.rt_reset_accumulation(self._h))

    def accumulation(self):
        """rt_get_accumulation: (frames, samples) the lighting planes of the frame drawn last hold (host-side state, no wait)."""
        frames, samples = C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.rt_get_accumulation(self._h, C.byref(frames), C.byref(samples)))
        return int(frames.value), int(samples.value)

    def read_history(self):
        """rt_read_history: uint32[H, W] per-pixel sample counts behind the lighting of the frame drawn last (RT_FLAG_REPROJECT
        contexts; row 0 = bottom).  Synchronises."""
        out = np.empty((self.cfg.height, self.cfg.width), dtype=np.uint32)
        self._check(self._lib.rt_read_history(self._h, _p(out), out.nbytes))
        return out

    def edit_boxes_pending(self):
        """rt_edit_boxes_pending: (boxes, overflowed) — the edited boxes that wait for the next frame of a context with
        edit_radius > 0, and whether the set overflowed so that the frame restarts (host-side state, no wait)."""
        boxes, over = C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.rt_edit_boxes_pending(self._h, C.byref(boxes), C.byref(over)))
        return int(boxes.value), bool(over.value)

    def slabs_pending(self):
        """rt_slabs_pending: (slabs, overflowed) — the slabs that wait for the next frame of a context with stream_history = 1, and
        whether the set overflowed so that the frame restarts (host-side state, no wait)."""
        slabs, over = C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.rt_slabs_pending(self._h, C.byref(slabs), C.byref(over)))
        return int(slabs.value), bool(over.value)

    def read_slab_boxes(self):
        """rt_read_slab_boxes: float32 [count, 2, 3] — (lo, hi) of the world boxes the pending slabs of the frame drawn last
        produced, in order; count = 0 when that frame had none or restarted.  Waits for the frame."""
        out = np.zeros((8, 2, 3), dtype=np.float32)
        n = C.c_uint32(0)
        self._check(self._lib.rt_read_slab_boxes(self._h, _p(out), C.byref(n)))
        return out[:int(n.value)].copy()

    def info(self):
        i = RtInfo()
        i.struct_size = C.sizeof(RtInfo)
        self._check(self._lib.rt_get_info(self._h, C.byref(i)))
        return i

    def timing(self):
        t = RtTiming()
        self._check(self._lib.rt_get_timing(self._h, C.byref(t)))
        return t

    def gather_timing(self):
        """rt_get_gather_timing: (sum of the rt_gather_gbuffer calls' device time in ms, number of calls) since the last call —
        events round the transfer + un-tile on the stream they run on; contexts with RT_FLAG_TIMING only (else (0.0, 0))."""
        ms, n = C.c_float(0.0), C.c_uint32(0)
        self._check(self._lib.rt_get_gather_timing(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)


# ---- host mirror of the reference API ------------------------------------------------------------------------

def compute_triple_euler_vector(heading, pitch):
    """src/util.rs:9-22 (C++ mirror). Returns (forward, up, right) as float32 arrays."""
    f = (C.c_float * 3)()
    u = (C.c_float * 3)()
    r = (C.c_float * 3)()
    _lib.host().rth_compute_triple_euler_vector(float(heading), float(pitch), f, u, r)
    return (np.array(f[:], dtype=np.float32), np.array(u[:], dtype=np.float32), np.array(r[:], dtype=np.float32))


class Camera:
    """render::Camera (src/render/mod.rs:20-34): view of the native Game's camera."""

    def __init__(self, game):
        self._game = game

    def _get(self):
        o = (C.c_float * 3)()
        h = C.c_float()
        p = C.c_float()
        _lib.host().rth_game_get_camera(self._game._h, o, C.byref(h), C.byref(p))
        return [o[0], o[1], o[2]], h.value, p.value

    @property
    def origin(self):
        return tuple(self._get()[0])

    @property
    def heading(self):
        return self._get()[1]

    @property
    def pitch(self):
        return self._get()[2]

    def set(self, origin=None, heading=None, pitch=None):
        o, h, p = self._get()
        if origin is not None:
            o = list(origin)
        if heading is not None:
            h = heading
        if pitch is not None:
            p = pitch
        _lib.host().rth_game_set_camera(self._game._h, (C.c_float * 3)(*o), float(h), float(p))


class Game:
    """game::Game (src/game/mod.rs:14-58): camera + sun angle + world.  `args` are the reference's six optional
    positional CLI floats `x y z heading pitch sun_angle` (mod.rs:45-52)."""

    def __init__(self, args=()):
        argv = [b"raytrace"] + [str(a).encode() for a in args]
        arr = (C.c_char_p * len(argv))(*argv)
        self._h = C.c_void_p(_lib.host().rth_game_new(len(argv), arr))
        if not self._h:
            raise MemoryError("Game")
        self.camera = Camera(self)

    def borrow_camera(self):
        return self.camera

    def get_sun_angle(self):
        return float(_lib.host().rth_game_get_sun_angle(self._h))

    def set_sun_angle(self, a):
        _lib.host().rth_game_set_sun_angle(self._h, float(a))

    @staticmethod
    def _check_region(rc, call):
        if rc != 0:
            raise RtError(rc, "%s: region must be 256, 512 or 1024" % call)

    def set_world(self, materials, minefield, region=256):
        materials, minefield = _records(materials, np.uint32), _records(minefield, np.uint8)
        if materials.size != region ** 3 or minefield.size != region ** 3:
            raise ValueError("world arrays must hold region^3 voxels")
        self._check_region(_lib.host().rth_game_set_world_r(self._h, _p(materials), _p(minefield), int(region)), "set_world")

    def generate_world(self, seed=0x5EED, region=256):
        self._check_region(_lib.host().rth_game_generate_world_r(self._h, C.c_uint64(int(seed)), int(region)), "generate_world")

    def use_device_world(self, seed=0x5EED, region=256):
        """The world of generate_world(seed, region) without its host bytes: create_instance generates it on the device
        (rt_generate_world) instead of uploading it."""
        self._check_region(_lib.host().rth_game_use_device_world(self._h, C.c_uint64(int(seed)), int(region)), "use_device_world")

    def close(self):
        if self._h:
            _lib.host().rth_game_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pipeline:
    """render::Pipeline (src/render/pipeline/pipeline.rs).  Create with `create_instance`."""

    def __init__(self, handle, cfg):
        self._h = C.c_void_p(handle)
        self.cfg = cfg
        self.context = Context(cfg=cfg, handle=_lib.host().rth_pipeline_context(self._h), owned=False)

    def _check(self, rc, message=None):
        """RtError for a failed call: with `message`, or with the pipeline's own last error."""
        if rc != 0:
            raise RtError(rc, message or _lib.host().rth_pipeline_last_error(self._h).decode())

    def draw_frame(self, game):
        """pipeline.rs:134-255: derive uniforms from the camera, submit the ray-trace work (asynchronous)."""
        self._check(_lib.host().rth_pipeline_draw_frame(self._h, game._h))

    def wait(self):
        self._check(_lib.host().rth_pipeline_wait(self._h))

    def uniforms(self):
        u = RtUniforms()
        _lib.host().rth_pipeline_uniforms(self._h, C.byref(u))
        return u

    def set_seed(self, seed):
        _lib.host().rth_pipeline_set_seed(self._h, C.c_uint32(int(seed)))

    def enable_terrain_streaming(self, seed=0x5EED, storage_dir="", on_device=False):
        """pipeline.rs:174-189: every draw_frame moves the TerrainUploadManager towards the camera (<= 1 slab per frame).
        on_device: the slabs are generated on the device (rt_generate_slice) instead of assembled from host chunks and uploaded."""
        if on_device:
            _lib.host().rth_pipeline_enable_streaming_on_device(self._h, C.c_uint64(int(seed)))
        else:
            _lib.host().rth_pipeline_enable_streaming(self._h, C.c_uint64(int(seed)), str(storage_dir).encode() if storage_dir else None)

    def enable_post_passes(self, faithful=True):
        """pipeline.rs:98-123: every draw_frame then enqueues ray trace -> six denoise dispatches -> finalize (the reference's one
        command buffer, :229-235); RT_BUF_FINAL_BGRA8 holds the frame's swapchain image.  Whole-frame contexts only."""
        self._check(_lib.host().rth_pipeline_enable_post_passes(self._h, 1 if faithful else 0),
                    "enable_post_passes: whole-frame contexts only (tile_world == 1)")

    def enable_history_denoise(self, params=None, faithful=True):
        """With enable_post_passes on an RT_FLAG_REPROJECT context: draw_frame enqueues rt_denoise_history(params) in place of
        rt_denoise.  `params` as Context.denoise_history.  RT_ERR_INVALID_ARG on a context that does not reproject or for a bad
        block."""
        if params is None:
            params = denoise_params(faithful=faithful, **HISTORY_DENOISE_PRESET)
        self._check(_lib.host().rth_pipeline_enable_history_denoise(self._h, C.byref(params)),
                    "enable_history_denoise: needs an RT_FLAG_REPROJECT context and a valid RtDenoiseParams")

    def pick(self, game, x, y_from_top):
        """The block under screen pixel (x, y_from_top) of the frame drawn last for `game` (Pipeline::pick: the pipeline's current
        uniforms, the `lr` terrain streaming moved included).  Returns a dict: `hit` (HIT_DTYPE record), `texel`, `normal`, `kind`,
        `adjacent` (the texel in front of the face, where a placed block goes) and `world` (the hit texel's world coordinate)."""
        del game   # the pick is of the frame the pipeline drew for it: its uniforms hold the camera
        hit = np.zeros(1, dtype=HIT_DTYPE)
        adj, wld = (C.c_int32 * 3)(), (C.c_int32 * 3)()
        self._check(_lib.host().rth_pipeline_pick(self._h, int(x), int(y_from_top), _p(hit), adj, wld))
        return _pick_result(hit, adj, wld)

    def pick_entity(self, x, y_from_top):
        """Pipeline::pick_entity: the entity under screen pixel (x, y_from_top) among the boxes and models of set_boxes / set_models,
        under the uniforms of the frame drawn last.  Returns a dict: `entity` (ENTITY_HIT_DTYPE record; kind != RT_ENTITY_NONE means
        the cursor is on an entity) and the world's `hit`, `texel`, `normal`, `kind`, `adjacent` and `world` as pick gives them."""
        ent = np.zeros(1, dtype=ENTITY_HIT_DTYPE)
        hit = np.zeros(1, dtype=HIT_DTYPE)
        adj, wld = (C.c_int32 * 3)(), (C.c_int32 * 3)()
        self._check(_lib.host().rth_pipeline_pick_entity(self._h, int(x), int(y_from_top), _p(ent), _p(hit), adj, wld))
        return _pick_result(hit, adj, wld, entity=ent[0])

    def set_boxes(self, boxes=None, face_lights=None):
        """Pipeline::set_boxes: every draw_frame from now on enqueues rt_draw_boxes for this set between the ray trace and the denoise
        (DRAW_BOX_DTYPE[N] and PROBE_LIGHT_DTYPE[6 N], copied); None or an empty set draws none."""
        boxes = _records(boxes, DRAW_BOX_DTYPE)
        lights = _face_lights(face_lights, boxes.size, "box")
        self._check(_lib.host().rth_pipeline_set_boxes(self._h, _ptr_or_none(boxes), _ptr_or_none(lights), boxes.size),
                    "set_boxes: at most %d boxes" % MAX_DRAW_BOXES)

    def set_models(self, models=None, face_lights=None):
        """Pipeline::set_models: every draw_frame from now on enqueues rt_draw_stamps for this set between the ray trace and the denoise,
        after the entity boxes (DRAW_STAMP_DTYPE[N] and PROBE_LIGHT_DTYPE[6 N], copied); None or an empty set draws none.  The stamps
        are the pipeline's (stamp_create / stamp_capture) and must be live at every draw."""
        models = _records(models, DRAW_STAMP_DTYPE)
        lights = _face_lights(face_lights, models.size, "model")
        self._check(_lib.host().rth_pipeline_set_models(self._h, _ptr_or_none(models), _ptr_or_none(lights), models.size),
                    "set_models: at most %d models" % MAX_DRAW_STAMPS)

    def set_lights(self, lights=None):
        """Pipeline::set_lights: every draw_frame from now on enqueues rt_add_lights for this set behind the ray trace and the entity
        boxes and in front of the denoise (POINT_LIGHT_DTYPE[N], copied); None or an empty set adds none."""
        lights = _records(lights, POINT_LIGHT_DTYPE)
        self._check(_lib.host().rth_pipeline_set_lights(self._h, _ptr_or_none(lights), lights.size), "set_lights: at most %d lights" % MAX_POINT_LIGHTS)

    def enable_entity_shadows(self, strength=1.0):
        """Pipeline::enable_entity_shadows: every draw_frame from now on enqueues rt_shadow_entities for the boxes and models set
        (set_boxes, set_models) behind their draws and in front of the point lights; strength in (0, 1], 0 switches it off again."""
        self._check(_lib.host().rth_pipeline_enable_entity_shadows(self._h, float(strength)),
                    "enable_entity_shadows: strength must be 0 (off) or lie in (0, 1]")

    def detach_voxels(self, params, result=None):
        """rt_detach_voxels on the pipeline's context (Context.detach_voxels): what the carve before it left unsupported in the box of
        `params` is carved and captured.  Returns the stamp's id when `params` captures — ready for set_models —, else the result
        record; with `result` given (an abi.DETACH_RESULT_DTYPE record) it is added to and merged in place."""
        res, stamp = self.context.detach_voxels(params, result)
        if isinstance(result, np.ndarray) and result.dtype == abi.DETACH_RESULT_DTYPE:
            result.reshape(-1)[0] = res
        return stamp if params.flags & abi.RT_DETACH_CAPTURE else res

    def enable_light_shadows(self, on=True):
        """Pipeline::enable_light_shadows: every draw_frame from now on hands the boxes and models set (set_boxes, set_models) to the
        lights step, which runs rt_add_lights_occluded in rt_add_lights' place: the entities cast shadows in the point lights."""
        self._check(_lib.host().rth_pipeline_enable_light_shadows(self._h, 1 if on else 0), "enable_light_shadows")

    def close(self):
        if self._h:
            _lib.host().rth_pipeline_free(self._h)   # impl Drop for Pipeline, pipeline.rs:258-277
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def create_instance(cfg, game, blue_noise_rgba8):
    """render::create_instance (src/render/mod.rs:36-43): builds the pipeline, uploads the game's world
    (generating the procedural one if the game has none) and the blue-noise table."""
    noise = _records(blue_noise_rgba8, np.uint8)
    if noise.size != 512 * 512 * 4:
        raise ValueError("noise must be 512x512 RGBA8")
    err = C.create_string_buffer(512)
    h = _lib.host().rth_create_instance(C.byref(cfg), _p(noise), game._h, err, 512)
    if not h:
        raise RtError(-1, err.value.decode())
    return Pipeline(h, cfg)


def camera_uniforms(origin, heading, pitch, sun_angle=0.0, seed=1, lr=(0, 0, 0)):
    """The uniform fill of Pipeline::draw_frame (pipeline.rs:191-207) as a standalone helper (product-side;
    the oracle has its own restatement)."""
    fwd, up, right = compute_triple_euler_vector(heading, pitch)
    u = RtUniforms()
    u.sun_angle = float(sun_angle)
    u.seed = int(seed)
    for a in range(3):
        u.origin[a] = float(origin[a])
        u.forward[a] = float(fwd[a])
        u.up[a] = float(np.float32(up[a]) * np.float32(0.4))
        u.right[a] = float(np.float32(right[a]) * np.float32(0.4))
        u.lr[a] = int(lr[a])
        u.lso[a] = int(lr[a])
    return u


DEFAULT_POSE = dict(origin=(-30.0, -128.0, 100.0), heading=math.pi / 2, pitch=0.0, sun_angle=0.0)  # game/mod.rs:53-55


# ---- device arguments of the *_async calls ------------------------------------------------------------------------
# A host address handed to a kernel faults the device, so every torch tensor an *_async call takes goes through _device_tensors and
# its size through record_count / _holds first.  Only host-side attributes of the tensors are read: no sync, no device work.

def record_count(name, nbytes, itemsize, cap=None, record=""):
    """N, where argument `name` holds `nbytes` bytes of `itemsize`-byte records (`record`: the struct's name, for the message).
    Pure integers.  ValueError for a partial record and for N above `cap`."""
    if nbytes % itemsize:
        raise ValueError("%s must hold whole %d-byte %srecords" % (name, itemsize, record and record + " "))
    n = nbytes // itemsize
    if cap is not None and n > cap:
        raise ValueError("at most %d %s per call" % (cap, name))
    return n


def _device_tensors(device, *named):
    """ValueError unless every (name, tensor) of `named` is a torch tensor — asked of all of them first — on GPU `device`, 16-byte
    aligned and contiguous: what a kernel may be given the address of."""
    import torch
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be a torch tensor" % name)
    for name, t in named:
        if not t.is_cuda or t.device.index != int(device):
            raise ValueError("%s must be a tensor on cuda:%d (the context's device), not %s" % (name, int(device), t.device))
        if t.data_ptr() % 16:
            raise ValueError("%s must be 16-byte aligned" % name)
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)


def _nbytes(t):
    return t.numel() * t.element_size()


def _holds(name, t, n, itemsize, per=1):
    """ValueError unless tensor `t` is exactly `per` records of `itemsize` bytes for each of the call's `n`."""
    if _nbytes(t) != per * n * itemsize:
        raise ValueError("%s must be a contiguous tensor of %sN * %d bytes" % (name, "%d " % per if per > 1 else "", itemsize))


def _ray_count(rays, cap=None):
    """N of a checked device tensor of RtRay rows, which the queries take as float32[N, 8] only."""
    import torch
    if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8:
        raise ValueError("rays must be a contiguous float32 tensor of shape [N, 8]")
    return record_count("rays", _nbytes(rays), 32, cap)


def _box_count(boxes):
    """N of a checked device tensor of RtDrawBox rows."""
    return record_count("boxes", _nbytes(boxes), DRAW_BOX_DTYPE.itemsize, MAX_DRAW_BOXES, "RtDrawBox")


def check_query_tensors(rays, hits, device):
    """Context.trace_rays_async's arguments: `rays` a contiguous float32[N, 8] tensor and `hits` a contiguous tensor of N * 48
    bytes, both on GPU `device` and 16-byte aligned.  Returns N; raises ValueError otherwise (a host tensor's address handed to the
    kernel would fault the device)."""
    _device_tensors(device, ("rays", rays), ("hits", hits))
    n = _ray_count(rays)
    _holds("hits", hits, n, HIT_DTYPE.itemsize)
    return n


def check_entity_query_tensors(rays, boxes, world_hits, entity_hits, device):
    """Context.trace_entities_async's device arguments: `rays` a contiguous float32[N, 8] tensor, `boxes` a contiguous tensor of B * 32
    bytes or None, `world_hits` a contiguous tensor of N * 48 bytes or None, `entity_hits` a contiguous tensor of N * 48 bytes, all on
    GPU `device` and 16-byte aligned, N at most 2^24 and B at most 4096.  Returns (N, B); raises ValueError otherwise (a host tensor's
    address handed to the kernel would fault the device)."""
    optional = [(name, t) for name, t in (("boxes", boxes), ("world_hits", world_hits)) if t is not None]
    _device_tensors(device, ("rays", rays), ("entity_hits", entity_hits), *optional)
    n = _ray_count(rays, MAX_ENTITY_RAYS)
    if world_hits is not None:
        _holds("world_hits", world_hits, n, HIT_DTYPE.itemsize)
    _holds("entity_hits", entity_hits, n, ENTITY_HIT_DTYPE.itemsize)
    return n, 0 if boxes is None else _box_count(boxes)


def make_sweeps(sweeps):
    """RtBoxSweep records (SWEEP_DTYPE) from float[N, 3, 3] rows of (lo, hi, motion); ready records pass through."""
    if isinstance(sweeps, np.ndarray) and sweeps.dtype == SWEEP_DTYPE:
        return np.ascontiguousarray(sweeps).reshape(-1)
    a = np.asarray(sweeps, dtype=np.float32)
    if a.size % 9:
        raise ValueError("sweeps must hold rows of lo[3], hi[3], motion[3]")
    a = a.reshape(-1, 3, 3)
    recs = np.zeros(a.shape[0], dtype=SWEEP_DTYPE)
    recs["lo"], recs["hi"], recs["motion"] = a[:, 0], a[:, 1], a[:, 2]
    return recs


def check_sweep_tensors(sweeps, hits, device):
    """Context.sweep_boxes_async's arguments: contiguous tensors of N * 48 and N * 64 bytes on GPU `device`, 16-byte aligned.
    Returns N; raises ValueError otherwise (a host tensor's address handed to the kernel would fault the device)."""
    _device_tensors(device, ("sweeps", sweeps), ("hits", hits))
    n = record_count("sweeps", _nbytes(sweeps), SWEEP_DTYPE.itemsize, None, "RtBoxSweep")
    _holds("hits", hits, n, SWEEP_HIT_DTYPE.itemsize)
    return n


def entity_sweep_tensor_counts(sweeps, boxes, world_hits, entity_hits, device):
    """Context.sweep_entities_async's device arguments: `sweeps` a contiguous tensor of N * 48 bytes, `boxes` a contiguous tensor of
    B * 32 bytes or None, `world_hits` a contiguous tensor of N * 64 bytes or None, `entity_hits` a contiguous tensor of N * 80 bytes,
    all on GPU `device` and 16-byte aligned, N at most 2^24 and B at most 4096.  Returns (N, B); raises ValueError otherwise (a host
    tensor's address handed to the kernel would fault the device)."""
    optional = [(name, t) for name, t in (("boxes", boxes), ("world_hits", world_hits)) if t is not None]
    _device_tensors(device, ("sweeps", sweeps), ("entity_hits", entity_hits), *optional)
    n = record_count("sweeps", _nbytes(sweeps), SWEEP_DTYPE.itemsize, MAX_ENTITY_SWEEPS, "RtBoxSweep")
    if world_hits is not None:
        _holds("world_hits", world_hits, n, SWEEP_HIT_DTYPE.itemsize)
    _holds("entity_hits", entity_hits, n, abi.ENTITY_SWEEP_HIT_DTYPE.itemsize)
    return n, 0 if boxes is None else _box_count(boxes)


def make_draw_boxes(lo, hi, materials, emissions=0xFF000000):
    """RtDrawBox records (DRAW_BOX_DTYPE) from float[N, 3] corners, u32[N] packed material words and u32[N] RGBA8 emission words (one
    value serves every box; a voxel's emission is 0xFF000000).  Refuses what rt_draw_boxes refuses: a non-finite float, a coordinate
    beyond 2^22, lo >= hi on an axis, more than 4096 boxes."""
    lo = np.asarray(lo, dtype=np.float32).reshape(-1, 3)
    hi = np.asarray(hi, dtype=np.float32).reshape(-1, 3)
    if lo.shape != hi.shape:
        raise ValueError("lo and hi must have the same shape [N, 3]")
    n = lo.shape[0]
    if n > MAX_DRAW_BOXES:
        raise ValueError("at most %d boxes per call" % MAX_DRAW_BOXES)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("box corners must be finite")
    if n and (np.abs(lo).max() > 2.0 ** 22 or np.abs(hi).max() > 2.0 ** 22):
        raise ValueError("box corners must lie within +-2^22")
    if not (lo < hi).all():
        raise ValueError("lo must be below hi on every axis")
    boxes = np.zeros(n, dtype=DRAW_BOX_DTYPE)
    boxes["lo"], boxes["hi"] = lo, hi
    boxes["material"] = np.broadcast_to(np.asarray(materials, dtype=np.uint32), (n,))
    boxes["emission"] = np.broadcast_to(np.asarray(emissions, dtype=np.uint32), (n,))
    return boxes


def face_probes(boxes, cells=(0, 0)):
    """The six RtLightProbe records (PROBE_DTYPE) per box that light its faces: record 6 b + n sits at the centre of box b's face with
    normal code n, moved 0.001 off the face along its normal, with normal n.  `cells`: int[N, 2] noise cells per box, or one pair for
    all.  probe_records(u, face_probes(boxes), samples, depth) is the face_lights of draw_boxes."""
    boxes = _records(boxes, DRAW_BOX_DTYPE)
    n = boxes.size
    lo, hi = boxes["lo"].astype(np.float32), boxes["hi"].astype(np.float32)
    centre = (lo + hi) * np.float32(0.5)
    pos = np.repeat(centre[:, None, :], 6, axis=1)
    for code in range(6):
        axis = code // 2
        # a ray travelling towards -axis (even code) crosses the high face, one towards +axis the low face
        pos[:, code, axis] = hi[:, axis] + np.float32(0.001) if code % 2 == 0 else lo[:, axis] - np.float32(0.001)
    cell = np.broadcast_to(np.asarray(cells).reshape(-1, 2), (n, 2))
    return make_probes(pos.reshape(-1, 3), np.tile(np.arange(6), n), np.repeat(cell, 6, axis=0))


def check_draw_box_tensors(boxes, face_lights, device):
    """Context.draw_boxes_async's arguments: contiguous tensors of N * 32 and 6 N * 16 bytes on GPU `device`, 16-byte aligned, N at most
    4096.  Returns N; raises ValueError otherwise (a host tensor's address handed to the kernel would fault the device)."""
    _device_tensors(device, ("boxes", boxes), ("face_lights", face_lights))
    n = _box_count(boxes)
    _holds("face_lights", face_lights, n, PROBE_LIGHT_DTYPE.itemsize, per=6)
    return n


def make_particles(centers, halves, materials, lights=0, emissions=0xFF000000):
    """RtParticle records (abi.PARTICLE_DTYPE) from float[N, 3] centres, float[N] half edges, u32[N] packed material words, u32[N] light
    indices and u32[N] RGBA8 emission words (one value serves every particle).  The records are not judged here: what is valid
    depends on the call's light count (rt_draw_particles refuses an invalid record, the asynchronous call skips it)."""
    c = np.asarray(centers, dtype=np.float32).reshape(-1, 3)
    n = c.shape[0]
    if n > MAX_PARTICLES:
        raise ValueError("at most %d particles per call" % MAX_PARTICLES)
    p = np.zeros(n, dtype=abi.PARTICLE_DTYPE)
    p["center"] = c
    p["half"] = np.broadcast_to(np.asarray(halves, dtype=np.float32), (n,))
    p["material"] = np.broadcast_to(np.asarray(materials, dtype=np.uint32), (n,))
    p["light"] = np.broadcast_to(np.asarray(lights, dtype=np.uint32), (n,))
    p["emission"] = np.broadcast_to(np.asarray(emissions, dtype=np.uint32), (n,))
    return p


def particle_tensor_counts(particles, lights, device):
    """Context.draw_particles_async's arguments: contiguous tensors of N * 32 and L * 16 bytes on GPU `device`, 16-byte aligned, N and L
    at most 2^20.  Returns (N, L); raises ValueError otherwise (a host tensor's address handed to the kernel would fault the device)."""
    _device_tensors(device, ("particles", particles), ("lights", lights))
    n = record_count("particles", _nbytes(particles), abi.PARTICLE_DTYPE.itemsize, MAX_PARTICLES, "RtParticle")
    return n, record_count("lights", _nbytes(lights), PROBE_LIGHT_DTYPE.itemsize, MAX_PARTICLE_LIGHTS, "RtProbeLight")


def make_particle_states(lo, hi, velocities=0.0, halves=None, responses=abi.RT_PARTICLE_DIE, lives=np.inf, materials=0, lights=0,
                         emissions=0xFF000000):
    """RtParticleState records (abi.PARTICLE_STATE_DTYPE) from float[N, 3] corners of the swept boxes, float[N, 3] velocities, float[N]
    half edges of the drawn cubes (None: half the box's x extent), RT_PARTICLE_* responses, float[N] seconds of life, u32[N] packed
    material words, light indices and RGBA8 emission words (one value serves every particle).  The records are not judged here:
    rt_step_particles refuses an invalid record, the asynchronous call marks it RT_PSTATE_INVALID."""
    lo = np.asarray(lo, dtype=np.float32).reshape(-1, 3)
    hi = np.asarray(hi, dtype=np.float32).reshape(-1, 3)
    if lo.shape != hi.shape:
        raise ValueError("lo and hi must have the same shape [N, 3]")
    n = lo.shape[0]
    if n > MAX_PARTICLES:
        raise ValueError("at most %d particles per call" % MAX_PARTICLES)
    s = np.zeros(n, dtype=abi.PARTICLE_STATE_DTYPE)
    s["lo"], s["hi"] = lo, hi
    s["velocity"] = np.broadcast_to(np.asarray(velocities, dtype=np.float32), (n, 3))
    s["half"] = (hi[:, 0] - lo[:, 0]) * np.float32(0.5) if halves is None else np.broadcast_to(np.asarray(halves, dtype=np.float32), (n,))
    s["flags"] = np.broadcast_to(np.asarray(responses, dtype=np.uint32), (n,)) & np.uint32(abi.RT_PSTATE_RESPONSE)
    s["life"] = np.broadcast_to(np.asarray(lives, dtype=np.float32), (n,))
    s["material"] = np.broadcast_to(np.asarray(materials, dtype=np.uint32), (n,))
    s["light"] = np.broadcast_to(np.asarray(lights, dtype=np.uint32), (n,))
    s["emission"] = np.broadcast_to(np.asarray(emissions, dtype=np.uint32), (n,))
    return s


def make_particle_step(dt, accel=(0.0, 0.0, 0.0), damping=1.0, restitution=0.5, friction=1.0, rest_speed=0.0, lr=(0, 0, 0), sweeps=3):
    """An abi.RtParticleStep: `dt` seconds, `accel` (gravity, wind), the velocity's `damping` per tick, a bounce's `restitution` on the
    blocked axis and `friction` on the other two, the speed below which a bounce comes to rest, the window `lr` and the sub-sweeps per
    tick.  Refuses what the calls refuse: a non-finite float, dt outside (0, 1], |accel| above 4096, a factor outside [0, 1], a
    negative rest_speed, sweeps outside 1..4."""
    p = abi.RtParticleStep()
    p.dt, p.damping, p.restitution, p.friction, p.rest_speed = float(dt), float(damping), float(restitution), float(friction), float(rest_speed)
    accel = [float(v) for v in accel]
    if len(accel) != 3 or len(lr) != 3:
        raise ValueError("accel and lr have three components")
    for k in range(3):
        p.accel[k], p.lr[k] = accel[k], int(lr[k])
    if not all(math.isfinite(v) for v in [p.dt, p.damping, p.restitution, p.friction, p.rest_speed] + accel):
        raise ValueError("every parameter must be finite")
    if not 0.0 < p.dt <= 1.0:
        raise ValueError("dt must be in (0, 1]")
    if max(abs(v) for v in accel) > 4096.0:
        raise ValueError("accel must lie within +-4096")
    if not (0.0 <= p.damping <= 1.0 and 0.0 <= p.restitution <= 1.0 and 0.0 <= p.friction <= 1.0):
        raise ValueError("damping, restitution and friction must be in [0, 1]")
    if p.rest_speed < 0.0:
        raise ValueError("rest_speed must not be negative")
    if not 1 <= int(sweeps) <= 4:
        raise ValueError("sweeps must be 1..4")
    p.sweeps = int(sweeps)
    return p


def particle_step_tensor_count(states_in, states_out, draw, device):
    """Context.step_particles_async's arguments: contiguous tensors of N * 64, N * 64 and (unless None) N * 32 bytes on GPU `device`,
    16-byte aligned, N at most 2^20; `states_out` may be `states_in`'s memory, no other overlap.  Returns N; raises ValueError otherwise
    (a host tensor's address handed to the kernel would fault the device)."""
    named = [("states_in", states_in), ("states_out", states_out)] + ([("draw", draw)] if draw is not None else [])
    _device_tensors(device, *named)
    n = record_count("states_in", _nbytes(states_in), abi.PARTICLE_STATE_DTYPE.itemsize, MAX_PARTICLES, "RtParticleState")
    _holds("states_out", states_out, n, abi.PARTICLE_STATE_DTYPE.itemsize)
    if draw is not None:
        _holds("draw", draw, n, abi.PARTICLE_DTYPE.itemsize)
    spans = [(name, t.data_ptr(), t.data_ptr() + _nbytes(t)) for name, t in named]
    for i, (na, a0, a1) in enumerate(spans):
        for nb, b0, b1 in spans[i + 1:]:
            if a0 < b1 and b0 < a1 and not (na == "states_in" and nb == "states_out" and a0 == b0):
                raise ValueError("%s and %s overlap (only states_out may be states_in's memory, whole)" % (na, nb))
    return n


def make_particle_emitters(shapes, origins, speeds=0.0, drifts=0.0, spreads=0.0, halves=0.125, life_mins=np.inf, life_spans=0.0, densities=256,
                           responses=abi.RT_PARTICLE_DIE, seeds=0, lights=0, emissions=0xFF000000):
    """RtParticleEmit records (abi.EMIT_DTYPE) from `shapes` — SHAPE_DTYPE rows or a sequence of box_shape / sphere_shape rows, of which
    a, b and kind are read — float[N, 3] blast centres, and per emitter (one value serves all) the radial speed, float[3] drift, jitter
    amplitude, half edge, least life and its random span in seconds, density 1..256, RT_PARTICLE_* response, hash seed, light index
    and RGBA8 emission word.  Refuses what the calls refuse of these fields: more than 256 emitters, a non-finite float (life_min may
    be inf), half outside [2^-8, 0.5], speed or spread outside [0, 4096], |drift| above 4096, |origin| above 2^22, life_min <= 0,
    life_span outside [0, 4096], density outside 1..256, response above 3.  The shape itself is judged by the call (it needs R)."""
    shapes = _rows(shapes, SHAPE_DTYPE)
    n = shapes.size
    if n > abi.MAX_EMITTERS:
        raise ValueError("at most %d emitters per call" % abi.MAX_EMITTERS)
    e = np.zeros(n, dtype=abi.EMIT_DTYPE)
    e["a"], e["b"], e["kind"] = shapes["a"], shapes["b"], shapes["kind"]
    e["origin"] = np.broadcast_to(np.asarray(origins, dtype=np.float32), (n, 3))
    e["drift"] = np.broadcast_to(np.asarray(drifts, dtype=np.float32), (n, 3))
    for name, v in (("speed", speeds), ("spread", spreads), ("half", halves), ("life_min", life_mins), ("life_span", life_spans)):
        e[name] = np.broadcast_to(np.asarray(v, dtype=np.float32), (n,))
    densities = np.broadcast_to(np.asarray(densities, dtype=np.int64), (n,))
    responses = np.broadcast_to(np.asarray(responses, dtype=np.int64), (n,))
    if ((densities < 1) | (densities > 256)).any():
        raise ValueError("density must be 1..256")
    if ((responses < 0) | (responses > abi.RT_PARTICLE_BOUNCE)).any():
        raise ValueError("response must be an RT_PARTICLE_* value")
    e["density"], e["response"] = densities, responses
    for name, v in (("seed", seeds), ("light", lights), ("emission", emissions)):
        e[name] = np.broadcast_to(np.asarray(v, dtype=np.uint32), (n,))
    finite = [e[k] for k in ("origin", "drift", "speed", "spread", "half", "life_span")]
    if not all(np.isfinite(v).all() for v in finite) or np.isnan(e["life_min"]).any():
        raise ValueError("every float must be finite (life_min may be inf)")
    if ((e["half"] < np.float32(2.0 ** -8)) | (e["half"] > np.float32(0.5))).any():
        raise ValueError("half must be in [2^-8, 0.5]")
    if ((e["speed"] < 0) | (e["speed"] > 4096) | (e["spread"] < 0) | (e["spread"] > 4096)).any():
        raise ValueError("speed and spread must be in [0, 4096]")
    if (np.abs(e["drift"]) > 4096).any():
        raise ValueError("drift must lie within +-4096")
    if (np.abs(e["origin"]) > 2.0 ** 22).any():
        raise ValueError("origin must lie within +-2^22")
    if not (e["life_min"] > 0).all():
        raise ValueError("life_min must be positive")
    if ((e["life_span"] < 0) | (e["life_span"] > 4096)).any():
        raise ValueError("life_span must be in [0, 4096]")
    return e


def emit_cursor(cursor=(0, 0, 0)):
    """The cursor of Context.emit_particles as one abi.EMIT_CURSOR_DTYPE record in an array of its own: from such a record, an
    abi.RtEmitCursor or (next, emitted, dropped)."""
    cur = np.zeros(1, dtype=abi.EMIT_CURSOR_DTYPE)
    if isinstance(cursor, abi.RtEmitCursor):
        cur[0] = (cursor.next, cursor.emitted, cursor.dropped, cursor.reserved)
    elif isinstance(cursor, (np.ndarray, np.void)) and cursor.dtype == abi.EMIT_CURSOR_DTYPE:
        cur[0] = np.asarray(cursor).reshape(-1)[0]
    else:
        nxt, emitted, dropped = cursor
        cur[0] = (int(nxt), int(emitted), int(dropped), 0)
    return cur


def emit_tensor_capacity(states, cursor, device):
    """Context.emit_particles_async's device arguments: `states` a contiguous tensor of capacity * 64 bytes with capacity in 1..2^20,
    `cursor` one of exactly 16 bytes, both on GPU `device` and 16-byte aligned, not overlapping.  Returns the capacity; raises
    ValueError otherwise (a host tensor's address handed to the kernel would fault the device)."""
    _device_tensors(device, ("states", states), ("cursor", cursor))
    capacity = record_count("states", _nbytes(states), abi.PARTICLE_STATE_DTYPE.itemsize, abi.MAX_EMIT_CAPACITY, "RtParticleState")
    if capacity < 1:
        raise ValueError("states must hold at least one record")
    if _nbytes(cursor) != abi.EMIT_CURSOR_DTYPE.itemsize:
        raise ValueError("cursor must be a contiguous tensor of 16 bytes (one RtEmitCursor)")
    if states.data_ptr() < cursor.data_ptr() + 16 and cursor.data_ptr() < states.data_ptr() + _nbytes(states):
        raise ValueError("states and cursor overlap")
    return capacity


def deposit_counts(counts=None):
    """The counters of Context.deposit_particles as one abi.DEPOSIT_COUNT_DTYPE record in an array of its own: zeros for None, else
    from such a record, an abi.RtDepositCount or (deposited, voxels, occupied, outside)."""
    cnt = np.zeros(1, dtype=abi.DEPOSIT_COUNT_DTYPE)
    if counts is None:
        return cnt
    if isinstance(counts, abi.RtDepositCount):
        cnt[0] = (counts.deposited, counts.voxels, counts.occupied, counts.outside)
    elif isinstance(counts, (np.ndarray, np.void)) and counts.dtype == abi.DEPOSIT_COUNT_DTYPE:
        cnt[0] = np.asarray(counts).reshape(-1)[0]
    else:
        cnt[0] = tuple(int(v) for v in counts)
    return cnt


def settle_counts(counts=None):
    """The counters of Context.settle_voxels as one abi.SETTLE_COUNT_DTYPE record in an array of its own: zeros for None, else from
    such a record, an abi.RtSettleCount or (moved, falling, distance, chunks)."""
    cnt = np.zeros(1, dtype=abi.SETTLE_COUNT_DTYPE)
    if counts is None:
        return cnt
    if isinstance(counts, abi.RtSettleCount):
        cnt[0] = (counts.moved, counts.falling, counts.distance, counts.chunks)
    elif isinstance(counts, (np.ndarray, np.void)) and counts.dtype == abi.SETTLE_COUNT_DTYPE:
        cnt[0] = np.asarray(counts).reshape(-1)[0]
    else:
        cnt[0] = tuple(int(v) for v in counts)
    return cnt


def flow_counts(counts=None):
    """The counters of Context.flow_voxels as one abi.FLOW_COUNT_DTYPE record in an array of its own: zeros for None, else from such a
    record, an abi.RtFlowCount or (wetted, dried, changed, active, chunks)."""
    cnt = np.zeros(1, dtype=abi.FLOW_COUNT_DTYPE)
    if counts is None:
        return cnt
    if isinstance(counts, abi.RtFlowCount):
        cnt[0] = np.frombuffer(bytes(counts), dtype=abi.FLOW_COUNT_DTYPE)[0]
    elif isinstance(counts, (np.ndarray, np.void)) and counts.dtype == abi.FLOW_COUNT_DTYPE:
        cnt[0] = np.asarray(counts).reshape(-1)[0]
    else:
        w, d, c, a, k = (int(v) for v in counts)
        cnt[0] = (w, d, c, a, k, (0, 0, 0))
    return cnt


def detach_result(result=None):
    """The result of Context.detach_voxels as one abi.DETACH_RESULT_DTYPE record in an array of its own: for None zero counters and
    empty bounds (lo INT32_MAX, hi INT32_MIN), else a copy of such a record or of an abi.RtDetachResult."""
    res = np.zeros(1, dtype=abi.DETACH_RESULT_DTYPE)
    if result is None:
        res["lo"], res["hi"] = 0x7FFFFFFF, -0x80000000
    elif isinstance(result, abi.RtDetachResult):
        res[0] = np.frombuffer(bytes(result), dtype=abi.DETACH_RESULT_DTYPE)[0]
    elif isinstance(result, (np.ndarray, np.void)) and result.dtype == abi.DETACH_RESULT_DTYPE:
        res[0] = np.asarray(result).reshape(-1)[0]
    else:
        raise ValueError("result is None, an abi.RtDetachResult or an abi.DETACH_RESULT_DTYPE record")
    return res


def deposit_tensor_count(states, draw, counts, device):
    """Context.deposit_particles_async's device arguments: `states` a contiguous tensor of N * 64 bytes with N at most 2^20, `draw`
    (unless None) one of N * 32 bytes, `counts` (unless None) one of exactly 16 bytes, all on GPU `device` and 16-byte aligned, none
    overlapping another.  Returns N; raises ValueError otherwise (a host tensor's address handed to the kernel would fault the
    device)."""
    named = [("states", states)] + ([("draw", draw)] if draw is not None else []) + ([("counts", counts)] if counts is not None else [])
    _device_tensors(device, *named)
    n = record_count("states", _nbytes(states), abi.PARTICLE_STATE_DTYPE.itemsize, MAX_PARTICLES, "RtParticleState")
    if draw is not None:
        _holds("draw", draw, n, abi.PARTICLE_DTYPE.itemsize)
    if counts is not None and _nbytes(counts) != abi.DEPOSIT_COUNT_DTYPE.itemsize:
        raise ValueError("counts must be a contiguous tensor of 16 bytes (one RtDepositCount)")
    spans = [(name, t.data_ptr(), t.data_ptr() + _nbytes(t)) for name, t in named]
    for i, (na, a0, a1) in enumerate(spans):
        for nb, b0, b1 in spans[i + 1:]:
            if a0 < b1 and b0 < a1:
                raise ValueError("%s and %s overlap" % (na, nb))
    return n


def check_shadow_box_tensor(boxes, device):
    """Context.shadow_entities_async's device argument: a contiguous tensor of N * 32 bytes on GPU `device`, 16-byte aligned, N at most
    4096.  Returns N; raises ValueError otherwise (a host tensor's address handed to the kernel would fault the device)."""
    _device_tensors(device, ("boxes", boxes))
    return _box_count(boxes)


# world axis k of a placed stamp is stamp axis STAMP_PERMS[orient >> 3][k] (include/rt_abi.h, rt_edit_stamps)
STAMP_PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def make_draw_stamps(stamps, origins, scales=1.0, orients=0, emissions=0xFF000000):
    """RtDrawStamp records (DRAW_STAMP_DTYPE) from u32[N] stamp ids, float[N, 3] low corners, float[N] scales, int[N] orientations and
    u32[N] RGBA8 emission words (one value serves every model).  Refuses what can be refused without the stamps' extents: a non-finite
    float, an origin beyond 2^22, a scale outside [2^-8, 64], orient >= 48, more than 4096 models."""
    origin = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    n = origin.shape[0]
    if n > MAX_DRAW_STAMPS:
        raise ValueError("at most %d models per call" % MAX_DRAW_STAMPS)
    scale = np.broadcast_to(np.asarray(scales, dtype=np.float32), (n,))
    orient = np.broadcast_to(np.asarray(orients, dtype=np.int64), (n,))
    if not (np.isfinite(origin).all() and np.isfinite(scale).all()):
        raise ValueError("origins and scales must be finite")
    if n and np.abs(origin).max() > 2.0 ** 22:
        raise ValueError("origins must lie within +-2^22")
    if n and (scale.min() < 2.0 ** -8 or scale.max() > 64.0):
        raise ValueError("scales must lie within [2^-8, 64]")
    if n and (orient.min() < 0 or orient.max() >= 48):
        raise ValueError("orient is 0..47")
    m = np.zeros(n, dtype=DRAW_STAMP_DTYPE)
    m["origin"], m["scale"], m["orient"] = origin, scale, orient
    m["stamp"] = np.broadcast_to(np.asarray(stamps, dtype=np.uint32), (n,))
    m["emission"] = np.broadcast_to(np.asarray(emissions, dtype=np.uint32), (n,))
    return m


def stamp_bounding_boxes(models, extents):
    """(lo, hi) float32[N, 3] of the models' bounding boxes: lo = origin, hi = origin + E' * scale with E'_k = E[perm[k]].  `extents`:
    int[N, 3] stamp extents (ex, ey, ez) per model, or one triple for all."""
    models = _records(models, DRAW_STAMP_DTYPE)
    n = models.size
    ext = np.broadcast_to(np.asarray(extents, dtype=np.int64).reshape(-1, 3), (n, 3))
    perm = np.array(STAMP_PERMS, dtype=np.int64)[models["orient"].astype(np.int64) >> 3] if n else np.zeros((0, 3), dtype=np.int64)
    placed = np.take_along_axis(ext, perm, axis=1)
    lo = models["origin"].astype(np.float32)
    hi = (placed.astype(np.float64) * models["scale"].astype(np.float64)[:, None] + lo.astype(np.float64)).astype(np.float32)
    return lo, hi


def stamp_face_probes(models, extents, cells=(0, 0)):
    """The six RtLightProbe records (PROBE_DTYPE) per model that light its bounding box's faces, as face_probes does for boxes: record
    6 i + n sits at the centre of the face with normal code n, 0.001 off it.  probe_records(u, stamp_face_probes(models, extents),
    samples, depth) is the face_lights of draw_stamps."""
    lo, hi = stamp_bounding_boxes(models, extents)
    boxes = np.zeros(lo.shape[0], dtype=DRAW_BOX_DTYPE)
    boxes["lo"], boxes["hi"] = lo, hi
    return face_probes(boxes, cells)


def check_draw_stamp_lights(n, face_lights, device):
    """Context.draw_stamps_async's device argument: a contiguous tensor of 6 n * 16 bytes on GPU `device`, 16-byte aligned, n at most
    4096.  Raises ValueError otherwise (a host tensor's address handed to the kernel would fault the device)."""
    _device_tensors(device, ("face_lights", face_lights))
    record_count("models", n * DRAW_STAMP_DTYPE.itemsize, DRAW_STAMP_DTYPE.itemsize, MAX_DRAW_STAMPS)     # the models are host records: n is exact
    _holds("face_lights", face_lights, n, PROBE_LIGHT_DTYPE.itemsize, per=6)


def make_point_lights(positions, radii, colors):
    """RtPointLight records (POINT_LIGHT_DTYPE) from float[N, 3] positions, float[N] radii and float[N, 3] colours in the shader's light
    unit (one radius or colour serves every light).  Refuses what rt_add_lights refuses: a non-finite float, a coordinate beyond 2^22,
    a radius outside (0, 1024], a colour outside [0, 2^20], more than 1024 lights."""
    pos = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
    n = pos.shape[0]
    if n > MAX_POINT_LIGHTS:
        raise ValueError("at most %d lights per call" % MAX_POINT_LIGHTS)
    radius = np.broadcast_to(np.asarray(radii, dtype=np.float32), (n,))
    color = np.broadcast_to(np.asarray(colors, dtype=np.float32), (n, 3))
    if not (np.isfinite(pos).all() and np.isfinite(radius).all() and np.isfinite(color).all()):
        raise ValueError("positions, radii and colours must be finite")
    if n and np.abs(pos).max() > 2.0 ** 22:
        raise ValueError("positions must lie within +-2^22")
    if not ((radius > 0) & (radius <= 1024.0)).all():
        raise ValueError("radii must lie in (0, 1024]")
    if not ((color >= 0) & (color <= 2.0 ** 20)).all():
        raise ValueError("colours must lie in [0, 2^20]")
    lights = np.zeros(n, dtype=POINT_LIGHT_DTYPE)
    lights["position"], lights["radius"], lights["color"] = pos, radius, color
    return lights


def check_point_light_tensors(lights, device):
    """Context.add_lights_async's argument: a contiguous tensor of N * 32 bytes on GPU `device`, 16-byte aligned, N at most 1024.
    Returns N; raises ValueError otherwise (a host tensor's address handed to the kernel would fault the device)."""
    _device_tensors(device, ("lights", lights))
    return record_count("lights", _nbytes(lights), POINT_LIGHT_DTYPE.itemsize, MAX_POINT_LIGHTS, "RtPointLight")


def make_probes(positions, normals, cells):
    """RtLightProbe records (PROBE_DTYPE) from float[N, 3] positions, int[N] normal codes and int[N, 2] noise cells."""
    pos = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
    nrm = np.asarray(normals).reshape(-1)
    cell = np.asarray(cells).reshape(-1, 2)
    if nrm.size != pos.shape[0] or cell.shape[0] != pos.shape[0]:
        raise ValueError("positions, normals and cells must describe the same number of probes")
    if pos.shape[0] and (cell.min() < 0 or cell.max() > 0xFFFF or nrm.min() < 0 or nrm.max() > 0xFFFFFFFF):
        raise ValueError("cells must fit uint16 and normals uint32 (the library checks the normal codes)")
    probes = np.zeros(pos.shape[0], dtype=PROBE_DTYPE)
    probes["position"], probes["normal"], probes["cell"] = pos, nrm, cell
    return probes


def workgroup_of(p):
    """The noise cell of a frame's pixel coordinate: the shader workgroup that owns it (raytrace.comp:291-294)."""
    p = np.asarray(p, dtype=np.int64)
    return (p // 128) * 16 + p % 16


def check_probe_tensors(probes, out, device):
    """Context.probe_light_async's arguments: contiguous tensors of N * 32 and N * 16 bytes on GPU `device`, 16-byte aligned.
    Returns N; raises ValueError otherwise (a host tensor's address handed to the kernel would fault the device)."""
    _device_tensors(device, ("probes", probes), ("out", out))
    n = record_count("probes", _nbytes(probes), PROBE_DTYPE.itemsize, None, "RtLightProbe")
    _holds("out", out, n, PROBE_LIGHT_DTYPE.itemsize)
    return n


def comm_unique_id():
    """ncclGetUniqueId: 128 opaque bytes one rank creates and the host hands to every rank (rt_comm_unique_id)."""
    buf = (C.c_char * 128)()
    rc = _lib.amd().rt_comm_unique_id(buf, 128)
    if rc != 0:
        raise RtError(rc, _lib.amd().rt_last_error(None).decode())
    return bytes(buf)


def comm_destroy(comm):
    if comm:
        _lib.amd().rt_comm_destroy(C.c_void_p(comm))
