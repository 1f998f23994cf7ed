"""RtConfig.stream_history restated in numpy float32 (include/rt_abi.h RT_FLAG_REPROJECT, DESIGN.md "Slabs under a kept history"):
tests/edit_history_ref.EditHistory plus the pending slabs, their occupancy masks, the boxes placed per set bit and the frame
classification with them.

    h = SlabHistory(W, H, cap=32, edit_radius=4, region=256, stream_history=1)
    h.slab(old_masks, new_masks)      # an accepted rt_upload_slice / rt_generate_slice (the masks: slab_masks of the minefield)
    h.slabs_pending()                 # rt_slabs_pending
    lighting_f32, lighting_rgba16, counts, accepted = h.step(planes_of_the_oracle_frame_of_the_NEW_world, uniforms)
    h.slab_boxes                      # rt_read_slab_boxes after that frame

A frame that goes on with pending slabs has mode "moved_slabs", whether or not a box came of them.  `SlabWalk` keeps the world
beside the history; the sequences the CPU contract test and the GPU test share are at the end."""
import numpy as np

from raytrace_amd import world
from tests import edit_history_ref as er
from tests import temporal_ref as tr

f32 = np.float32
MAX_SLABS = 4
SLICE = 16


def slab_slices(axis, t0):
    """Index of the 16-thick slab at texel t0 of `axis` in a [z, y, x] array."""
    s = [slice(None)] * 3
    s[2 - axis] = slice(int(t0), int(t0) + SLICE)
    return tuple(s)


def slab_masks(mine, axis, t0):
    """bool[3, R]: bits[a][t] — some occupied voxel (minefield byte 0) of the slab has coordinate t on axis a."""
    return masks_of_slab(mine[slab_slices(axis, t0)], axis, t0)


def masks_of_slab(slab_mine, axis, t0):
    """slab_masks from the slab's own bytes ([z, y, x], 16 thick along `axis`: what rt_read_box returns of it)."""
    R = max(slab_mine.shape)
    occ = slab_mine == 0
    bits = np.zeros((3, R), dtype=bool)
    for a in range(3):
        line = occ.any(axis=tuple(k for k in range(3) if k != 2 - a))
        if a == axis:
            bits[a, t0:t0 + SLICE] = line
        else:
            bits[a] = line
    return bits


def place(bits, lr, region):
    """[(lo, hi)] float32[3] — the world box of a mask set under render offset lr, or [] for a set without a bit:
    w_a(t) = lr_a - R/2 + (t - lr_a) mod R per set bit, lo = min w, hi = max w + 1."""
    if not bits.any():
        return []
    R = int(region)
    lo, hi = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64)
    for a in range(3):
        t = np.nonzero(bits[a])[0].astype(np.int64)
        w = int(lr[a]) - R // 2 + (t - int(lr[a])) % R
        lo[a], hi[a] = w.min(), w.max() + 1
    return [(lo.astype(f32), hi.astype(f32))]


class SlabHistory(er.EditHistory):
    def __init__(self, width, height, cap=tr.DEFAULT_CAP, edit_radius=0, region=256, stream_history=0):
        super().__init__(width, height, cap, edit_radius, region)
        self.stream = int(stream_history)
        self.slabs, self.slab_overflowed = [], False     # pending: (old masks, new masks) in call order
        self.frame_slabs = 0                             # the frame in step(): the slabs it consumed ...
        self.slab_boxes = []                             # ... and the boxes they gave (rt_read_slab_boxes)

    def reset(self):
        super().reset()
        self.slabs, self.slab_overflowed = [], False

    def slab(self, old, new):
        """An ACCEPTED slab (a rejected one changes nothing here)."""
        if not self.stream:
            self.reset()
        elif self.slab_overflowed:
            pass
        elif len(self.slabs) == MAX_SLABS:
            self.slabs, self.slab_overflowed = [], True
        else:
            self.slabs.append((old, new))

    def slabs_pending(self):
        return len(self.slabs), self.slab_overflowed

    def step(self, planes, u):
        if self.overflowed or self.slab_overflowed:
            self.valid = False
        lr = [int(v) for v in u.lr[:]]
        boxes = [er.world_box(b, lr, self.region) for b in self.boxes]
        self.frame_slabs, self.slab_boxes = len(self.slabs), []
        if self.valid:
            prev_lr = self.key[13:16]
            for old, new in self.slabs:
                self.slab_boxes += place(old, prev_lr, self.region) + place(new, lr, self.region)
        self.frame_boxes = boxes + self.slab_boxes
        self.sun = er.po.sun(u.sun_angle)[0]
        self.boxes, self.overflowed, self.slabs, self.slab_overflowed = [], False, [], False
        out = tr.History.step(self, planes, u)
        if self.mode != "moved_slabs":
            self.slab_boxes = []                         # (a frame that restarts places nothing)
        return out

    def _classify(self, key):
        mode = tr.History._classify(self, key)
        if mode == "restart":
            return mode
        return "moved_slabs" if self.frame_slabs else ("moved_boxes" if self.frame_boxes else mode)

    def _moved(self, cam, L, nrm, dep):
        s, n, acc = super()._moved(cam, L, nrm, dep)
        if not self.frame_boxes:
            none = np.zeros((self.H, self.W), dtype=bool)
            self.touch = dict(near=none, shadow=none, touched=none, base_accepted=acc, P=None)
        return s, n, acc


class SlabWalk(er.Walk):
    def __init__(self, region_arrays, noise, width, height, edit_radius=er.RADIUS, cap=tr.DEFAULT_CAP, region=256, depth=2,
                 stream_history=1):
        super().__init__(region_arrays, noise, width, height, edit_radius, cap, region, depth)
        self.h = SlabHistory(width, height, cap, edit_radius, region, stream_history)

    def slab(self, axis, t0, mats, mine):
        """rt_upload_slice(axis, t0, mats, mine), accepted: the slab replaces the world's; the masks are taken round the write."""
        if not self.owned:
            self.mats, self.mine, self.owned = self.mats.copy(), self.mine.copy(), True
        sl = slab_slices(axis, t0)
        old = slab_masks(self.mine, axis, t0)
        self.mats[sl] = np.asarray(mats).reshape(self.mats[sl].shape)
        self.mine[sl] = np.asarray(mine).reshape(self.mine[sl].shape)
        self.h.slab(old, slab_masks(self.mine, axis, t0))


# ---- scrolls: the slab a 16-voxel move of the window brings, cut out of world.toroidal_region of the new lr ---------------------
_regions = {}


def window(lr, region=256):
    """world.toroidal_region(lr), read-only; at R = 256 built once per lr and shared (80 MB each: the sequences need a dozen)."""
    key = (tuple(int(v) for v in lr), int(region))
    if key in _regions:
        return _regions[key]
    m, f = world.toroidal_region(key[0], region=key[1])
    m.setflags(write=False)
    f.setflags(write=False)
    if key[1] == 256:
        _regions[key] = (m, f)
    return m, f


def scroll(lr, axis, inc, region=256):
    """(lr after the move, texel offset of the slab it rewrites, window_lo of rt_generate_slice)."""
    R = int(region)
    lr1 = list(lr)
    lr1[axis] += SLICE if inc else -SLICE
    first = lr[axis] + R // 2 if inc else lr1[axis] - R // 2        # the first world voxel that arrives
    lo = [lr1[a] - R // 2 for a in range(3)]
    lo[axis] = first
    return tuple(lr1), (first + R // 2) % R, tuple(lo)


def scroll_op(lr, axis, inc, region=256):
    """(("slab", axis, t0, mats, mine, window_lo), lr after): the op of one scroll from lr."""
    lr1, t0, lo = scroll(lr, axis, inc, region)
    m, f = window(lr1, region)
    sl = slab_slices(axis, t0)
    return ("slab", axis, t0, np.ascontiguousarray(m[sl]), np.ascontiguousarray(f[sl]), lo), lr1


def same_op(lr, axis, t0, region=256):
    """The slab at t0 of the window at lr, uploaded again: the world and lr stay as they are."""
    m, f = window(lr, region)
    sl = slab_slices(axis, t0)
    R = int(region)
    lo = [lr[a] - R // 2 for a in range(3)]
    lo[axis] = int(lr[axis] - R // 2 + (t0 - lr[axis]) % R)
    return ("slab", axis, t0, np.ascontiguousarray(m[sl]), np.ascontiguousarray(f[sl]), tuple(lo))


def dotted_op(lr, axis, t0, texels, region=256):
    """That slab with the voxels at `texels` (x, y, z rows, inside the slab) made solid: host bytes only (window_lo is None)."""
    op = same_op(lr, axis, t0, region)
    R = int(region)
    m, f = np.zeros((R, R, R), np.uint32), np.ones((R, R, R), np.uint8)
    sl = slab_slices(axis, t0)
    m[sl], f[sl] = op[3], op[4]
    for x, y, z in texels:
        m[z, y, x], f[z, y, x] = er.WORD, 0
    return ("slab", axis, t0, np.ascontiguousarray(m[sl]), np.ascontiguousarray(f[sl]), None)


# ---- the sequences: lists of ("frame", uniforms), ("slab", axis, t0, mats, mine, window_lo) and edit_history_ref's ("edit", ...) --
W, H, DEPTH, RADIUS = er.W, er.H, er.DEPTH, er.RADIUS
SW, SH = er.SW, er.SH
# The two cameras: edit_history_ref.CAMERA (36 above the terrain, looking down along +y, sun 1.0 rad: the sun vector is mostly +y,
# so that what arrives at the window's +y edge shadows most of the view) and temporal_ref.path_uniforms' (100 up, looking along +y
# at the horizon, sun 0.3: it sees the terrain out to the window's edges, where an x slab lies within the radius of a few pixels).
# "edge" is the first one moved to 38 voxels from the window's -x edge: the x slab that leaves there lies within the radius of the
# pixels on its left.
CAMERAS = {"down": er.CAMERA, "far": dict(base=tr.TERRAIN_BASE, pitch=-0.02, sun=0.3), "edge": dict(er.CAMERA, base=(-90.0, -60.0, 50.0))}
AIR_T0 = 240                                       # world z 112..127 of the window at lr z = 0: above the terrain, nothing occupied


def frames(steps, lr, first=0, camera="down", **kw):
    c = dict(CAMERAS[camera])
    c.update(kw)
    return [("frame", tr.path_uniforms(first + i, step=s, lr=lr, **c)) for i, s in enumerate(steps)]


def main_ops(axis=0, inc=True, camera="edge", lr=(0, 0, 0), **kw):
    """Path (frames 0..3), the scroll's slab, three moved frames (4..6) under the new lr, one still frame (7 at pose 6)."""
    op, lr1 = scroll_op(lr, axis, inc)
    return frames((0, 1, 2, 3), lr, camera=camera, **kw) + [op] + frames((4, 5, 6, 6), lr1, first=4, camera=camera, **kw)


def short_ops(slabs, lr1, camera="down", lr=(0, 0, 0), **kw):
    """Two path frames, the slab ops, two moved frames under lr1."""
    return frames((0, 1), lr, camera=camera, **kw) + list(slabs) + frames((2, 3), lr1, first=2, camera=camera, **kw)


def scroll_ops(axis, inc, camera="down", **kw):
    op, lr1 = scroll_op((0, 0, 0), axis, inc)
    return short_ops([op], lr1, camera, **kw)


# the axis / direction runs: (axis, increasing, camera) — x under the camera that sees the window's x edges, y under the one whose
# sun shadow falls along y, z under either
AXES = [(0, True, "far"), (0, False, "far"), (1, True, "down"), (1, False, "down"), (2, True, "down"), (2, False, "far")]


def chain_ops(moves, lr=(0, 0, 0), camera="down", **kw):
    """Several scrolls before one frame: (axis, inc) each, every one from where the one before left lr."""
    ops, at = [], lr
    for axis, inc in moves:
        op, at = scroll_op(at, axis, inc)
        ops.append(op)
    return short_ops(ops, at, camera, lr, **kw)


# Region 512 with a scrolling window: frame k has lr = edit_history_ref.seam_lr(k) = (k // 2, -(k // 3), 0), so frame 6 places with
# lr = (3, -2, 0) and the window's seam lies at texels x = 3, y = 510.  Before it the z slab at texel 368 (world z 112..127: air) comes
# again with four solid voxels in it, at texels x = 1 and 6, y = 505 and 1: on both sides of the seam on both other axes.  Placed per
# bit they are world x 257 and -250, y 249 and -255: the box [-250, 258) x [-255, 250) x [114, 115), not the window
# [-253, 259) x [-258, 254) that a texel box cut by the seam would become.  What left is air: one box.
SEAM_T0, SEAM_FRAME = 368, 6
SEAM_TEXELS = [(1, 505, 370), (6, 505, 370), (1, 1, 370), (6, 1, 370)]
SEAM_BOX = ((-250.0, -255.0, 114.0), (258.0, 250.0, 115.0))


def seam_ops():
    ops = []
    for k, s in enumerate(tr.GPU_PATH_STEPS[:9]):
        if k == SEAM_FRAME:
            ops.append(dotted_op((0, 0, 0), 2, SEAM_T0, SEAM_TEXELS, region=512))
        ops.append(("frame", tr.path_uniforms(k, step=s, lr=er.seam_lr(k))))
    return ops


def run(walk, ops):
    """Walks ops on the reference alone: per frame what edit_history_ref.run gives, plus the slabs pending before it, the slabs it
    consumed and their boxes."""
    out = []
    for op in ops:
        if op[0] == "edit":
            walk.edit(*op[1:])
        elif op[0] == "slab":
            walk.slab(*op[1:5])
        else:
            pending, slabs = walk.h.pending(), walk.h.slabs_pending()
            want, counts = walk.frame(op[1])
            h = walk.h
            out.append(dict(planes=want, counts=counts, mode=h.mode, touch=dict(h.touch) if h.mode in ("moved_boxes", "moved_slabs") else None,
                            accumulation=(h.frames, h.samples), pending_before=pending, slabs_before=slabs, boxes=list(h.frame_boxes),
                            slab_boxes=list(h.slab_boxes), hit=(h.nrm < 6) & (h.dep < f32(65535.0)), uniforms=op[1]))
    return out
