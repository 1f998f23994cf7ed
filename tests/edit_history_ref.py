"""RtConfig.edit_radius restated in numpy float32 (include/rt_abi.h RT_FLAG_REPROJECT, DESIGN.md "Edits under a kept history"):
tests/temporal_ref.History plus the pending edit boxes, the frame classification with them and the per-pixel near / shadow test.

    h = EditHistory(W, H, cap=32, edit_radius=4, region=256)
    h.edit(xyz)                       # rt_edit_voxels(count > 0): one texel box per touched 64^3 chunk, or the overflow mark
    h.pending()                       # rt_edit_boxes_pending
    lighting_f32, lighting_rgba16, counts, accepted = h.step(planes_of_the_oracle_frame_of_the_EDITED_world, uniforms)

A frame that goes on with boxes has mode "moved_boxes"; h.touch then holds what the test saw of every pixel.  `Walk` keeps the
edited world (tests/voxel_edits.apply_edits) and the oracle's frames beside the history; the sequences the CPU contract test and
the GPU test share are at the end."""
import numpy as np

from oracle import pyoracle as po
from tests import temporal_ref as tr
from tests import voxel_edits as ve

f32 = np.float32
MAX_BOXES = 16
MAX_RADIUS = 64


def rmin(x, y):
    """rtm_min(x, y) = y < x ? y : x, elementwise."""
    return np.where(y < x, y, x)


def rmax(x, y):
    """rtm_max(x, y) = x < y ? y : x, elementwise."""
    return np.where(x < y, y, x)


def chunk_boxes(xyz, region=256):
    """One texel box (lo[3], hi[3], inclusive) per touched 64^3 chunk, in chunk order (z, then y, then x): the min / max over
    every record of the chunk, whether or not it changes the voxel."""
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    nl = int(region).bit_length() - 1 - 6
    c = ((xyz[:, 2] >> 6) << (2 * nl)) | ((xyz[:, 1] >> 6) << nl) | (xyz[:, 0] >> 6)
    return [(xyz[c == k].min(axis=0), xyz[c == k].max(axis=0)) for k in np.unique(c)]


def world_box(box, lr, region=256):
    """(lo, hi) float32[3] of a texel box in the world coordinates of a frame with render offset lr: render.texel_to_world's
    w = lr - R/2 + (t - lr) mod R per axis, the box [w(min), w(max) + 1]; the whole window where its seam cuts the box."""
    R = int(region)
    lr = np.asarray(lr, dtype=np.int64)
    base = lr - R // 2
    lo = base + (box[0] - lr) % R
    hi = base + (box[1] - lr) % R
    cut = lo > hi
    return np.where(cut, base, lo).astype(f32), np.where(cut, base + R, hi + 1).astype(f32)


def touch_test(P, boxes, radius, sun):
    """The per-pixel test on hit points P float32[..., 3]: (near, shadowed) bool arrays, each the OR over the boxes."""
    s = np.asarray(sun, dtype=f32)
    with np.errstate(all="ignore"):
        inv = f32(1) / s
    r2 = f32(radius * radius)
    near = np.zeros(P.shape[:-1], dtype=bool)
    shadow = np.zeros(P.shape[:-1], dtype=bool)
    one, zero = f32(1), f32(0)
    with np.errstate(all="ignore"):
        for lo, hi in boxes:
            d = []
            tn = np.full(P.shape[:-1], -np.inf, dtype=f32)
            tf = np.full(P.shape[:-1], np.inf, dtype=f32)
            miss = np.zeros(P.shape[:-1], dtype=bool)
            for k in range(3):
                p = P[..., k]
                if s[k] != 0:
                    ta = ((lo[k] - one) - p) * inv[k]
                    tb = ((hi[k] + one) - p) * inv[k]
                    tn = rmax(tn, rmin(ta, tb))
                    tf = rmin(tf, rmax(ta, tb))
                else:
                    miss |= ~(((lo[k] - one) <= p) & (p <= (hi[k] + one)))
                d.append(rmax(rmax(lo[k] - p, p - hi[k]), zero))
            dist2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            near |= dist2 <= r2
            shadow |= ~miss & (tn <= tf) & (tf > 0)
    return near, shadow


class EditHistory(tr.History):
    def __init__(self, width, height, cap=tr.DEFAULT_CAP, edit_radius=0, region=256):
        super().__init__(width, height, cap)
        self.radius, self.region = int(edit_radius), int(region)
        self.boxes, self.overflowed = [], False      # pending: texel boxes in call order
        self.frame_boxes, self.sun = [], None        # the frame in step(): its world boxes and sun vector
        self.touch = {}                              # moved_boxes frames: near, shadow, touched, base_accepted (bool [H, W])

    def reset(self):
        """An upload, rt_generate_*, rt_upload_noise or rt_reset_accumulation: the next frame restarts and pending boxes go."""
        super().reset()
        self.boxes, self.overflowed = [], False

    def edit(self, xyz):
        """rt_edit_voxels with count > 0 (the world itself is the caller's: see Walk)."""
        if self.radius == 0:
            self.valid = False
            return
        if self.overflowed:
            return
        new = chunk_boxes(xyz, self.region)
        if len(self.boxes) + len(new) > MAX_BOXES:
            self.boxes, self.overflowed = [], True
        else:
            self.boxes += new

    def pending(self):
        return len(self.boxes), self.overflowed

    def step(self, planes, u):
        if self.overflowed:
            self.valid = False
        self.frame_boxes = [world_box(b, u.lr[:], self.region) for b in self.boxes]
        self.sun = po.sun(u.sun_angle)[0]
        self.boxes, self.overflowed = [], False      # the frame consumes them
        return super().step(planes, u)

    def _classify(self, key):
        mode = super()._classify(key)
        return "moved_boxes" if mode != "restart" and self.frame_boxes else mode

    def _moved(self, cam, L, nrm, dep):
        s, n, acc = super()._moved(cam, L, nrm, dep)
        if not self.frame_boxes:
            return s, n, acc
        W, H = self.W, self.H
        ys, xs = np.mgrid[0:H, 0:W]
        with np.errstate(all="ignore"):
            P = cam[0] + tr.directions(cam, xs, ys, W, H) * (dep / f32(32))[..., None]      # step 2
        near, shadow = touch_test(P, self.frame_boxes, self.radius, self.sun)
        hit = self.diag["hit"]
        touched = hit & (near | shadow)
        s = np.where(touched[..., None], f32(0) + L, s).astype(f32)
        n = np.where(touched, 1, n).astype(np.uint32)
        self.touch = dict(near=near & hit, shadow=shadow & hit, touched=touched, base_accepted=acc, P=P)
        return s, n, acc & ~touched


class Walk:
    """The reference beside a context: the edited world, the oracle's one-sample frames of it and the history."""

    def __init__(self, region_arrays, noise, width, height, edit_radius, cap=tr.DEFAULT_CAP, region=256, depth=2):
        self.mats, self.mine = region_arrays
        self.owned = False
        self.noise, self.W, self.H, self.R, self.depth = noise, int(width), int(height), int(region), int(depth)
        self.h = EditHistory(width, height, cap, edit_radius, region)

    def edit(self, xyz, words, solid):
        if not self.owned:
            self.mats, self.mine, self.owned = self.mats.copy(), self.mine.copy(), True
        ve.apply_edits(self.mats, self.mine, xyz, words, solid)
        self.h.edit(xyz)

    def render(self, u, spp=1):
        return po.render(self.mats, self.mine, self.noise, u, self.W, self.H, spp, self.depth, region=self.R)[0]

    def frame(self, u):
        """(planes the contract asks for, counts) of the next frame."""
        want = dict(self.render(u))
        want["lighting_f32"], want["lighting_rgba16"], counts, _ = self.h.step(want, u)
        return want, counts


# ---- the sequences: lists of ("frame", uniforms) and ("edit", xyz, words, solid) ------------------------------------------------
# tests/test_edit_history_contract.py asserts on the CPU what each one exercises; tests/test_gpu_edit_history.py walks them.
W, H, DEPTH = 104, 56, 2          # the main frame (a partial tile in x); the small one is temporal_ref.SEQ_W x SEQ_H = 72 x 44
SW, SH = tr.SEQ_W, tr.SEQ_H
RADIUS = 4
WORD = (1 << 15) | (90 << 14) | (60 << 7) | 30     # the material word of rt_bench's edit brush
# The camera: 36 voxels above the terrain, looking down at -0.5 rad along +y, a low sun (1.0 rad) behind its left shoulder, so
# that a pillar's shadow is long and falls towards the camera.  The centre pixel of pose 4 sees the top of texel (98, 133, 141).
CAMERA = dict(base=(-30.0, -60.0, 50.0), pitch=-0.5, sun=1.0)
PILLAR = (97, 132, 142, 3, 3, 10)                  # x0, y0, z0, ex, ey, ez: 3 x 3 x 10 on that surface
PIT = (96, 131, 138, 5, 5, 4)                      # the ground round its place, for the broken block (the top layer is partly air)


def block(x0, y0, z0, ex, ey, ez, solid=1, word=WORD):
    """("edit", xyz, words, solid) of the box [x0, x0 + ex) x [y0, y0 + ey) x [z0, z0 + ez), texel coordinates."""
    z, y, x = np.mgrid[z0:z0 + ez, y0:y0 + ey, x0:x0 + ex]
    xyz = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    return ("edit", xyz, np.full(len(xyz), word if solid else 0, np.uint32), np.full(len(xyz), solid, bool))


def pose(k, step=None, **kw):
    for name, v in CAMERA.items():
        kw.setdefault(name, v)
    return tr.path_uniforms(k, step=step, **kw)


def frames(steps, first=0, **kw):
    return [("frame", pose(first + i, step=s, **kw)) for i, s in enumerate(steps)]


def main_ops(edit=None, **kw):
    """Path (frames 0..3), the edit (default: the pillar), three moved frames (4..6), one still frame (7 at pose 6)."""
    return frames((0, 1, 2, 3), **kw) + [edit or block(*PILLAR)] + frames((4, 5, 6, 6), first=4, **kw)


def still_ops():
    """A camera that holds still: three frames, the pillar, two more — the first of them the moved pass into the same camera."""
    return frames((2, 2, 2)) + [block(*PILLAR)] + frames((2, 2), first=3)


# sixteen one-voxel calls on the ground round the pillar's place, 4 apart (one box each), and a seventeenth
SINGLES = [block(90 + 4 * (i % 4), 124 + 4 * (i // 4), 143, 1, 1, 1) for i in range(17)]


def boxes_ops(n):
    """n one-voxel edit calls before frame 2; four frames in all."""
    return frames((0, 1)) + SINGLES[:n] + frames((2, 3), first=2)


# Region 512 with a scrolling window: frame k has lr = (k // 2, -(k // 3), 0), so the seam of the window lies at texel x = 3 when
# the edit before frame 6 is placed: its box, texels x 2..4, is cut and covers the whole window in x.  y and z put that slab
# through the terrain the camera (temporal_ref's default path) looks at.
SEAM_BLOCK = (2, 326, 292, 3, 3, 10)
SEAM_EDIT_FRAME = 6


def seam_lr(k):
    return (k // 2, -(k // 3), 0)


def seam_ops():
    ops = []
    for k, s in enumerate(tr.GPU_PATH_STEPS[:9]):
        if k == SEAM_EDIT_FRAME:
            ops.append(block(*SEAM_BLOCK))
        ops.append(("frame", tr.path_uniforms(k, step=s, lr=seam_lr(k))))
    return ops


def run(walk, ops):
    """Walks ops on the reference alone: per frame a dict of planes, counts, mode, touch (moved_boxes frames), accumulation and
    what was pending before the frame."""
    out = []
    for op in ops:
        if op[0] == "edit":
            walk.edit(*op[1:])
        else:
            pending = walk.h.pending()
            want, counts = walk.frame(op[1])
            h = walk.h
            out.append(dict(planes=want, counts=counts, mode=h.mode, touch=dict(h.touch) if h.mode == "moved_boxes" else None,
                            accumulation=(h.frames, h.samples), pending_before=pending, boxes=list(h.frame_boxes)))
    return out
