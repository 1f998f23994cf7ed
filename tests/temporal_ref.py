"""RT_FLAG_REPROJECT restated in numpy float32 (include/rt_abi.h, DESIGN.md "Reprojection"): one history set and the previous
camera, fed with the oracle's one-sample frames.  Every operation is a float32 array operation rounded on its own; directions come
from the oracle's normalize (rtm_normalize3, the one primary_ray uses), the UNORM plane from the oracle's unorm.

    h = History(W, H, cap=32)
    lighting_f32, lighting_rgba16, counts, accepted = h.step(planes_of_the_oracle_frame, uniforms)

`accepted` marks the pixels that continued a history (every pixel of a still frame, none of a restart)."""
import numpy as np

from oracle import pyoracle as po

f32 = np.float32
DEFAULT_CAP = 32
MAX_SAMPLES = 1 << 24
PLANE_TOLERANCE = f32(0.25)


def live_key(u):
    """The live uniforms other than seed, as bit patterns: (sun_angle, origin, forward, up, right, lr)."""
    cam = np.array([u.sun_angle] + list(u.origin) + list(u.forward) + list(u.up) + list(u.right), dtype=f32).view(np.uint32)
    return tuple(int(v) for v in cam) + tuple(int(v) for v in u.lr)


def camera_of(u):
    g = lambda a: np.array(a[:], dtype=f32)
    return g(u.origin), g(u.forward), g(u.right), g(u.up)


def dotp(a, b):
    return (a[..., 0] * b[0] + a[..., 1] * b[1]) + a[..., 2] * b[2]


def directions(cam, xs, ys, W, H):
    """primary_ray's direction of pixels (xs, ys) (integer arrays of one shape) under `cam`: float32[..., 3]."""
    _, fwd, right, up = cam
    sx = (xs.astype(f32) / f32(W)) * f32(2) - f32(1)
    sy = (ys.astype(f32) / f32(H)) * f32(2) - f32(1)
    v = (fwd + right * sx[..., None]) + up * sy[..., None]
    flat = v.reshape(-1, 3)
    out = np.empty_like(flat)
    for i in range(flat.shape[0]):
        out[i] = po.normalize(flat[i])
    return out.reshape(v.shape)


def unorm16(x):
    """rtm_unorm(x, 65535) elementwise through the oracle (one call per distinct value)."""
    vals, inv = np.unique(np.ascontiguousarray(x, dtype=f32).view(np.uint32), return_inverse=True)
    q = np.array([po.unorm(v, 65535.0) for v in vals.view(f32)], dtype=np.uint16)
    return q[inv].reshape(x.shape)


class History:
    def __init__(self, width, height, cap=DEFAULT_CAP):
        self.W, self.H, self.cap = int(width), int(height), int(cap)
        self.valid = False
        self.frames = self.samples = 0      # rt_get_accumulation's pair
        self.mode = None                    # "restart" / "still" / "moved" of the last step
        self.diag = {}                      # moved frames: what steps 3-5 saw (for the contract tests)

    def reset(self):
        """A world or noise change, or rt_reset_accumulation: the next frame restarts."""
        self.valid = False

    def _classify(self, key):
        if not self.valid or key[0] != self.key[0]:
            return "restart"
        if key == self.key:
            return "still" if self.samples + 1 <= MAX_SAMPLES else "restart"
        return "moved"

    def step(self, planes, u):
        W, H = self.W, self.H
        key, cam = live_key(u), camera_of(u)
        L = planes["lighting_f32"][..., :3].astype(f32) * f32(16)
        nrm = planes["normal_r8"].astype(np.int64)
        dep = planes["depth_f32"].astype(f32)
        mode = self._classify(key)
        if mode == "restart":
            s = f32(0) + L
            n = np.ones((H, W), dtype=np.uint32)
            acc = np.zeros((H, W), dtype=bool)
            self.frames, self.samples = 1, 1
        elif mode == "still":
            s = self.sum + L
            n = self.n + np.uint32(1)
            acc = np.ones((H, W), dtype=bool)
            self.frames, self.samples = self.frames + 1, self.samples + 1
        else:
            s, n, acc = self._moved(cam, L, nrm, dep)
            self.frames, self.samples = self.frames + 1, min(self.samples, self.cap) + 1
        self.sum, self.n, self.nrm, self.dep = s.astype(f32), n.astype(np.uint32), nrm, dep
        self.key, self.cam, self.valid, self.mode = key, cam, True, mode
        light = np.empty((H, W, 4), dtype=f32)
        light[..., :3] = (self.sum / self.n.astype(f32)[..., None]) / f32(16)
        light[..., 3] = f32(1) / f32(16)
        return light, unorm16(light), self.n.copy(), acc

    def _moved(self, cam, L, nrm, dep):
        W, H, cap = self.W, self.H, self.cap
        o = cam[0]
        o1, f1, r1, u1 = self.cam
        ys, xs = np.mgrid[0:H, 0:W]
        with np.errstate(all="ignore"):
            hit = (nrm < 6) & (dep < f32(65535.0))                                   # 1
            t = dep / f32(32)                                                        # 2
            P = o + directions(cam, xs, ys, W, H) * t[..., None]
            v = P - o1                                                               # 3
            a = dotp(v, f1) / dotp(f1, f1)
            in_front = a > 0
            sx = (dotp(v, r1) / dotp(r1, r1)) / a
            sy = (dotp(v, u1) / dotp(u1, u1)) / a
            qx = np.floor(((sx + f32(1)) * f32(0.5)) * f32(W) + f32(0.5))            # 4
            qy = np.floor(((sy + f32(1)) * f32(0.5)) * f32(H) + f32(0.5))
            in_frame = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        ok = hit & in_front & in_frame
        qxi = np.where(ok, qx, 0).astype(np.int64)
        qyi = np.where(ok, qy, 0).astype(np.int64)
        same_face = ok & (self.nrm[qyi, qxi] == nrm) & (self.n[qyi, qxi] > 0)         # 5
        P1 = o1 + directions(self.cam, qxi, qyi, W, H) * (self.dep[qyi, qxi] / f32(32))[..., None]
        k = np.clip(nrm >> 1, 0, 2)[..., None]
        with np.errstate(all="ignore"):
            diff = np.abs(np.take_along_axis(P, k, 2)[..., 0] - np.take_along_axis(P1, k, 2)[..., 0])
        acc = same_face & (diff <= PLANE_TOLERANCE)
        c = self.n[qyi, qxi]                                                         # 6
        sp = self.sum[qyi, qxi]
        with np.errstate(all="ignore"):
            scaled = (sp / np.maximum(c, 1).astype(f32)[..., None]) * f32(cap)
        base = np.where((c <= cap)[..., None], sp, scaled)
        s = np.where(acc[..., None], base, f32(0)).astype(f32) + L
        n = np.where(acc, np.minimum(c, cap) + 1, 1).astype(np.uint32)
        self.diag = dict(hit=hit, in_front=in_front, in_frame=in_frame, qx=qxi, qy=qyi, same_face=same_face, plane_diff=diff,
                         accepted=acc)
        return s, n, acc


# ---- the camera paths the tests walk (the contract test checks on the CPU that the GPU tests' path exercises both branches) ------
SEED0 = 512 * 512 * 4 - 5          # RT_NOISE_BYTES - 5: every run of frames crosses the seed wrap
TERRAIN_BASE = (-30.0, -128.0, 100.0)
GPU_PATH_STEPS = (0, 1, 2, 3, 4, 4, 4, 5, 6, 7, 8, 9)   # pose index of frame k: two still frames in the middle


def path_uniforms(k, step=None, base=TERRAIN_BASE, dx=0.25, dh=0.002, heading=np.pi / 2, pitch=-0.02, sun=0.3, lr=(0, 0, 0),
                  seed0=SEED0):
    """Uniforms of frame k: pose `step` (default k) of a path that moves dx voxels along x and turns dh rad per step; the seed
    advances by one per FRAME (mod RT_NOISE_BYTES)."""
    j = k if step is None else step
    return po.camera_uniforms((base[0] + dx * j, base[1], base[2]), heading + dh * j, pitch, sun, (seed0 + k) % (512 * 512 * 4), lr)
