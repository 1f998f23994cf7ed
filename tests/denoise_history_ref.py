"""The history-aware denoise (rt_denoise_history / rt_denoise_planes_counted; include/rt_abi.h, DESIGN.md "History-aware denoise")
restated in numpy float32.  With neutral parameters it is the oracle's six bilateral_denoise.comp dispatches bit for bit
(tests/test_denoise_history_contract.py anchors it there), so what it says with counts is the contract's arithmetic and nothing else.

The contract, dispatch i of sizes (1, 2, 4, 8, 8, 16), m(p) = min(max(count(p), 1), 127):
  * the dispatch is rt_denoise's: same tap spacing; on odd dispatches of a `faithful` run the depth binding reads the normal plane and
    the normal binding the depth plane;
  * settle: settle[i] != 0 and m(p) >= settle[i] -> p takes the copy branch (value and computed flag unchanged), whatever its normal
    binding says; its neighbours still read it as a tap;
  * weight_by_count: total_weight starts from 0.146634f * float(m(c)), sum from L_c * total_weight, and a tap's weight is the
    quotient weight / (distance_difference + normal_difference + 1) times float(m(tap)) — one fp32 multiply behind the division;
  * sums by fp32 fma in tap order, sum / total_weight stored as UNORM16 between dispatches; alpha is 65535 once any dispatch filtered
    the pixel, else the input texel's.

Every operation is a float32 array operation rounded on its own.  fp32 fma is emulated: the product of two floats is exact in
float64, the float64 sum is turned into a round-to-odd sum with TwoSum's error term, and the cast to float32 then rounds once."""
import numpy as np

f32 = np.float32
f64 = np.float64
SIZES = (1, 2, 4, 8, 8, 16)
NEUTRAL = (0, 0, 0, 0, 0, 0)
TAPS = ((0, 1, 0.092566), (0, -1, 0.092566), (1, 0, 0.092566), (-1, 0, 0.092566),
        (1, 1, 0.058434), (-1, 1, 0.058434), (-1, -1, 0.058434), (1, -1, 0.058434),
        (2, 0, 0.023205), (-2, 0, 0.023205), (0, 2, 0.023205), (0, -2, 0.023205),
        (2, 2, 0.003672), (-2, 2, 0.003672), (-2, -2, 0.003672), (2, -2, 0.003672),
        (2, 1, 0.014648), (-2, 1, 0.014648), (-2, -1, 0.014648), (2, -1, 0.014648),
        (1, 2, 0.014648), (-1, 2, 0.014648), (-1, -2, 0.014648), (1, -2, 0.014648),
        (3, 0, 0.002289), (-3, 0, 0.002289), (0, 3, 0.002289), (0, -3, 0.002289),
        (3, 1, 0.001445), (-3, 1, 0.001445), (-3, -1, 0.001445), (3, -1, 0.001445),
        (1, 3, 0.001445), (-1, 3, 0.001445), (-1, -3, 0.001445), (1, -3, 0.001445))


def fma(a, b, c):
    """fl32(a * b + c) of float32 arrays."""
    p = a.astype(f64) * b.astype(f64)            # exact: 24 + 24 bits
    c = c.astype(f64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)              # TwoSum: p + c = s + err exactly
    bits = s.view(np.int64)
    inexact = (err != 0) & ((bits & 1) == 0)
    toward = np.where((err > 0) == (s > 0), 1, -1)   # one ulp away from zero if err has s's sign, else towards it
    return np.where(inexact, bits + toward, bits).view(f64).astype(f32)


def unorm16(x):
    """rtm_unorm(x, 65535): 0 for x <= 0 (and NaN), floor(min(x, 1) * 65535 + 0.5) otherwise, each operation in float32."""
    x = x.astype(f32)
    q = np.floor(np.minimum(x, f32(1)) * f32(65535) + f32(0.5))
    return np.where(x > 0, q, 0).astype(np.uint32)


def clamp_counts(counts):
    """m(p)."""
    return np.clip(np.asarray(counts).astype(np.int64), 1, 127)


def start(lighting_rgba16):
    """The working state in front of dispatch 0: (value float32[H, W, 3], computed bool[H, W])."""
    light = np.asarray(lighting_rgba16)
    return light[..., :3].astype(f32) / f32(65535), np.zeros(light.shape[:2], dtype=bool)


def dispatch(value, computed, depth, normal, size, swapped=False, m=None, weight_by_count=False, settle=0):
    """One dispatch on the working state; returns the new (value, computed).  `m` = clamp_counts(counts), or None for no counts."""
    H, W = depth.shape
    yy, xx = np.mgrid[0:H, 0:W]
    b1 = (normal if swapped else depth).astype(f32)              # what the shader's depth binding returns
    b2 = (depth if swapped else normal).astype(np.int64)         # ... and its normal binding
    cd = b1 / f32(256)
    tw = np.full((H, W), f32(0.146634))
    if weight_by_count:
        tw = tw * m.astype(f32)
    s = value * tw[..., None]
    for dx, dy, w in TAPS:
        sx = np.clip(xx + dx * size, 0, W - 1)
        sy = np.clip(yy + dy * size, 0, H - 1)
        dd = f32(4) * np.abs(cd - b1[sy, sx] / f32(256))
        nd = np.where(b2[sy, sx] == b2, f32(0), f32(10))
        wt = (f32(w) / ((dd + nd) + f32(1))).astype(f32)
        if weight_by_count:
            wt = wt * m[sy, sx].astype(f32)
        tw = tw + wt
        s = fma(value[sy, sx], wt[..., None], s)
    q = unorm16(s / tw[..., None])
    filt = b2 < 16
    if settle:
        filt = filt & ~(m >= settle)
    return np.where(filt[..., None], q.astype(f32) / f32(65535), value), computed | filt


def finish(value, computed, lighting_rgba16):
    """The RGBA16 plane the sixth dispatch stores."""
    light = np.asarray(lighting_rgba16)
    out = np.empty(light.shape, dtype=np.uint16)
    out[..., :3] = unorm16(value)
    out[..., 3] = np.where(computed, 65535, light[..., 3])
    return out


def denoise(lighting_rgba16, depth_r16, normal_r8, faithful=True, counts=None, weight_by_count=False, settle=NEUTRAL):
    """uint16[H, W, 4]: what rt_denoise_planes_counted leaves in the lighting plane.  counts None: rt_denoise_planes (neutral
    parameters only)."""
    depth, normal = np.asarray(depth_r16), np.asarray(normal_r8)
    if counts is None:
        assert not weight_by_count and not any(settle)
        m = None
    else:
        m = clamp_counts(counts)
    value, computed = start(lighting_rgba16)
    for i, size in enumerate(SIZES):
        value, computed = dispatch(value, computed, depth, normal, size, bool(faithful) and i % 2 == 1, m, weight_by_count, int(settle[i]))
    return finish(value, computed, lighting_rgba16)


def random_planes(h, w, seed=3):
    """Random planes with what a rendered frame need not hold: a patch with depth < 16 (the pong dispatches of a faithful run then
    filter something) and sky rows (normal 16, depth 0xFFFF) at the top."""
    rng = np.random.default_rng(seed)
    lighting = rng.integers(0, 20000, size=(h, w, 4), dtype=np.uint16)
    lighting[..., 3] = 4096
    depth = rng.integers(100, 4000, size=(h, w), dtype=np.uint16)
    normal = rng.integers(0, 6, size=(h, w), dtype=np.uint8)
    depth[:5, :7] = rng.integers(0, 20, size=(5, 7))
    normal[-6:] = 16
    depth[-6:] = 0xFFFF
    return lighting, depth, normal


EDGE_COUNTS = (0, 1, 2, 7, 8, 126, 127, 128, 1 << 24, (1 << 27) - 1)


def edge_counts(h, w, seed=11):
    """Counts drawn from the values round every clamp and threshold."""
    rng = np.random.default_rng(seed)
    return np.array(EDGE_COUNTS, dtype=np.uint32)[rng.integers(0, len(EDGE_COUNTS), size=(h, w))]


def random_counts(h, w, seed=12):
    return np.random.default_rng(seed).integers(0, 201, size=(h, w)).astype(np.uint32)


# ---- the quality measurement (DESIGN.md "History-aware denoise", the table) --------------------------------------------------------
QUALITY_W, QUALITY_H, QUALITY_FRAMES, QUALITY_DEPTH = 96, 64, 24, 2
QUALITY_TRUTH_SPP, QUALITY_TRUTH_SEED = 256, 100
_quality = {}


def quality_camera(k, seed):
    from oracle import pyoracle as po
    return po.camera_uniforms((-30.0 + 0.15 * k, -128.0, 100.0), np.pi / 2 + 0.002 * k, -0.1, 0.3, seed)


def quality_scene(world, noise):
    """24 one-sample oracle frames of a slowly moving camera fed through temporal_ref.History, and the last camera's frame at
    QUALITY_TRUTH_SPP samples: dict(lighting uint16[H, W, 4], depth, normal, counts, truth float64[H, W, 3]).  Computed once."""
    if "scene" not in _quality:
        from oracle import pyoracle as po
        from tests import temporal_ref as tr
        mats, mine = world
        W, H = QUALITY_W, QUALITY_H
        h = tr.History(W, H)
        for k in range(QUALITY_FRAMES):
            u = quality_camera(k, 5 + k)
            planes, _ = po.render(mats, mine, noise, u, W, H, 1, QUALITY_DEPTH)
            _, l16, counts, _ = h.step(planes, u)
        truth, _ = po.render(mats, mine, noise, quality_camera(QUALITY_FRAMES - 1, QUALITY_TRUTH_SEED), W, H, QUALITY_TRUTH_SPP, QUALITY_DEPTH)
        _quality["scene"] = dict(lighting=l16, depth=planes["depth_r16"], normal=planes["normal_r8"], counts=counts,
                                 truth=truth["lighting_f32"][..., :3].astype(f64))
        for a in _quality["scene"].values():
            a.setflags(write=False)
    return _quality["scene"]


def rms_errors(image_rgba16, scene):
    """RMS of image / 65535 - truth over (all surface pixels, those with counts >= 8, those with counts <= 2)."""
    surface = scene["normal"] < 16
    e = np.asarray(image_rgba16)[..., :3].astype(f64) / 65535.0 - scene["truth"]
    rms = lambda mask: float(np.sqrt((e[mask] ** 2).mean()))
    return rms(surface), rms(surface & (scene["counts"] >= 8)), rms(surface & (scene["counts"] <= 2))
