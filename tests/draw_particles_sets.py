"""Inputs of the particle tests: the record table the validity tests share (tests/test_draw_particles_contract.py judges it with the
restatement, tests/draw_particles_main.cpp with the host's own predicate), seeded clouds, and the adversarial set of the GPU test.
Test infrastructure; no GPU."""
import numpy as np

from raytrace_amd import abi, render

f32 = np.float32
TWO22 = 4194304.0
TABLE_LIGHTS = 5          # the light count the record table is judged under


def record_table():
    """(particles PARTICLE_DTYPE[N], expected bool[N], names): one record per rule of the valid particle and per edge of it."""
    nan, inf = float("nan"), float("inf")
    rows = [
        # name, centre, half, light, reserved, valid
        ("plain", (1.0, 2.0, 3.0), 0.0625, 0, 0, True),
        ("last light", (1.0, 2.0, 3.0), 0.0625, TABLE_LIGHTS - 1, 0, True),
        ("light == nlights", (1.0, 2.0, 3.0), 0.0625, TABLE_LIGHTS, 0, False),
        ("light far beyond", (1.0, 2.0, 3.0), 0.0625, 0xFFFFFFFF, 0, False),
        ("reserved != 0", (1.0, 2.0, 3.0), 0.0625, 0, 1, False),
        ("reserved high bit", (1.0, 2.0, 3.0), 0.0625, 0, 0x80000000, False),
        ("NaN centre x", (nan, 2.0, 3.0), 0.0625, 0, 0, False),
        ("NaN centre z", (1.0, 2.0, nan), 0.0625, 0, 0, False),
        ("infinite centre", (1.0, inf, 3.0), 0.0625, 0, 0, False),
        ("minus infinite centre", (1.0, -inf, 3.0), 0.0625, 0, 0, False),
        ("NaN half", (1.0, 2.0, 3.0), nan, 0, 0, False),
        ("infinite half", (1.0, 2.0, 3.0), inf, 0, 0, False),
        ("zero half", (1.0, 2.0, 3.0), 0.0, 0, 0, False),
        ("minus zero half", (1.0, 2.0, 3.0), -0.0, 0, 0, False),
        ("negative half", (1.0, 2.0, 3.0), -0.5, 0, 0, False),
        ("denormal half at the origin", (0.0, 0.0, 0.0), 1.0e-45, 0, 0, True),
        ("denormal half beside 1", (1.0, 0.0, 0.0), 1.0e-45, 0, 0, False),          # vanishes on x
        # at |centre| = 2^22 the spacing is 1/4 below and 1/2 above
        ("half 0.1 vanishes at 2^22", (TWO22, 0.0, 0.0), 0.1, 0, 0, False),          # lo and hi both round to 2^22
        ("half 0.25 at 2^22: hi rounds to even", (TWO22, 0.0, 0.0), 0.25, 0, 0, True),   # lo = 2^22 - 1/4, hi = 2^22
        ("half 0.5 at 2^22 leaves the domain", (TWO22, 0.0, 0.0), 0.5, 0, 0, False),  # hi = 2^22 + 1/2
        ("half 0.1 vanishes at -2^22", (0.0, -TWO22, 0.0), 0.1, 0, 0, False),
        ("half 0.25 at -2^22", (0.0, 0.0, -TWO22), 0.25, 0, 0, True),
        ("half 1/16 vanishes at 3e6", (3.0e6, 0.0, 0.0), 0.0625, 0, 0, False),        # spacing 1/4
        ("half 1/16 survives at 1e6", (1.0e6, 1.0e6, -1.0e6), 0.0625, 0, 0, True),    # spacing 1/16
        ("half 2^22 at the origin", (0.0, 0.0, 0.0), TWO22, 0, 0, True),
        ("half 2^22 + 1/2 at the origin", (0.0, 0.0, 0.0), TWO22 + 0.5, 0, 0, False),
        ("centre beyond 2^22", (TWO22 + 1.0, 0.0, 0.0), 0.5, 0, 0, False),
        ("centre 2^22 - 1, half 1", (TWO22 - 1.0, 0.0, 0.0), 1.0, 0, 0, True),
        ("huge finite centre", (3.0e38, 0.0, 0.0), 1.0, 0, 0, False),
        ("huge finite half", (0.0, 0.0, 0.0), 3.0e38, 0, 0, False),
    ]
    p = np.zeros(len(rows), dtype=abi.PARTICLE_DTYPE)
    for i, (_, c, h, light, reserved, _) in enumerate(rows):
        p["center"][i], p["half"][i], p["light"][i], p["reserved"][i] = c, h, light, reserved
    p["material"] = 0x12345 + np.arange(len(rows))
    p["emission"] = 0xFF000000
    return p, np.array([r[5] for r in rows]), [r[0] for r in rows]


def _basis(u):
    return (np.array(v[:], dtype=np.float64) for v in (u.origin, u.forward, u.right, u.up))


def cloud(u, n, seed, near=8.0, far=900.0, half=(0.03, 0.4), nlights=7):
    """n small cubes spread over (and a little beyond) the view at log-uniform distances — in front of the terrain and behind it —
    sharing `nlights` light records."""
    rng = np.random.default_rng(seed)
    o, f, r, up = _basis(u)
    sx, sy = rng.uniform(-1.05, 1.05, n), rng.uniform(-1.05, 1.05, n)
    v = f[None] + r[None] * sx[:, None] + up[None] * sy[:, None]
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    dist = np.exp(rng.uniform(np.log(near), np.log(far), n))
    c = o[None] + v * dist[:, None]
    h = rng.uniform(half[0], half[1], n) * np.maximum(1.0, dist / 60.0)      # the far ones larger, so that they still cover pixels
    return render.make_particles(c, h, rng.integers(0, 1 << 21, n), rng.integers(0, nlights, n), rng.integers(0, 1 << 32, n, dtype=np.uint64))


def some_lights(n, seed=9):
    """n light records: mostly what probes return (0 .. 20), with a zero, a value that saturates the UNORM16 plane, a negative and a huge one."""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, dtype=render.PROBE_LIGHT_DTYPE)
    out["light"] = rng.random((n, 3), dtype=np.float32) * f32(20.0)
    if n > 4:
        out["light"][1] = 0.0
        out["light"][2, 1] = 400.0
        out["light"][3, 2] = -2.5
        out["light"][4, 0] = 1.0e30
    out["sun_samples"] = rng.integers(0, 5, n)
    return out


def pixel_point(u, width, height, px, py, dist):
    """The point `dist` along the exact direction of pixel (px, py)'s ray (float64 of the float32 direction)."""
    from tests import draw_boxes_ref
    d = draw_boxes_ref.directions(u, width, height)[py, px].astype(np.float64)
    return np.array(u.origin[:], dtype=np.float64) + d * dist


def adversarial(u, width, height):
    """(particles, nlights, notes) for a camera that looks along +y with right = +x and up = +z (the GPU test's _axis_u)."""
    o = np.array(u.origin[:], dtype=np.float64)
    rows = []   # (centre, half, light, reserved)

    def add(c, h, light=0, reserved=0):
        rows.append((tuple(float(x) for x in c), float(h), light, reserved))
        return len(rows) - 1

    notes = {}
    # a size sweep at a fixed distance, dead ahead and off axis: under a pixel to beyond the frame (the frame is 0.8 wide at distance 1)
    dist = 40.0
    notes["sweep"] = [add(o + (0.0 if k % 2 == 0 else 3.0 + k, dist + 3.0 * k, 0.0 if k % 2 == 0 else -2.0), h, k % 3)
                      for k, h in enumerate((0.004, 0.02, 0.1, 0.2, 0.45, 0.9, 1.8, 2.4, 3.5, 5.0))]
    # ... and behind them three that cover a few tiles, half the frame and all of it
    notes["sweep"] += [add(o + (-20.0, 100.0, 8.0), 9.0, 1), add(o + (0.0, 125.0, 0.0), 25.0, 2), add(o + (0.0, 450.0, 0.0), 200.0, 0)]
    # faces exactly on the rays of tile-boundary pixels: a cube whose low x face and low z face pass through the point on pixel
    # (8 i, 8 j)'s ray at its own depth
    notes["boundary"] = []
    for (px, py) in ((8, 8), (16, 24), (32, 16), (40, 32), (56, 8), (24, 24)):
        if px < width and py < height:
            q = pixel_point(u, width, height, px, py, 30.0)
            h = 0.25
            notes["boundary"].append(add((f32(q[0]) + f32(h), q[1], f32(q[2]) + f32(h)), h, 1))
            notes["boundary"].append(add((f32(q[0]) - f32(h), q[1], f32(q[2]) - f32(h)), h, 2))
    notes["behind"] = add(o + (0.0, -30.0, 0.0), 1.0)
    notes["straddle"] = add(o + (-1.2, 0.5, -0.5), 1.0)                 # crosses the camera plane, off axis
    notes["inside"] = add(o + (0.1, 0.1, -0.1), 0.8)                    # the camera inside the cube
    notes["on_face"] = add(o + (0.0, 1.0, 0.0), 1.0)                    # the camera on a face: t_in == 0
    notes["behind_terrain"] = add(o + (50.0, 305.0, -112.0), 6.0)
    notes["partly_behind_terrain"] = add(o + (0.0, 205.0, -65.0), 20.0)
    notes["over_sky"] = add(o + (-5.0, 43.0, 12.0), 2.0)
    notes["too_far"] = add(o + (0.0, 3000.0, 0.0), 30.0)                # beyond the sky's depth: never drawn
    notes["at_2^22"] = [add((o[0] + 14.0, o[1] + 60.0, TWO22 - 8.0), 8.0), add((-TWO22 + 16.0, o[1] + 100.0, o[2] + 20.0), 16.0),
                        add((0.0, 0.0, 0.0), TWO22)]                    # ... and the cube that fills the domain (the camera is inside)
    # exact duplicates with different materials: the lowest index shows
    notes["duplicates"] = [add(o + (6.0, 31.0, -7.0), 1.0, 3), add(o + (6.0, 31.0, -7.0), 1.0, 4), add(o + (6.0, 31.0, -7.0), 1.0, 5)]
    # ... and equal entry faces (the same low y face) with different extents beside each other
    notes["coplanar"] = [add(o + (-6.0, 36.0, 4.0), 2.0, 1), add(o + (-5.0, 35.0, 5.0), 1.0, 2)]
    # invalid records between the valid ones
    notes["invalid"] = [add((np.nan, 0.0, 0.0), 1.0), add(o + (0.0, 20.0, 0.0), 0.0), add(o + (0.0, 20.0, 0.0), -1.0),
                        add(o + (0.0, 20.0, 0.0), 1.0, light=6), add(o + (0.0, 20.0, 0.0), 1.0, reserved=7), add((TWO22, 0.0, 0.0), 0.1),
                        add(o + (0.0, 20.0, 0.0), np.inf)]
    notes["after_invalid"] = add(o + (-3.0, 25.0, -3.0), 0.7, 5)
    p = np.zeros(len(rows), dtype=abi.PARTICLE_DTYPE)
    for i, (c, h, light, reserved) in enumerate(rows):
        p["center"][i], p["half"][i], p["light"][i], p["reserved"][i] = c, h, light, reserved
    p["material"] = (np.arange(len(rows)) * 0x1234F + 0x7F) & 0x1FFFFF
    p["emission"] = 0xFF000000 + np.arange(len(rows))
    # interleave: move the invalid records apart
    order = list(range(len(rows)))
    for k, i in enumerate(notes["invalid"]):
        order.remove(i)
        order.insert(3 + 5 * k, i)
    where = {old: new for new, old in enumerate(order)}
    remap = lambda v: [where[i] for i in v] if isinstance(v, list) else where[v]
    return p[order], 6, {k: remap(v) for k, v in notes.items()}
