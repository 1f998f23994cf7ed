"""Restatement of the box-sweep rules (include/rt_abi.h "Box sweeps", DESIGN.md "Box sweeps") for the sweep tests: scalar numpy
float32, one rounding per operation, integers once the event times are known.  Written from the rules and not from the kernel.
Test infrastructure; Python loops, meant for a few thousand sweeps.

A world is an `Occupancy`: which world voxels are occupied under (materials, minefield, lr, R)."""
import numpy as np

f32 = np.float32
FREE, BLOCKED, EMBEDDED, INVALID = 0, 1, 2, 3
MAX_COORD = f32(4194304.0)   # 2^22
MAX_EXTENT = f32(8.0)
MAX_MOTION = f32(64.0)
NO_TEXEL = (-1, -1, -1)

# numpy view of RtSweepHit, declared here a second time on purpose (the binding's own is raytrace_amd.render.SWEEP_HIT_DTYPE)
HIT_DTYPE = np.dtype([("t", "<f4"), ("kind", "<u4"), ("normal", "<u4"), ("material", "<u4"), ("texel", "<i4", 3), ("axis", "<u4"),
                      ("lo", "<f4", 3), ("reserved0", "<u4"), ("hi", "<f4", 3), ("reserved1", "<u4")])
assert HIT_DTYPE.itemsize == 64


class Occupancy:
    """World voxel v (the cell [v, v + 1) per axis) is occupied iff lr - R/2 <= v < lr + R/2 on every axis and the minefield byte at
    texel (v + R/2) mod R is 0.  Arrays are [z, y, x] in texel order."""

    def __init__(self, materials, minefield, lr=(0, 0, 0), R=256):
        self.R = int(R)
        self.materials = np.asarray(materials).reshape(R, R, R)
        self.minefield = np.asarray(minefield).reshape(R, R, R)
        self.lr = tuple(int(v) for v in lr)

    def texel(self, v):
        """The texel of world voxel v (x, y, z), or None outside the window."""
        h = self.R // 2
        for a in range(3):
            if not (self.lr[a] - h <= v[a] < self.lr[a] + h):
                return None
        return tuple((int(v[a]) + h) % self.R for a in range(3))

    def occupied(self, v):
        t = self.texel(v)
        return t is not None and self.minefield[t[2], t[1], t[0]] == 0

    def first_occupied(self, cx, cy, cz):
        """The first occupied voxel of the closed integer ranges cx x cy x cz in ascending (z, y, x) order: (texel, material) or None."""
        for z in range(cz[0], cz[1] + 1):
            for y in range(cy[0], cy[1] + 1):
                for x in range(cx[0], cx[1] + 1):
                    t = self.texel((x, y, z))
                    if t is not None and self.minefield[t[2], t[1], t[0]] == 0:
                        return t, int(self.materials[t[2], t[1], t[0]])
        return None

    def solid_world_voxels(self):
        """int64[N, 3] world coordinates (x, y, z) of every occupied voxel of the window."""
        z, y, x = np.nonzero(self.minefield == 0)
        t = np.stack([x, y, z], 1).astype(np.int64)
        lr = np.asarray(self.lr, dtype=np.int64)
        return lr - self.R // 2 + (t - lr) % self.R


def in_domain(lo, hi, motion):
    """The validated domain: every float finite, |lo|, |hi| <= 2^22, per axis 0 < hi - lo <= 8 (the fp32 difference), |motion| <= 64
    per component."""
    with np.errstate(all="ignore"):
        for a in range(3):
            l, h, m = f32(lo[a]), f32(hi[a]), f32(motion[a])
            if not (np.isfinite(l) and np.isfinite(h) and np.isfinite(m)):
                return False
            if np.abs(l) > MAX_COORD or np.abs(h) > MAX_COORD or np.abs(m) > MAX_MOTION:
                return False
            e = f32(h - l)
            if not (e > 0 and e <= MAX_EXTENT):
                return False
    return True


def _floor(x):
    return int(np.floor(x))


def _ceil(x):
    return int(np.ceil(x))


def _max(x, c):
    """The clamp of the returned box: x unless it is below float(c)."""
    c = f32(c)
    return c if x < c else x


def _min(x, c):
    c = f32(c)
    return c if x > c else x


def _hit(kind, t, normal, material, texel, axis, lo, hi):
    return {"t": f32(t), "kind": kind, "normal": normal, "material": material, "texel": tuple(texel), "axis": axis,
            "lo": [f32(v) for v in lo], "hi": [f32(v) for v in hi]}


def sweep(occ, lo, hi, motion):
    """One sweep against `occ`; a dict with the fields of RtSweepHit."""
    lo = [f32(v) for v in lo]
    hi = [f32(v) for v in hi]
    m = [f32(v) for v in motion]
    if not in_domain(lo, hi, m):
        return _hit(INVALID, 0.0, 6, 0, NO_TEXEL, 3, lo, hi)
    with np.errstate(all="ignore"):
        c = [[_floor(lo[a]), _ceil(hi[a]) - 1] for a in range(3)]
        found = occ.first_occupied(c[0], c[1], c[2])
        if found:
            return _hit(EMBEDDED, 0.0, 6, found[1], found[0], 3, lo, hi)

        # one pending plane per (axis, trailing / leading): [plane g, time t]; None when the sequence has no event below t = 1
        def time_of(g, face, a):
            return f32(f32(f32(g) - face) / m[a])

        seq = {}
        for a in range(3):
            if m[a] == 0:
                continue
            if m[a] > 0:
                lead, trail = (_ceil(hi[a]), hi[a]), (_floor(lo[a]) + 1, lo[a])
            else:
                lead, trail = (_floor(lo[a]), lo[a]), (_ceil(hi[a]) - 1, hi[a])
            seq[(0, a)] = [trail[0], time_of(trail[0], trail[1], a), trail[1]]   # kind 0 = trailing: goes first at equal t
            seq[(1, a)] = [lead[0], time_of(lead[0], lead[1], a), lead[1]]

        def returned_box(t, blocked_axis=None, g=None):
            rl, rh = [None] * 3, [None] * 3
            for a in range(3):
                if m[a] == 0:               # an axis that does not move returns its input, bit for bit
                    rl[a], rh[a] = lo[a], hi[a]
                    continue
                rl[a] = _max(f32(lo[a] + f32(m[a] * t)), c[a][0])
                rh[a] = _min(f32(hi[a] + f32(m[a] * t)), c[a][1] + 1)
            if blocked_axis is not None:
                a = blocked_axis
                size = f32(hi[a] - lo[a])
                if m[a] > 0:
                    rh[a] = f32(g)
                    rl[a] = _max(f32(f32(g) - size), c[a][0])
                else:
                    rl[a] = f32(g)
                    rh[a] = _min(f32(f32(g) + size), c[a][1] + 1)
            return rl, rh

        while True:
            best = None
            for key in sorted(seq):            # (kind, axis) ascending: the tie order at equal t
                s = seq[key]
                if not (s[1] < 1):
                    continue
                if best is None or s[1] < seq[best][1]:
                    best = key
            if best is None:
                rl, rh = returned_box(f32(1.0))
                return _hit(FREE, 1.0, 6, 0, NO_TEXEL, 3, rl, rh)
            kind, a = best
            g, t, face = seq[best]
            up = m[a] > 0
            if kind == 0:
                if up:
                    c[a][0] = g
                else:
                    c[a][1] = g - 1
            else:
                layer = g if up else g - 1
                r = [list(c[0]), list(c[1]), list(c[2])]
                r[a] = [layer, layer]
                found = occ.first_occupied(r[0], r[1], r[2])
                if found:
                    rl, rh = returned_box(t, a, g)
                    return _hit(BLOCKED, t, 2 * a + (1 if up else 0), found[1], found[0], a, rl, rh)
                if up:
                    c[a][1] = layer
                else:
                    c[a][0] = layer
            g2 = g + 1 if up else g - 1
            seq[best] = [g2, time_of(g2, face, a), face]


def pack(hits):
    """A list of sweep() results -> HIT_DTYPE[N], byte for byte what the library's hit records hold."""
    out = np.zeros(len(hits), dtype=HIT_DTYPE)
    for i, h in enumerate(hits):
        out[i]["t"], out[i]["kind"], out[i]["normal"], out[i]["material"] = h["t"], h["kind"], h["normal"], h["material"]
        out[i]["texel"], out[i]["axis"] = h["texel"], h["axis"]
        out[i]["lo"], out[i]["hi"] = h["lo"], h["hi"]
    return out


def sweep_batch(occ, sweeps):
    """float32[N, 3, 3] (lo, hi, motion per row) -> HIT_DTYPE[N]."""
    sweeps = np.asarray(sweeps, dtype=np.float32).reshape(-1, 3, 3)
    return pack([sweep(occ, s[0], s[1], s[2]) for s in sweeps])


def move_and_slide(occ, lo, hi, motion, iterations=3):
    """The character-controller loop: sweep; on BLOCKED take the returned box, zero the blocked axis of motion * (1 - t) and sweep
    again; stop on FREE, on EMBEDDED / INVALID, on a zero remainder or after `iterations` sweeps.  Returns (lo, hi, hits)."""
    lo = [f32(v) for v in lo]
    hi = [f32(v) for v in hi]
    m = [f32(v) for v in motion]
    hits = []
    for _ in range(int(iterations)):
        h = sweep(occ, lo, hi, m)
        hits.append(h)
        if h["kind"] in (EMBEDDED, INVALID):
            break
        lo, hi = h["lo"], h["hi"]
        if h["kind"] == FREE:
            break
        rest = f32(f32(1.0) - h["t"])
        m = [f32(v * rest) for v in m]
        m[h["axis"]] = f32(0.0)
        if all(v == 0 for v in m):
            break
    return lo, hi, hits
