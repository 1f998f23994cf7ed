"""Inputs of the particle-simulation tests, built from the world they run on: boxes a fraction of a voxel above, beside and below
occupied voxels found by Occupancy.solid_world_voxels, with velocities aimed at faces, edges and corners; particles resting on a
floor; particles in open air; particles that straddle the seam of a scrolled window; and the table of invalid and inactive records
that the validity tests share (tests/test_particle_step_contract.py judges it with the restatement, tests/particle_step_main.cpp
with the host's own predicate).  What a set holds is asserted from the restatement by `census`.  Test infrastructure; no GPU."""
import numpy as np

from tests import particle_step_ref as ref
from tests import sweep_ref

f32 = np.float32
TWO22 = 4194304.0
DT = 1.0 / 16.0
GRAVITY = (0.0, 0.0, -32.0)


def state(lo, hi, velocity=(0, 0, 0), response=ref.SLIDE, life=np.inf, half=0.0625, flags=0, material=0x00C0FFEE, emission=0xFF000000, light=0,
          reserved=0):
    s = np.zeros(1, dtype=ref.STATE_DTYPE)[0]
    s["lo"], s["hi"], s["velocity"], s["life"], s["half"] = lo, hi, velocity, life, half
    s["flags"], s["material"], s["emission"], s["light"], s["reserved"] = int(response) | int(flags), material, emission, light, reserved
    return s


# ---- the table of invalid and inactive records ------------------------------------------------------------------------------------
def record_table():
    """(states STATE_DTYPE[N], verdict[N], names): verdict 'valid', 'invalid' or 'inactive' per record — one per rule of the valid
    record and per edge of it.  A NaN here is the canonical quiet one and sits alone on its axis (the draw record's centre of such a
    record is then the same NaN on every machine)."""
    nan, inf = float("nan"), float("inf")
    lo, hi = (1.0, 2.0, 3.0), (1.25, 2.25, 3.25)
    rows = [
        ("plain", state(lo, hi, (1, -2, 3)), "valid"),
        ("lives for ever", state(lo, hi, life=inf), "valid"),
        ("negative life (dies this tick)", state(lo, hi, life=-1.0), "valid"),
        ("input contact bits are ignored", state(lo, hi, flags=ref.CONTACT), "valid"),
        ("every response", state(lo, hi, response=ref.BOUNCE), "valid"),
        ("extent exactly 8", state((0, 0, 0), (8, 1, 1)), "valid"),
        ("box at 2^22", state((TWO22 - 1, 0, 0), (TWO22, 1, 1)), "valid"),
        ("half differs from the box", state(lo, hi, half=3.0), "valid"),
        ("denormal half", state(lo, hi, half=1.0e-45), "valid"),
        ("NaN lo", state((nan, 2.0, 3.0), hi), "invalid"),
        ("NaN hi", state(lo, (1.25, 2.25, nan)), "invalid"),
        ("infinite lo", state((1.0, -inf, 3.0), hi), "invalid"),
        ("infinite hi", state(lo, (1.25, inf, 3.25)), "invalid"),
        ("lo == hi", state(lo, (1.25, 2.0, 3.25)), "invalid"),
        ("lo above hi", state(lo, (0.5, 2.25, 3.25)), "invalid"),
        ("extent above 8", state((0, 0, 0), (1, 8.5, 1)), "invalid"),
        ("coordinate beyond 2^22", state((TWO22, 0, 0), (TWO22 + 1, 1, 1)), "invalid"),
        ("NaN velocity", state(lo, hi, (0, nan, 0)), "invalid"),
        ("infinite velocity", state(lo, hi, (inf, 0, 0)), "invalid"),
        ("huge finite velocity", state(lo, hi, (3.0e38, -3.0e38, 0)), "valid"),
        ("NaN life", state(lo, hi, life=nan), "invalid"),
        ("minus infinite life", state(lo, hi, life=-inf), "invalid"),
        ("zero half", state(lo, hi, half=0.0), "invalid"),
        ("negative half", state(lo, hi, half=-0.5), "invalid"),
        ("NaN half", state(lo, hi, half=nan), "invalid"),
        ("infinite half", state(lo, hi, half=inf), "invalid"),
        ("reserved != 0", state(lo, hi, reserved=1), "invalid"),
        ("unknown flag bit 2", state(lo, hi, flags=0x4), "invalid"),
        ("unknown flag bit 31", state(lo, hi, flags=0x80000000), "invalid"),
        ("unknown flag beside contact", state(lo, hi, flags=0x80000), "invalid"),
        ("dead", state(lo, hi, (1, 2, 3), flags=ref.DEAD), "inactive"),
        ("dead with garbage", state((nan, 2.0, 3.0), (0.0, inf, 3.25), (0, nan, 0), flags=ref.DEAD | 0x4000, half=-1.0, reserved=7), "inactive"),
        ("marked invalid", state(lo, hi, flags=ref.INVALID | ref.CONTACT), "inactive"),
        ("dead and invalid", state(lo, hi, flags=ref.INVALID | ref.DEAD, life=-3.0), "inactive"),
    ]
    states = np.array([r[1] for r in rows], dtype=ref.STATE_DTYPE)
    states["material"] = 0x12345 + np.arange(len(rows))
    states["light"] = np.arange(len(rows)) % 5
    return states, [r[2] for r in rows], [r[0] for r in rows]


def params_table():
    """[(name, kwargs of ref.Params / render.make_particle_step, valid)]: one row per rule of the call parameters and per edge."""
    nan, inf = float("nan"), float("inf")
    base = dict(dt=DT, accel=GRAVITY, damping=1.0, restitution=0.5, friction=0.75, rest_speed=0.25, sweeps=3)
    rows = [("plain", {}, True), ("dt 1", dict(dt=1.0), True), ("dt 0", dict(dt=0.0), False), ("dt negative", dict(dt=-0.1), False),
            ("dt above 1", dict(dt=1.0001), False), ("dt NaN", dict(dt=nan), False), ("dt infinite", dict(dt=inf), False),
            ("accel 4096", dict(accel=(4096.0, -4096.0, 0.0)), True), ("accel beyond", dict(accel=(0.0, 4097.0, 0.0)), False),
            ("accel NaN", dict(accel=(0.0, 0.0, nan)), False), ("accel infinite", dict(accel=(-inf, 0.0, 0.0)), False),
            ("damping 0", dict(damping=0.0), True), ("damping above 1", dict(damping=1.5), False), ("damping negative", dict(damping=-0.1), False),
            ("damping NaN", dict(damping=nan), False), ("restitution 1", dict(restitution=1.0), True), ("restitution above 1", dict(restitution=1.01), False),
            ("restitution NaN", dict(restitution=nan), False), ("friction 0", dict(friction=0.0), True), ("friction above 1", dict(friction=2.0), False),
            ("friction negative", dict(friction=-1.0), False), ("rest_speed 0", dict(rest_speed=0.0), True), ("rest_speed negative", dict(rest_speed=-1.0), False),
            ("rest_speed infinite", dict(rest_speed=inf), False), ("rest_speed NaN", dict(rest_speed=nan), False), ("sweeps 1", dict(sweeps=1), True),
            ("sweeps 4", dict(sweeps=4), True), ("sweeps 0", dict(sweeps=0), False), ("sweeps 5", dict(sweeps=5), False)]
    return [(name, dict(base, **kw), ok) for name, kw, ok in rows]


# ---- sets built from the world -----------------------------------------------------------------------------------------------------
def seam_planes(occ):
    """Per axis the world plane inside the window at which the texel coordinate wraps from R - 1 to 0 (the window's own low edge when
    lr is 0 on that axis)."""
    return [occ.lr[a] - occ.R // 2 + (-occ.lr[a]) % occ.R for a in range(3)]


def _free(occ, lo, hi):
    c = [[int(np.floor(f32(lo[a]))), int(np.ceil(f32(hi[a]))) - 1] for a in range(3)]
    return occ.first_occupied(c[0], c[1], c[2]) is None


def world_set(occ, seed, per=10, speed=12.0):
    """(states, kinds): STATE_DTYPE[N] active valid particles placed from the occupied voxels of `occ`, and the kind each was placed as
    — 'face a+' / 'face a-' (a fraction of a voxel off a face of an occupied voxel, moving at it along axis a), 'edge', 'corner' (moving
    at it along two and three axes), 'rest' (standing on a voxel's top, no velocity), 'air' (no occupied voxel within reach), 'seam'
    (the box straddles a seam plane), 'floor' (below the window, moving up into its lowest layer) and 'dying' (life runs out this
    tick).  Responses go round.  What happens to them is the restatement's to say (census)."""
    rng = np.random.default_rng(seed)
    solid = occ.solid_world_voxels()
    solid = solid[rng.permutation(len(solid))[:4000]]
    out, kinds = [], []
    size = lambda: f32(rng.choice([0.125, 0.25, 0.375, 0.5]))

    def add(kind, lo, hi, vel, **kw):
        lo, hi = np.float32(lo), np.float32(hi)
        if not _free(occ, lo, hi):
            return False
        out.append(state(lo, hi, np.float32(vel), response=len(out) % 4, half=f32(hi[0] - lo[0]) * f32(0.5), material=0x00A00000 + len(out),
                         light=len(out) % 3, **kw))
        kinds.append(kind)
        return True

    def beside(v, axis, sign, s, gap):
        """A box of edge s in the cell beside voxel v on side `sign` of `axis`, `gap` off its face."""
        lo = v.astype(np.float64) + rng.uniform(0.0, 1.0 - float(s), 3)
        lo[axis] = v[axis] + 1 + gap if sign > 0 else v[axis] - gap - float(s)
        return lo, lo + float(s)

    want = {}
    for v in solid:
        for axis in range(3):
            for sign in (1, -1):
                n = v.copy()
                n[axis] += sign
                if occ.occupied(n):
                    continue
                s, gap = size(), rng.uniform(0.01, 0.4)
                lo, hi = beside(v, axis, sign, s, gap)
                name = "face %s%s" % ("xyz"[axis], "-" if sign > 0 else "+")     # the direction of travel
                vel = np.zeros(3)
                vel[axis] = -sign * speed
                if want.get(name, 0) < per and add(name, lo, hi, vel):
                    want[name] = want.get(name, 0) + 1
                # an edge and a corner: the same start, moving along two and three axes
                for kind, others in (("edge", 1), ("corner", 2)):
                    if want.get(kind, 0) < 3 * per:
                        vel2 = vel.copy()
                        for o in rng.permutation([a for a in range(3) if a != axis])[:others]:
                            vel2[o] = rng.choice([-1, 1]) * speed * rng.uniform(0.5, 1.5)
                        if add(kind, lo, hi, vel2):
                            want[kind] = want.get(kind, 0) + 1
                if axis == 2 and sign > 0 and want.get("rest", 0) < 3 * per:          # standing on the voxel's top
                    lo, hi = beside(v, 2, 1, s, 0.0)
                    if add("rest", lo, hi, (0, 0, 0)):
                        want["rest"] = want.get("rest", 0) + 1
                if want.get("dying", 0) < per:
                    if add("dying", *beside(v, axis, sign, s, 0.45), vel * 0.01, life=DT * rng.choice([0.5, 1.0])):
                        want["dying"] = want.get("dying", 0) + 1
        if all(want.get(k, 0) >= (3 * per if k in ("edge", "corner", "rest") else per) for k in
               ["face x+", "face x-", "face y+", "face y-", "face z-", "edge", "corner", "rest", "dying"]):
            break
    # nooks: empty cells with occupied neighbours on three perpendicular sides, entered along the diagonal — two and three contacts in
    # one tick for the responses that go on (found in blocks of texels around occupied voxels; the restatement judges the outcome)
    full, R, nooks = occ.minefield == 0, occ.R, 0
    for v in solid[:64]:
        if nooks >= 4 * per:
            break
        t = occ.texel(v)
        b = [slice(max(1, t[a] - 40), min(R - 1, t[a] + 40)) for a in (2, 1, 0)]          # [z, y, x], away from the wrap
        for signs in [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]:
            shifted = [full[tuple(slice(s.start - (signs[2 - i] if i == j else 0), s.stop - (signs[2 - i] if i == j else 0)) for j, s in enumerate(b))]
                       for i in range(3)]                                                    # the neighbour on side -sign of z, y, x
            found = np.argwhere(~full[tuple(b)] & shifted[0] & shifted[1] & shifted[2])
            for z, y, x in found[rng.permutation(len(found))[:2]]:
                tex = np.array([x + b[2].start, y + b[1].start, z + b[0].start])
                n = np.asarray(occ.lr) - R // 2 + (tex - np.asarray(occ.lr)) % R
                if occ.occupied(n) or not all(occ.occupied(n - np.eye(3, dtype=int)[a] * signs[a]) for a in range(3)):
                    continue
                s = f32(rng.choice([0.125, 0.25]))
                gap = rng.uniform(0.03, 0.2, 3)
                lo = np.array([n[a] + gap[a] if signs[a] > 0 else n[a] + 1 - gap[a] - float(s) for a in range(3)])
                vel = -np.array(signs) * speed * rng.uniform(0.8, 1.2, 3)
                if nooks % 4 >= 2:
                    vel[rng.integers(3)] = 0.0                                                  # along an edge of the nook: two contacts
                if add("nook", lo, lo + float(s), vel):
                    out[-1]["flags"] = ref.SLIDE if nooks % 2 else ref.BOUNCE
                    nooks += 1
    # terrain has no overhang: a face is met from below only by coming up from under the window, where everything is air
    floor_z = occ.lr[2] - occ.R // 2
    for v in solid[solid[:, 2] == floor_z][:4 * per] if (solid[:, 2] == floor_z).any() else []:
        s = size()
        lo, hi = beside(v, 2, -1, s, rng.uniform(0.01, 0.3))
        add("floor", lo, hi, (0, 0, speed))
    # open air: far above every occupied voxel of the column's neighbourhood
    top = int(solid[:, 2].max())
    for _ in range(2 * per):
        c = np.array([rng.integers(occ.lr[0] - occ.R // 4, occ.lr[0] + occ.R // 4), rng.integers(occ.lr[1] - occ.R // 4, occ.lr[1] + occ.R // 4),
                      top + 4]) + rng.uniform(0, 1, 3)
        s = size()
        add("air", c, c + float(s), rng.uniform(-speed, speed, 3))
    # the seam: boxes across each seam plane, beside occupied voxels that lie near it
    planes = seam_planes(occ)
    for axis in range(3):
        near = solid[np.abs(solid[:, axis] - planes[axis]) <= 2]
        placed = 0
        for v in near:
            if placed >= per:
                break
            s = size()
            c = v + 0.5 + rng.uniform(-2.0, 2.0, 3)
            c[axis] = planes[axis]
            lo = c - float(s) * 0.5
            aim = (v + 0.5 - c)
            aim[axis] = rng.choice([-1.0, 1.0]) * 0.5
            placed += add("seam", lo, lo + float(s), aim / np.abs(aim).max() * speed)
    return np.array(out, dtype=ref.STATE_DTYPE), kinds


def edited(occ, boxes):
    """The Occupancy after box edits [(texel lo, texel hi, solid, material word)] (both corners inclusive, (x, y, z)): what
    render.box_shape rows do to the resident world, as far as occupancy and materials go."""
    mine, mats = occ.minefield.copy(), occ.materials.copy()
    for lo, hi, solid, word in boxes:
        sel = (slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1), slice(lo[0], hi[0] + 1))
        mine[sel] = 0 if solid else 1
        mats[sel] = word
    return sweep_ref.Occupancy(mats, mine, occ.lr, occ.R)


def floor_texels(occ, states):
    """Per particle the texels (x, y, z) of the cells just below its box."""
    cells = []
    for s in states:
        z = int(np.floor(s["lo"][2])) - 1
        cells.append([occ.texel((x, y, z)) for x in range(int(np.floor(s["lo"][0])), int(np.ceil(s["hi"][0])))
                      for y in range(int(np.floor(s["lo"][1])), int(np.ceil(s["hi"][1])))])
    return cells


def with_table(states, kinds):
    """The set with the table's invalid and inactive records spread through it, at most one in ten."""
    table, verdicts, _ = record_table()
    extra = [i for i, v in enumerate(verdicts) if v != "valid"]
    extra = extra[:len(states) // 10]
    out, names = list(states), list(kinds)
    step = max(1, len(states) // (len(extra) + 1))
    for j, i in enumerate(extra):
        out.insert((j + 1) * step + j, table[i])
        names.insert((j + 1) * step + j, verdicts[i])
    return np.array(out, dtype=ref.STATE_DTYPE), names


def census(states, logs, out, planes=None):
    """What one restated tick did, counted: {'free', 'blocked x+' ... 'blocked z-' (axis and the direction of travel), 'contacts 2',
    'contacts 3' (BLOCKED sub-sweeps in one tick), 'embedded', 'died of age', 'invalid', 'inactive on input', 'straddles seam'}."""
    n = dict.fromkeys(["free", "embedded", "contacts 2", "contacts 3", "died of age", "invalid", "inactive on input", "straddles seam"] +
                      ["blocked %s%s" % (a, d) for a in "xyz" for d in "+-"], 0)
    for i, hits in enumerate(logs):
        if ref.inactive(states[i]):
            n["inactive on input"] += 1
            continue
        if int(out[i]["flags"]) & ref.INVALID:
            n["invalid"] += 1
            continue
        blocked = [h for h in hits if h["kind"] == sweep_ref.BLOCKED]
        for h in blocked:
            n["blocked %s%s" % ("xyz"[h["axis"]], "+" if h["normal"] & 1 else "-")] += 1
        if len(blocked) >= 2:
            n["contacts %d" % min(len(blocked), 3)] += 1
        n["free"] += bool(hits) and hits[-1]["kind"] == sweep_ref.FREE and not blocked
        n["embedded"] += any(h["kind"] == sweep_ref.EMBEDDED for h in hits)
        n["died of age"] += bool(int(out[i]["flags"]) & ref.DEAD) and not any(h["kind"] == sweep_ref.EMBEDDED for h in hits) and \
            not (blocked and int(states[i]["flags"]) & ref.RESPONSE == ref.DIE)
        if planes is not None:
            n["straddles seam"] += any(states[i]["lo"][a] < planes[a] < states[i]["hi"][a] for a in range(3))
    return n
