"""numpy restatement of rt_emit_particles (include/rt_abi.h "Particle emitters") for the emitter tests.  Test infrastructure, written
from the rules and not from the kernels.

Membership and the bounding box are tests/shape_edits.py's (`bounding_box`, `selected`): no shape rule is restated here.  Arrays are
[z, y, x] in texel order; an emitter is one row of EMIT_DTYPE (RtParticleEmit's 96 bytes), a particle one row of
particle_step_ref.STATE_DTYPE.  Integers are int64 / uint32 on whole arrays; the float block is float32 arrays, one rounding per
operation, with draw_boxes_ref's fused multiply-add for rtm_length3."""
import numpy as np

from tests import draw_boxes_ref
from tests import particle_step_ref
from tests import shape_edits as se

f32 = np.float32
u32 = np.uint32
STATE_DTYPE = particle_step_ref.STATE_DTYPE

# numpy views of RtParticleEmit and RtEmitCursor, declared here a second time on purpose (the binding's own are
# raytrace_amd.abi.EMIT_DTYPE and EMIT_CURSOR_DTYPE)
EMIT_DTYPE = np.dtype([("a", "<i4", 3), ("seed", "<u4"), ("b", "<i4", 3), ("kind", "u1"), ("response", "u1"), ("reserved0", "u1", 2),
                       ("origin", "<f4", 3), ("speed", "<f4"), ("drift", "<f4", 3), ("spread", "<f4"), ("half", "<f4"), ("life_min", "<f4"),
                       ("life_span", "<f4"), ("density", "<u4"), ("light", "<u4"), ("emission", "<u4"), ("reserved", "<u4", 2)])
CURSOR_DTYPE = np.dtype([("next", "<u4"), ("emitted", "<u4"), ("dropped", "<u4"), ("reserved", "<u4")])
assert EMIT_DTYPE.itemsize == 96 and CURSOR_DTYPE.itemsize == 16

MAX_EMITTERS, MAX_CAPACITY, MAX_BRICKS = 256, 1 << 20, 1 << 18


def emitter(shape, origin, seed=0, speed=0.0, drift=(0, 0, 0), spread=0.0, half=0.125, life_min=np.inf, life_span=0.0, density=256,
            response=0, light=0, emission=0xFF000000):
    """One EMIT_DTYPE row from a shape_edits row (a, b and kind are read)."""
    e = np.zeros((), EMIT_DTYPE)
    e["a"], e["b"], e["kind"] = shape["a"], shape["b"], shape["kind"]
    e["origin"], e["drift"] = origin, drift
    e["seed"], e["speed"], e["spread"], e["half"], e["life_min"], e["life_span"] = seed, speed, spread, half, life_min, life_span
    e["density"], e["response"], e["light"], e["emission"] = density, response, light, emission
    return e


def batch(emitters):
    return np.array([np.asarray(e, dtype=EMIT_DTYPE) for e in emitters], dtype=EMIT_DTYPE).reshape(-1)


def shape_of(e):
    """The emitter's shape as a shape_edits row (where ALL: occupancy is this module's business)."""
    s = np.zeros((), se.SHAPE_DTYPE)
    s["a"], s["b"], s["kind"] = e["a"], e["b"], e["kind"]
    return s


def valid(e, R):
    """The host's verdict on one emitter."""
    s = shape_of(e)
    if e["kind"] > se.SPHERE or not se.valid(s, R):
        return False
    if e["response"] > 3 or e["reserved0"].any() or e["reserved"].any() or not 1 <= int(e["density"]) <= 256:
        return False
    floats = [e["speed"], e["spread"], e["half"], e["life_span"]] + list(e["origin"]) + list(e["drift"])
    if not all(np.isfinite(v) for v in floats) or np.isnan(e["life_min"]):
        return False
    return bool(2.0 ** -8 <= e["half"] <= 0.5 and 0 <= e["speed"] <= 4096 and 0 <= e["spread"] <= 4096 and
                (np.abs(e["drift"]) <= 4096).all() and (np.abs(e["origin"]) <= 2.0 ** 22).all() and e["life_min"] > 0 and
                0 <= e["life_span"] <= 4096)


def window_valid(lr, R):
    return all(abs(int(v)) <= 2 ** 22 - R for v in lr)


def brick_boxes(emitters, R):
    """The plan: per emitter with a bounding box (emitter index, low brick (x, y, z), bricks per axis (x, y, z), first item), and the
    number of items (bricks) in all."""
    out, items = [], 0
    for i, e in enumerate(emitters):
        bb = se.bounding_box(shape_of(e), R)
        if bb is None:
            continue
        blo, bhi = bb[0] >> 2, bb[1] >> 2
        n = bhi - blo + 1
        out.append((i, tuple(int(v) for v in blo), tuple(int(v) for v in n), items))
        items += int(n[0] * n[1] * n[2])
    return out, items


def mix(h):
    h = h.astype(u32).copy()
    h ^= h >> u32(16)
    h *= u32(0x7feb352d)
    h ^= h >> u32(15)
    h *= u32(0x846ca68b)
    h ^= h >> u32(16)
    return h


def world_voxels(xyz, lr, R):
    """int64[N, 3] texels -> the world voxels they hold under window centre lr."""
    lr = np.asarray(lr, dtype=np.int64)
    return lr - R // 2 + np.mod(xyz - lr, R)


def voxel_hash(seed, v):
    """uint32[N]: h of the world voxels int64[N, 3]."""
    w = (v & 0xFFFFFFFF).astype(u32)
    return mix(u32(seed) ^ mix(w[:, 0] ^ mix(w[:, 1] ^ mix(w[:, 2]))))


def select(mine, e, lr):
    """The texels int64[N, 3] (x, y, z) one emitter selects in a region whose minefield is `mine`, in emission order."""
    R = mine.shape[0]
    bb = se.bounding_box(shape_of(e), R)
    if bb is None:
        return np.zeros((0, 3), np.int64)
    sl = tuple(slice(int(bb[0][k]), int(bb[1][k]) + 1) for k in (2, 1, 0))        # (only to look at fewer voxels)
    z, y, x = np.nonzero(se.selected(shape_of(e), R, None)[sl] & (mine[sl] == 0))
    xyz = (np.stack([x, y, z], axis=1).astype(np.int64) + bb[0]).reshape(-1, 3)
    h = voxel_hash(e["seed"], world_voxels(xyz, lr, R))
    xyz = xyz[(h & u32(255)) < u32(e["density"])]
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    order = np.lexsort((x & 3, y & 3, z & 3, x >> 2, y >> 2, z >> 2))     # the last key is the primary one
    return xyz[order]


def order_key(xyz):
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return [tuple(int(v) for v in k) for k in zip(z >> 2, y >> 2, x >> 2, z & 3, y & 3, x & 3)]


def states_of(mats, e, xyz, lr):
    """STATE_DTYPE[N]: the particles of the texels `xyz` of one emitter."""
    R = mats.shape[0]
    n = len(xyz)
    out = np.zeros(n, dtype=STATE_DTYPE)
    if n == 0:
        return out
    v = world_voxels(xyz, lr, R)
    h = voxel_hash(e["seed"], v)
    with np.errstate(all="ignore"):
        u = [(mix(h + u32(i)) >> u32(8)).astype(f32) * f32(2.0 ** -24) for i in (1, 2, 3, 4)]
        half, speed, spread = f32(e["half"]), f32(e["speed"]), f32(e["spread"])
        c = v.astype(f32) + f32(0.5)
        out["lo"], out["hi"] = c - half, c + half
        r = c - e["origin"].astype(f32)
        length = draw_boxes_ref.length3(r[:, 0], r[:, 1], r[:, 2])
        for k in range(3):
            d = np.where(length > 0, r[:, k] / np.where(length > 0, length, f32(1.0)), f32(0.0)).astype(f32)
            jitter = ((u[k] * f32(2.0)) - f32(1.0)) * spread
            out["velocity"][:, k] = ((d * speed) + jitter) + f32(e["drift"][k])
        out["life"] = f32(e["life_min"]) + u[3] * f32(e["life_span"])
    out["flags"] = u32(e["response"])
    out["material"] = mats[xyz[:, 2], xyz[:, 1], xyz[:, 0]]
    out["light"], out["emission"], out["half"] = e["light"], e["emission"], e["half"]
    return out


def particles(mats, mine, emitters, lr):
    """Every particle the batch emits before the ring cuts it, in order -> (STATE_DTYPE[N], texels int64[N, 3], emitter index[N])."""
    parts, texels, who = [np.zeros(0, STATE_DTYPE)], [np.zeros((0, 3), np.int64)], [np.zeros(0, np.int64)]
    for i, e in enumerate(emitters):
        xyz = select(mine, e, lr)
        parts.append(states_of(mats, e, xyz, lr))
        texels.append(xyz)
        who.append(np.full(len(xyz), i, np.int64))
    return np.concatenate(parts), np.concatenate(texels), np.concatenate(who)


def emit(mats, mine, emitters, lr, ring, max_emit, cursor, device=True):
    """One call -> (N, the ring after it, the cursor after it).  `ring`: STATE_DTYPE[capacity] (any bytes), `cursor` a CURSOR_DTYPE
    record.  `device`: an input next >= capacity is taken mod capacity (the synchronous call refuses it)."""
    ring = np.array(ring, dtype=STATE_DTYPE).reshape(-1)
    cur = np.array(cursor, dtype=CURSOR_DTYPE).reshape(1)[0].copy()
    capacity = ring.size
    assert 1 <= max_emit <= capacity <= MAX_CAPACITY and len(emitters) <= MAX_EMITTERS
    assert device or int(cur["next"]) < capacity
    all_states, _, _ = particles(mats, mine, emitters, lr)
    N = len(all_states)
    if not brick_boxes(emitters, mine.shape[0])[0]:
        return 0, ring, cur                                    # nothing enqueued: the cursor keeps even a next >= capacity
    n = min(N, int(max_emit))
    start = int(cur["next"]) % capacity
    ring[(start + np.arange(n)) % capacity] = all_states[:n]
    cur["next"] = (start + n) % capacity
    cur["emitted"] = (int(cur["emitted"]) + n) & 0xFFFFFFFF
    cur["dropped"] = (int(cur["dropped"]) + N - n) & 0xFFFFFFFF
    return N, ring, cur
