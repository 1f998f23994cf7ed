"""numpy restatement of rt_sweep_entities (include/rt_abi.h "Entity sweeps", DESIGN.md "Entity sweeps").  Test infrastructure.

Written from the header's words, not from the kernel: no cull, no cell ranges — every box and every SOLID cell of every model is
one obstacle box under the obstacle rule, for every sweep.  float32, one rounding per operation; the planes of a model go through
the exact fma emulation the drawing references use.  The world part W is tests/sweep_ref.sweep; the event loop is restated here a
second time with a horizon (`world_events`), which gives the cell ranges the returned box of an entity block is clamped with, and
which at horizon 1 is sweep_ref.sweep itself (tests/test_sweep_entities_contract.py holds the two against each other).

    sweep_entities(occ, sweeps, boxes, models, stamps)  -> (world_hits sweep_ref.HIT_DTYPE[N], entity_hits HIT_DTYPE[N])
    obstacle(olo, ohi, lo, hi, m)                       -> the obstacle rule for arrays of boxes against one sweep
    entity_part(lo, hi, m, boxes, models, stamps, ...)  -> what the entities do to one sweep before the world is looked at

`occ` is a sweep_ref.Occupancy (or anything with its first_occupied); `sweeps` RtBoxSweep records (SWEEP_DTYPE below; reserved0 /
reserved1 carry the self exemption); boxes RtDrawBox records; models RtDrawStamp records; `stamps` maps a stamp id to
(materials u32[ez, ey, ex], state u8[ez, ey, ex])."""
import numpy as np

from tests import stamp_edits as se
from tests import sweep_ref as sr
from tests.draw_boxes_ref import fma

f32 = np.float32
FREE, BLOCKED, EMBEDDED, INVALID = 0, 1, 2, 3
NONE, BOX, MODEL = 0, 1, 2
MAX_COORD = f32(4194304.0)

# numpy views of the records, declared here a second time on purpose (the binding's own are raytrace_amd.render's)
SWEEP_DTYPE = np.dtype([("lo", "<f4", 3), ("reserved0", "<u4"), ("hi", "<f4", 3), ("reserved1", "<u4"), ("motion", "<f4", 3), ("reserved2", "<u4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("kind", "<u4"), ("normal", "<u4"), ("material", "<u4"),
                      ("entity", "<u4"), ("index", "<u4"), ("axis", "<u4"), ("voxel", "<u4"),
                      ("cell", "<i4", 3), ("reserved0", "<u4"), ("lo", "<f4", 3), ("reserved1", "<u4"), ("hi", "<f4", 3), ("reserved2", "<u4")])
assert SWEEP_DTYPE.itemsize == 48 and HIT_DTYPE.itemsize == 80


def make_sweeps(lo, hi, motion, skip_box=None, skip_model=None):
    """SWEEP_DTYPE[N] from float[N, 3] arrays; skip_box / skip_model: per sweep the index of the entity it ignores, or -1."""
    lo = np.asarray(lo, dtype=f32).reshape(-1, 3)
    out = np.zeros(lo.shape[0], dtype=SWEEP_DTYPE)
    out["lo"], out["hi"], out["motion"] = lo, np.asarray(hi, dtype=f32).reshape(-1, 3), np.asarray(motion, dtype=f32).reshape(-1, 3)
    if skip_box is not None:
        out["reserved0"] = np.asarray(skip_box, dtype=np.int64) + 1
    if skip_model is not None:
        out["reserved1"] = np.asarray(skip_model, dtype=np.int64) + 1
    return out


def box_valid(lo, hi):
    """rt_draw_boxes' valid box."""
    with np.errstate(invalid="ignore"):
        return bool(((np.abs(lo) <= MAX_COORD) & (np.abs(hi) <= MAX_COORD) & (lo < hi)).all())


# ---- the obstacle rule -------------------------------------------------------------------------------------------------------------
def axis_terms(olo, ohi, lo, hi, m):
    """One axis of obstacles [olo, ohi] (arrays) against the sweep's scalars: (start, te, tx); te and tx are None when m == 0."""
    olo, ohi = np.asarray(olo, dtype=f32), np.asarray(ohi, dtype=f32)
    with np.errstate(all="ignore"):
        start = (lo < ohi) & (olo < hi)
        if m > 0:
            return start, ((olo - hi).astype(f32) / m).astype(f32), ((ohi - lo).astype(f32) / m).astype(f32)
        if m < 0:
            return start, ((ohi - lo).astype(f32) / m).astype(f32), ((olo - hi).astype(f32) / m).astype(f32)
    return start, None, None


def combine(terms):
    """The rule from the three axes' (start, te, tx), whose arrays broadcast against each other: (embedded, blocked, t, axis)."""
    shape = np.broadcast_shapes(*[t[0].shape for t in terms])
    embedded = np.ones(shape, dtype=bool)
    still = np.ones(shape, dtype=bool)          # every axis that does not move overlaps at the start
    have = False
    te_a = np.zeros(shape, dtype=f32)
    a = np.full(shape, 3, dtype=np.int64)
    with np.errstate(all="ignore"):
        for k, (start, te, tx) in enumerate(terms):
            embedded = embedded & start
            if te is None:
                still = still & start
                continue
            take = np.ones(shape, dtype=bool) if not have else np.broadcast_to(te, shape) >= te_a   # the highest axis on equal values
            te_a = np.where(take, te, te_a).astype(f32)
            a = np.where(take, k, a)
            have = True
        blocked = ~embedded & still & have & (te_a >= 0) & (te_a < 1)
        for start, te, tx in terms:
            if te is not None:
                blocked = blocked & (te_a < tx)
    return embedded, blocked, te_a, a


def obstacle(olo, ohi, lo, hi, m):
    """The rule for obstacle boxes olo, ohi [B, 3] against one sweep: (embedded[B], blocked[B], t[B], axis[B])."""
    olo, ohi = np.asarray(olo, dtype=f32).reshape(-1, 3), np.asarray(ohi, dtype=f32).reshape(-1, 3)
    return combine([axis_terms(olo[:, k], ohi[:, k], lo[k], hi[k], m[k]) for k in range(3)])


# ---- one model: every SOLID cell as a box ----------------------------------------------------------------------------------------------
def model_planes(origin, scale, ext):
    """plane_k(i) = rtm_fma(float(i), scale, origin_k), i = 0..E'_k, per axis."""
    return [fma(np.arange(ext[k] + 1, dtype=f32), np.full(ext[k] + 1, scale, dtype=f32), np.full(ext[k] + 1, origin[k], dtype=f32)) for k in range(3)]


def model_obstacle(planes, state, lo, hi, m):
    """What one placed model (state [z, y, x]) does to one sweep: None, ("E", cell) or ("B", t, axis, cell, face)."""
    shapes = [(1, 1, -1), (1, -1, 1), (-1, 1, 1)]     # the cells as a [z, y, x] array
    terms, merged = [], np.zeros((1, 1, 1), dtype=bool)
    for k in range(3):
        p0, p1 = planes[k][:-1], planes[k][1:]
        start, te, tx = axis_terms(p0, p1, lo[k], hi[k], m[k])
        terms.append((start.reshape(shapes[k]), None if te is None else te.reshape(shapes[k]), None if tx is None else tx.reshape(shapes[k])))
        merged = merged | (p0 == p1).reshape(shapes[k])
    embedded, blocked, t, a = combine(terms)
    exists = (np.asarray(state) == se.SOLID) & ~merged
    emb = np.argwhere(embedded & exists)              # rows in ascending (z, y, x)
    if emb.size:
        z, y, x = emb[0]
        return ("E", (int(x), int(y), int(z)))
    cand = blocked & exists
    if not cand.any():
        return None
    t = np.broadcast_to(t, cand.shape)
    a = np.broadcast_to(a, cand.shape)
    tmin = t[cand].min()
    cand = cand & (t == tmin)
    amin = a[cand].min()
    z, y, x = np.argwhere(cand & (a == amin))[0]
    cell = (int(x), int(y), int(z))
    face = planes[amin][cell[amin] if m[amin] > 0 else cell[amin] + 1]
    return ("B", f32(t[z, y, x]), int(amin), cell, f32(face))      # (the winner's own te: a -0 stays a -0)


def place(models, stamps):
    """Per model: (planes, placed state [z, y, x], the stamp voxel index each placed cell shows [z, y, x], materials flat)."""
    out, cache = [], {}
    for mrec in np.asarray(models).reshape(-1):
        key = (int(mrec["stamp"]), int(mrec["orient"]))
        if key not in cache:
            mats, state = stamps[key[0]]
            state = np.asarray(state, dtype=np.uint8)
            cache[key] = (se.oriented(state, key[1]), se.oriented(np.arange(state.size, dtype=np.int64).reshape(state.shape), key[1]),
                          np.asarray(mats, dtype=np.uint32).reshape(-1))
        st, vox, mats = cache[key]
        out.append((model_planes(mrec["origin"].astype(f32), f32(mrec["scale"]), se.extent_of(st)), st, vox, mats))
    return out


# ---- the entity part of one sweep ---------------------------------------------------------------------------------------------------
def entity_part(lo, hi, m, boxes, placed, skip_box=0, skip_model=0):
    """None, or a dict: kind EMBEDDED / BLOCKED, entity, index, and for a block t, axis, face; for a model cell, voxel; material."""
    nb = 0 if boxes is None else boxes.size
    blocks = []
    if nb:
        olo, ohi = boxes["lo"].astype(f32), boxes["hi"].astype(f32)
        ok = np.array([box_valid(olo[j], ohi[j]) for j in range(nb)], dtype=bool)
        if 1 <= skip_box <= nb:
            ok[skip_box - 1] = False
        emb, blk, t, a = obstacle(olo, ohi, lo, hi, m)
        emb, blk = emb & ok, blk & ok
        if emb.any():
            j = int(np.argmax(emb))
            return {"kind": EMBEDDED, "entity": BOX, "index": j, "material": int(boxes["material"][j])}
        for j in np.nonzero(blk)[0]:
            ax = int(a[j])
            blocks.append((t[j], 0, int(j), ax, f32(olo[j, ax] if m[ax] > 0 else ohi[j, ax]), None))
    found = []
    for j, (planes, state, vox, mats) in enumerate(placed):
        if j + 1 == skip_model:
            continue
        r = model_obstacle(planes, state, lo, hi, m)
        if r is None:
            continue
        cell = r[1] if r[0] == "E" else r[3]
        v = int(vox[cell[2], cell[1], cell[0]])
        if r[0] == "E":
            if not any(f[0] == "E" for f in found):
                found.append(("E", j, cell, v, int(mats[v])))
        else:
            blocks.append((r[1], 1, j, r[2], r[4], (cell, v, int(mats[v]))))
    for f in found:
        return {"kind": EMBEDDED, "entity": MODEL, "index": f[1], "cell": f[2], "voxel": f[3], "material": f[4]}
    if not blocks:
        return None
    t, kind, j, ax, face, more = min(blocks, key=lambda b: (b[0], b[1], b[2]))   # smallest t; boxes before models; lowest index
    out = {"kind": BLOCKED, "entity": MODEL if kind else BOX, "index": j, "t": f32(t), "axis": ax, "face": face}
    if kind:
        out["cell"], out["voxel"], out["material"] = more
    else:
        out["material"] = int(boxes["material"][j])
    return out


# ---- the world's event loop, restated with a horizon -----------------------------------------------------------------------------------
def world_events(occ, lo, hi, m, horizon=f32(1.0)):
    """rt_sweep_boxes' embedded scan and event loop for a sweep inside the domain, over the events with t < horizon only.  Returns
    (kind, t, axis, plane g, found, c): c the cell ranges when the loop ended.  At horizon 1 this is the whole sweep."""
    lo, hi, m = [f32(v) for v in lo], [f32(v) for v in hi], [f32(v) for v in m]
    horizon = f32(horizon)
    with np.errstate(all="ignore"):
        c = [[int(np.floor(lo[k])), int(np.ceil(hi[k])) - 1] for k in range(3)]
        found = occ.first_occupied(c[0], c[1], c[2])
        if found:
            return EMBEDDED, f32(0.0), 3, None, found, c
        # per (trailing = 0 / leading = 1, axis): the face and the pending plane
        pend = {}
        for k in range(3):
            if m[k] > 0:
                pend[(0, k)] = [lo[k], c[k][0] + 1]
                pend[(1, k)] = [hi[k], c[k][1] + 1]
            elif m[k] < 0:
                pend[(0, k)] = [hi[k], c[k][1]]
                pend[(1, k)] = [lo[k], c[k][0]]
        while True:
            best, bt = None, horizon
            for key in sorted(pend):                 # trailing before leading, then x, y, z: a strict < keeps the first
                face, g = pend[key]
                t = f32(f32(f32(g) - face) / m[key[1]])
                if t < bt:
                    best, bt = key, t
            if best is None:
                return FREE, f32(1.0), 3, None, None, c
            lead, k = best
            g = pend[best][1]
            up = m[k] > 0
            if not lead:
                if up:
                    c[k][0] = g
                else:
                    c[k][1] = g - 1
            else:
                layer = g if up else g - 1
                r = [list(c[0]), list(c[1]), list(c[2])]
                r[k] = [layer, layer]
                found = occ.first_occupied(r[0], r[1], r[2])
                if found:
                    return BLOCKED, bt, k, g, found, c
                if up:
                    c[k][1] = layer
                else:
                    c[k][0] = layer
            pend[best][1] = g + 1 if up else g - 1


def returned_box(lo, hi, m, t, c, axis=None, face=None):
    """rt_sweep_boxes' "Returned box" at time t with the ranges c; on the blocked axis the faces snap to `face`."""
    rl, rh = list(lo), list(hi)
    with np.errstate(all="ignore"):
        for k in range(3):
            if m[k] == 0:
                continue
            cl, ch = f32(c[k][0]), f32(c[k][1] + 1)
            x = f32(lo[k] + f32(m[k] * t))
            rl[k] = cl if x < cl else x
            x = f32(hi[k] + f32(m[k] * t))
            rh[k] = ch if x > ch else x
            if axis == k:
                size = f32(hi[k] - lo[k])
                if m[k] > 0:
                    rh[k] = f32(face)
                    x = f32(f32(face) - size)
                    rl[k] = cl if x < cl else x
                else:
                    rl[k] = f32(face)
                    x = f32(f32(face) + size)
                    rh[k] = ch if x > ch else x
    return rl, rh


def horizon_sweep(occ, lo, hi, m):
    """world_events at horizon 1 as a sweep_ref hit dict: what the contract test holds against sweep_ref.sweep."""
    lo, hi, m = [f32(v) for v in lo], [f32(v) for v in hi], [f32(v) for v in m]
    if not sr.in_domain(lo, hi, m):
        return sr._hit(INVALID, 0.0, 6, 0, sr.NO_TEXEL, 3, lo, hi)
    kind, t, axis, g, found, c = world_events(occ, lo, hi, m)
    if kind == EMBEDDED:
        return sr._hit(EMBEDDED, 0.0, 6, found[1], found[0], 3, lo, hi)
    if kind == FREE:
        rl, rh = returned_box(lo, hi, m, f32(1.0), c)
        return sr._hit(FREE, 1.0, 6, 0, sr.NO_TEXEL, 3, rl, rh)
    rl, rh = returned_box(lo, hi, m, t, c, axis, f32(g))
    return sr._hit(BLOCKED, t, 2 * axis + (1 if m[axis] > 0 else 0), found[1], found[0], axis, rl, rh)


# ---- the call -------------------------------------------------------------------------------------------------------------------------
def sweep_one(occ, s, boxes, placed):
    """One record: (the world's sweep_ref hit dict W, the entity record as a dict, the outcome class for the census)."""
    lo, hi, m = [f32(v) for v in s["lo"]], [f32(v) for v in s["hi"]], [f32(v) for v in s["motion"]]
    W = sr.sweep(occ, lo, hi, m)
    rec = {"t": f32(1.0), "kind": FREE, "normal": 6, "material": 0, "entity": NONE, "index": 0xFFFFFFFF, "axis": 3, "voxel": 0xFFFFFFFF,
           "cell": (-1, -1, -1), "lo": W["lo"], "hi": W["hi"]}
    if W["kind"] == INVALID:
        rec["kind"], rec["t"] = INVALID, f32(0.0)
        return W, rec, "invalid"
    e = entity_part(lo, hi, m, boxes, placed, int(s["reserved0"]), int(s["reserved1"]))
    if e is None:
        return W, rec, "none" if W["kind"] == FREE else "world only"
    if e["kind"] == BLOCKED and not (W["kind"] in (FREE, BLOCKED) and e["t"] < W["t"]):
        return W, rec, "tie" if W["kind"] == BLOCKED and e["t"] == W["t"] else "world earlier"
    rec["entity"], rec["index"], rec["material"] = e["entity"], e["index"], e["material"]
    if e["entity"] == MODEL:
        rec["cell"], rec["voxel"] = e["cell"], e["voxel"]
    if e["kind"] == EMBEDDED:
        rec["kind"], rec["t"], rec["lo"], rec["hi"] = EMBEDDED, f32(0.0), lo, hi
        return W, rec, "embedded"
    kind, _, _, _, _, c = world_events(occ, lo, hi, m, e["t"])
    assert kind == FREE, "no world event before t_e blocks: t_e < W.t"
    a = e["axis"]
    rec["kind"], rec["t"], rec["axis"], rec["normal"] = BLOCKED, e["t"], a, 2 * a + (1 if m[a] > 0 else 0)
    rec["lo"], rec["hi"] = returned_box(lo, hi, m, e["t"], c, a, e["face"])
    return W, rec, "box" if e["entity"] == BOX else "model"


def pack(recs):
    out = np.zeros(len(recs), dtype=HIT_DTYPE)
    for i, r in enumerate(recs):
        for name in ("t", "kind", "normal", "material", "entity", "index", "axis", "voxel", "cell", "lo", "hi"):
            out[i][name] = r[name]
    return out


def sweep_entities(occ, sweeps, boxes=None, models=None, stamps=None, classes=False):
    """rt_sweep_entities: (world_hits sweep_ref.HIT_DTYPE[N], entity_hits HIT_DTYPE[N]) and, with classes=True, the outcome class of
    every sweep: "box", "model", "world earlier", "tie", "embedded", "invalid", "none" (nothing anywhere), "world only"."""
    sweeps = np.asarray(sweeps).reshape(-1)
    boxes = None if boxes is None else np.asarray(boxes).reshape(-1)
    placed = place(models, stamps or {}) if models is not None and np.asarray(models).size else []
    res = [sweep_one(occ, s, boxes, placed) for s in sweeps]
    out = sr.pack([r[0] for r in res]), pack([r[1] for r in res])
    return out + ([r[2] for r in res],) if classes else out
