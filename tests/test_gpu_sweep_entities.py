"""Entity sweeps on the GPU (rt_sweep_entities, rt_sweep_entities_async).  Every comparison is bit for bit, on every byte of both
outputs: the entity part with tests/sweep_entities_ref.py — which has no cull and tests every box and every SOLID cell against every
sweep — the world part with that file's sweep_ref records and with rt_sweep_boxes itself.  The cases are those whose census
tests/test_sweep_entities_contract.py asserts: sweep counts round the 256-thread workgroup and the 64-lane wave, entity counts round
the kernel's 64-record batches; then models in all 48 orientations at three scales, the cull's margin on both sides, region 512
across a scrolled seam, an edit between two calls, the asynchronous call behind a capture, the refusals, and the returned boxes
swept again."""
import ctypes as C

import numpy as np
import pytest
import torch

from raytrace_amd import abi, render, world
from tests import stamp_edits as se
from tests import sweep_entities_ref as ref
from tests import sweep_entities_sets as sets
from tests import sweep_ref as sr
from tests import test_sweep_entities_contract as tc

pytestmark = pytest.mark.gpu
f32 = np.float32


def _dev(records):
    a = np.ascontiguousarray(records)
    return torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], -1).copy()).cuda()


def _out(n, width):
    t = torch.full((n, width), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def same_records(got, want, what):
    assert got.dtype.itemsize == want.dtype.itemsize and got.size == want.size, what
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.view(np.uint8).reshape(got.size, -1) != want.view(np.uint8).reshape(want.size, -1)).any(axis=1))[0]
        raise AssertionError("%s: %d of %d records differ, first %s\n got  %s\n want %s" % (what, bad.size, got.size, bad[:8].tolist(), got[bad[0]], want[bad[0]]))


def run_async(ctx, c, lr=(0, 0, 0), world_hits=True):
    """The asynchronous call on device copies of the case: (world_hits or None, entity_hits) as numpy records."""
    n = c["sweeps"].size
    sweeps = _dev(c["sweeps"])
    boxes = _dev(c["boxes"]) if c["boxes"] is not None and c["boxes"].size else None
    wh, eh = (_out(n, 64) if world_hits else None), _out(n, 80)
    ctx.sweep_entities_async(sweeps, boxes, c["models"], wh, eh, lr)
    ctx.sync()
    return (None if wh is None else wh.cpu().numpy().view(render.SWEEP_HIT_DTYPE).reshape(-1)), eh.cpu().numpy().view(abi.ENTITY_SWEEP_HIT_DTYPE).reshape(-1)


def check_case(ctx, occ, c, stamps, what, lr=(0, 0, 0)):
    """Both calls against the restatement and against rt_sweep_boxes; the entity part alone with world_hits NULL; the returned boxes
    swept again with no motion."""
    W, E = ref.sweep_entities(occ, c["sweeps"], c["boxes"], c["models"], stamps)
    valid = W["kind"] != sr.INVALID
    if valid.all():
        gw, ge = ctx.sweep_entities(c["sweeps"], lr, c["boxes"], c["models"])
        same_records(gw, W, what + ": world part against the restatement")
        same_records(gw, ctx.sweep_boxes(c["sweeps"], lr), what + ": world part against rt_sweep_boxes")
        same_records(ge, E, what + ": entity part")
        none, ge2 = ctx.sweep_entities(c["sweeps"], lr, c["boxes"], c["models"], world=False)
        assert none is None
        same_records(ge2, E, what + ": entity part with world_hits NULL")
    aw, ae = run_async(ctx, c, lr)
    same_records(aw, W, what + ": asynchronous world part")
    same_records(ae, E, what + ": asynchronous entity part")
    _, ae2 = run_async(ctx, c, lr, world_hits=False)
    same_records(ae2, E, what + ": asynchronous entity part with world_hits NULL")
    # the combined box is the next sweep's: never world-EMBEDDED unless this sweep's start was
    again = valid & (W["kind"] != sr.EMBEDDED)
    if again.any():
        rest = np.zeros(int(again.sum()), dtype=render.SWEEP_DTYPE)
        rest["lo"], rest["hi"] = ae["lo"][again], ae["hi"][again]
        kinds = ctx.sweep_boxes(rest, lr)["kind"]
        assert (kinds == sr.FREE).all(), (what, np.bincount(kinds, minlength=4))
    return W, E


@pytest.fixture(scope="module")
def arena(native_built):
    mats, mine = world.region_from_ids(sets.arena_ids())
    occ = sr.Occupancy(mats, mine, (0, 0, 0), 256)
    ctx = render.Context(render.make_config(64, 40))
    ctx.upload_world(mats, mine)
    ids = [ctx.stamp_create(*sets.stamp_arrays(*spec)) for spec in sets.SPECS]
    stamps, cases = tc.cases(ids)
    yield ctx, occ, ids, stamps, cases
    ctx.destroy()


def test_hand_built_and_seeded_cases(arena):
    """Every case of the census: sweep counts 1, 12, 40, 63, 64, 65, 257; nboxes 0, 1, 12, 63, 64, 65, 130; nmodels 0, 1, 3, 12, 65."""
    ctx, occ, ids, stamps, cases = arena
    total = {k: 0 for k in tc.CLASSES}
    for i, c in enumerate(cases):
        check_case(ctx, occ, c, stamps, "case %d (%s)" % (i, c["aim"]))
        for k, v in tc.census(occ, c, stamps)[2].items():
            total[k] += v
    assert min(total.values()) >= 8, total          # (the contract test's census, on the ids this context gave its stamps)
    assert {c["sweeps"].size for c in cases} >= {1, 63, 64, 65, 257}
    assert {0 if c["boxes"] is None else c["boxes"].size for c in cases} >= {0, 1, 63, 64, 65, 130}
    assert {0 if c["models"] is None else c["models"].size for c in cases} >= {0, 1, 65}


@pytest.mark.parametrize("scale", [1.0 / 16.0, 1.0, 3.0])
def test_models_in_all_48_orientations(arena, scale):
    ctx, occ, ids, stamps, _ = arena
    rng = np.random.default_rng(31)
    n = 48
    grid = np.stack([(np.arange(n) % 8) * 60.0 * max(scale, 0.25) - 20.0, (np.arange(n) // 8) * 60.0 * max(scale, 0.25) - 20.0, rng.uniform(0.0, 2.0, n)], 1)
    models = sets.models_of(np.array([ids[0], ids[1]], dtype=np.uint32)[np.arange(n) % 2], grid, scale, np.arange(n))
    c = {"aim": "orientations", "boxes": None, "models": models, "sweeps": sets.sweeps_at(32, 144, None, models, stamps)}
    W, E = check_case(ctx, occ, c, stamps, "orientations at scale %g" % scale)
    hit = E["entity"] == ref.MODEL
    assert len(set(E["index"][hit])) >= 24 and (E["kind"][hit] == ref.BLOCKED).sum() >= 40 and (E["kind"][hit] == ref.EMBEDDED).sum() >= 4


def test_obstacles_at_the_culls_margin(arena):
    """A wave of far-apart sweeps — its bounds span the arena, so nothing is culled for want of distance — and per sweep obstacles
    whose faces lie exactly on the faces of its swept hull, one float inside and one float outside, on both sides of an axis: what
    the exact rule says at te = 1, at tx = te and at a touching start is what the kernel says."""
    ctx, occ, ids, stamps, _ = arena
    rng = np.random.default_rng(41)
    n = 64
    lo = np.stack([rng.uniform(-100.0, 100.0, n), rng.uniform(-100.0, 100.0, n), rng.uniform(8.0, 40.0, n)], 1).astype(f32)
    size = rng.uniform(0.3, 2.0, (n, 3)).astype(f32)
    hi = (lo + size).astype(f32)
    k = (np.arange(n) // 2) % 3
    sign = np.where((np.arange(n) // 6) % 2, -1.0, 1.0)
    m = np.zeros((n, 3), dtype=f32)
    m[np.arange(n), k] = (sign * rng.uniform(0.5, 6.0, n)).astype(f32)
    m[np.arange(n), (k + 1) % 3] = rng.uniform(-0.25, 0.25, n).astype(f32)
    blo, bhi, origins = [], [], []
    E3 = np.array(se.extent_of(stamps[ids[2]][1]), dtype=f32)                                # the solid 3 x 11 x 4 stamp at scale 1
    for i in range(n):
        a = k[i]
        end = f32(hi[i, a] + m[i, a]) if sign[i] > 0 else f32(lo[i, a] + m[i, a])          # where the leading face ends
        start = lo[i, a] if sign[i] > 0 else hi[i, a]                                        # the trailing face at the start
        ahead = (end, np.nextafter(end, f32(-sign[i] * np.inf)), np.nextafter(end, f32(sign[i] * np.inf)))[(i // 12) % 3]
        behind = [(start, -1.0)] + ([(np.nextafter(start, f32(sign[i] * np.inf)), -1.0)] if i % 8 == 7 else [])
        if i % 2 == 0:                                       # ahead: a model whose first (or last) plane is that face
            o = (lo[i] - f32(0.5)).astype(f32)
            o[a] = ahead if sign[i] > 0 else f32(ahead - E3[a])
            origins.append(o)
        for face, thick in ([(ahead, 1.0)] if i % 2 else []) + behind:
            l, h = lo[i].copy() - f32(0.5), hi[i].copy() + f32(0.5)
            near, far = f32(face), f32(face + f32(sign[i] * thick))
            l[a], h[a] = min(near, far), max(near, far)
            blo.append(l)
            bhi.append(h)
    c = {"aim": "margin", "boxes": sets.boxes_of(np.array(blo), np.array(bhi), 4), "models": sets.models_of(ids[2], np.array(origins), 1.0, 0),
         "sweeps": ref.make_sweeps(lo, hi, m)}
    W, E = check_case(ctx, occ, c, stamps, "the cull's margin")
    kinds = np.bincount(E["kind"], minlength=4)
    assert kinds[ref.BLOCKED] >= 16 and kinds[ref.FREE] >= 8 and kinds[ref.EMBEDDED] >= 8, kinds
    assert (E["t"][E["kind"] == ref.BLOCKED] > f32(0.99)).sum() >= 8          # blocked by the box one float inside the hull's end


def test_region_512_across_a_scrolled_seam():
    """Region 512 with lr != 0: the entities and the sweeps stand where the window's texels wrap in x and y."""
    R, lr = 512, (48, -16, 32)
    rng = np.random.default_rng(51)
    mine = np.full((R, R, R), 7, dtype=np.uint8)
    mats = np.zeros((R, R, R), dtype=np.uint32)
    mine[32:200], mats[32:200] = 0, 0x00012345              # texel z 32 .. 199 is world z -224 .. -57: the floor's top is z = -56
    for _ in range(200):                                      # pillars round the seam's corner, texels (0, 0) +- 24
        x, y = rng.integers(-24, 24, 2)
        top = 200 + int(rng.integers(1, 4))
        mine[200:top, y % R, x % R], mats[200:top, y % R, x % R] = 0, 0x00054321
    occ = sr.Occupancy(mats, mine, lr, R)
    centre = (float(lr[0] - R // 2 + (0 - lr[0]) % R), float(lr[1] - R // 2 + (0 - lr[1]) % R), -56.0)   # the world voxel of texel (0, 0): (256, -256)
    with render.Context(render.make_config(64, 40, region=R)) as ctx:
        ctx.upload_world(mats.reshape(-1), mine.reshape(-1))
        ids = [ctx.stamp_create(*sets.stamp_arrays(*spec)) for spec in sets.SPECS]
        stamps = sets.stamps_by_id(ids)
        c = sets.seeded(52, 130, 40, 6, ids, stamps, centre=centre, spread=14.0)
        W, E = check_case(ctx, occ, c, stamps, "region 512", lr)
    kinds = np.bincount(W["kind"], minlength=4)
    assert kinds[sr.BLOCKED] >= 10 and kinds[sr.FREE] >= 10, kinds
    assert (E["entity"] != ref.NONE).sum() >= 20
    tex = W["texel"][W["kind"] == sr.BLOCKED]
    assert (tex[:, 0] < 64).any() and (tex[:, 0] > 448).any() and (tex[:, 1] < 64).any() and (tex[:, 1] > 448).any()   # both sides of the seam


def test_an_edit_between_two_calls_needs_no_sync(arena):
    """A sweep that an entity blocks, rt_edit_voxels placing a voxel nearer in its path, the same call again — enqueued with no host
    wait: the first answer reports the entity, the second leaves it to the world."""
    ctx, occ, ids, stamps, _ = arena
    lo, hi, m = f32([60.5, 60.5, 0.25]), f32([61.0, 61.0, 1.0]), f32([4.0, 0.0, 0.0])
    c = {"aim": "edit", "sweeps": ref.make_sweeps([lo], [hi], [m]), "boxes": sets.boxes_of([[64.0, 60.0, 0.0]], [[65.0, 62.0, 2.0]]), "models": None}
    texel = (62 + 128, 60 + 128, 0 + 128)
    mine2, mats2 = occ.minefield.copy(), occ.materials.copy()
    mine2[texel[2], texel[1], texel[0]], mats2[texel[2], texel[1], texel[0]] = 0, 0x00ABCDEF
    W0, E0 = ref.sweep_entities(occ, c["sweeps"], c["boxes"], None, stamps)
    W1, E1 = ref.sweep_entities(sr.Occupancy(mats2, mine2, (0, 0, 0), 256), c["sweeps"], c["boxes"], None, stamps)
    assert E0[0]["entity"] == ref.BOX and E0[0]["kind"] == ref.BLOCKED and W0[0]["kind"] == sr.FREE
    assert E1[0]["entity"] == ref.NONE and W1[0]["kind"] == sr.BLOCKED and W1[0]["material"] == 0x00ABCDEF
    sweeps, boxes = _dev(c["sweeps"]), _dev(c["boxes"])
    wa, ea, wb, eb = _out(1, 64), _out(1, 80), _out(1, 64), _out(1, 80)
    try:
        ctx.sweep_entities_async(sweeps, boxes, None, wa, ea)
        ctx.edit_voxels([texel], [0x00ABCDEF], [1])          # no host wait between the calls and the edit
        ctx.sweep_entities_async(sweeps, boxes, None, wb, eb)
        ctx.sync()
        view = lambda t, d: t.cpu().numpy().view(d).reshape(-1)
        same_records(view(wa, render.SWEEP_HIT_DTYPE), W0, "before the edit: world")
        same_records(view(ea, abi.ENTITY_SWEEP_HIT_DTYPE), E0, "before the edit: entities")
        same_records(view(wb, render.SWEEP_HIT_DTYPE), W1, "after the edit: world")
        same_records(view(eb, abi.ENTITY_SWEEP_HIT_DTYPE), E1, "after the edit: entities")
    finally:
        ctx.edit_voxels([texel], [0], [0])                   # the arena is the module's: take the voxel out again
        ctx.sync()
    same_records(ctx.sweep_entities(c["sweeps"], (0, 0, 0), c["boxes"], None)[1], E0, "the voxel removed again")


def test_async_behind_a_capture_needs_no_sync(arena):
    """rt_stamp_capture of a piece of the pillar field and at once, with no host wait, sweeps against that stamp drawn as a model
    elsewhere; then rt_stamp_destroy at once: the answers are the captured voxels'."""
    ctx, occ, ids, stamps, _ = arena
    lo_t, ext = (128 - 8, 128 - 8, 128 - 2), (16, 16, 6)
    mats, state = se.capture(occ.materials, occ.minefield, lo_t, ext, 0)
    assert (state == se.SOLID).sum() > 16 * 16 * 2 and (state != se.SOLID).sum() > 100
    sid = ctx.stamp_capture(lo_t, ext)
    try:
        model = sets.models_of(sid, [[40.25, 50.5, 3.0]], 0.5, 13)
        both = dict(stamps)
        both[sid] = (mats, state)
        sweeps = sets.sweeps_at(61, 96, None, model, both)
        n = sweeps.size
        dev, wh, eh = _dev(sweeps), _out(n, 64), _out(n, 80)
        ctx.sweep_entities_async(dev, None, model, wh, eh)
    finally:
        ctx.stamp_destroy(sid)                                 # waits for the enqueued call
    ctx.sync()
    W, E = ref.sweep_entities(occ, sweeps, None, model, both)
    same_records(wh.cpu().numpy().view(render.SWEEP_HIT_DTYPE).reshape(-1), W, "behind a capture: world")
    same_records(eh.cpu().numpy().view(abi.ENTITY_SWEEP_HIT_DTYPE).reshape(-1), E, "behind a capture: entities")
    assert (E["entity"] == ref.MODEL).sum() >= 20


def test_refusals(arena):
    ctx, occ, ids, stamps, cases = arena
    lib = render._lib.amd()
    lr = (C.c_int32 * 3)(0, 0, 0)
    c = cases[-4]                                            # (63 sweeps, 63 boxes, 3 models)
    n = 4
    recs, boxes, models = c["sweeps"][:n].copy(), c["boxes"][:1].copy(), sets.models_of(ids[0], [[0.0, 0.0, 0.0]], 1.0)
    out = np.full(n * 80, 0x5A, dtype=np.uint8)
    wout = np.full(n * 64, 0x5A, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with render.Context(render.make_config(64, 40)) as empty:          # no world resident
        assert lib.rt_sweep_entities(empty.handle, p(recs), n, lr, p(boxes), 1, None, 0, p(wout), p(out)) == abi.RT_ERR_NOT_READY
        assert lib.rt_sweep_entities(empty.handle, p(recs), 0, lr, p(boxes), 1, None, 0, p(wout), p(out)) == abi.RT_OK
    h = ctx.handle
    for fn in (lib.rt_sweep_entities, lib.rt_sweep_entities_async):
        assert fn(None, p(recs), n, lr, p(boxes), 1, None, 0, p(wout), p(out)) == abi.RT_ERR_INVALID_ARG
        assert fn(h, None, 0, None, None, 0, None, 0, None, None) == abi.RT_OK
        assert fn(h, p(recs), (1 << 24) + 1, lr, p(boxes), 1, None, 0, None, p(out)) == abi.RT_ERR_INVALID_ARG
        assert fn(h, p(recs), n, lr, p(boxes), 4097, None, 0, None, p(out)) == abi.RT_ERR_INVALID_ARG
        assert fn(h, p(recs), n, lr, None, 0, p(models), 4097, None, p(out)) == abi.RT_ERR_INVALID_ARG
        assert fn(h, None, n, lr, p(boxes), 1, None, 0, None, p(out)) == abi.RT_ERR_INVALID_ARG
        assert fn(h, p(recs), n, None, p(boxes), 1, None, 0, None, p(out)) == abi.RT_ERR_INVALID_ARG
        assert fn(h, p(recs), n, lr, p(boxes), 1, None, 0, None, None) == abi.RT_ERR_INVALID_ARG
        assert fn(h, p(recs), n, lr, None, 1, None, 0, None, p(out)) == abi.RT_ERR_INVALID_ARG
        assert fn(h, p(recs), n, lr, None, 0, None, 1, None, p(out)) == abi.RT_ERR_INVALID_ARG
        for field, value in (("stamp", 0x7FFFFFFF), ("orient", 48), ("scale", 0.001), ("reserved", 1)):
            bad = models.copy()
            bad[field] = value
            assert fn(h, p(recs), n, lr, None, 0, p(bad), 1, None, p(out)) == abi.RT_ERR_INVALID_ARG, field
    assert lib.rt_sweep_entities_async(h, p(recs), n, lr, None, 0, None, 0, None, p(out)) == abi.RT_ERR_INVALID_ARG      # host addresses
    nan = recs.copy()
    nan["lo"][2, 1] = np.nan
    assert lib.rt_sweep_entities(h, p(nan), n, lr, p(boxes), 1, None, 0, p(wout), p(out)) == abi.RT_ERR_INVALID_ARG      # a sweep outside the domain
    flat = boxes.copy()
    flat["hi"][0, 2] = flat["lo"][0, 2]
    assert lib.rt_sweep_entities(h, p(recs), n, lr, p(flat), 1, None, 0, p(wout), p(out)) == abi.RT_ERR_INVALID_ARG     # an invalid box
    ctx.sync()
    assert (out == 0x5A).all() and (wout == 0x5A).all()
    # the device skips the invalid box and the rest answers as if it were not there
    two = np.concatenate([flat, c["boxes"][1:]])
    _, ae = run_async(ctx, {"sweeps": c["sweeps"], "boxes": two, "models": None})
    keep = c["boxes"].copy()
    keep["lo"][0], keep["hi"][0] = 1000.0, 1001.0            # (the same indices, the first box out of everybody's way)
    same_records(ae, ref.sweep_entities(occ, c["sweeps"], keep, None, stamps)[1], "an invalid box is skipped")
    with pytest.raises(ValueError):
        ctx.sweep_entities_async(torch.zeros((4, 48), dtype=torch.uint8), None, None, None, _out(4, 80))
    with pytest.raises(ValueError):
        ctx.sweep_entities_async(_dev(recs), None, None, _out(4, 48), _out(4, 80))


def test_move_box_entities_stands_on_a_platform_and_stops_at_a_mob(arena):
    """The controller loop: a player that falls lands on a model's top face and not on the floor below it, slides along it, and
    stops at a mob's box; its own box in the list is ignored."""
    ctx, occ, ids, stamps, _ = arena
    platform = sets.models_of(ids[2], [[70.0, 70.0, 2.0]], 1.0, 0)      # the solid 3 x 11 x 4 stamp: top face at z = 6
    player = ([70.5, 71.0, 6.5], [71.1, 71.6, 8.3])
    boxes = sets.boxes_of([player[0], [70.25, 74.0, 6.0]], [player[1], [71.75, 75.0, 8.0]])
    lo, hi, hits = ctx.move_box_entities(player[0], player[1], (0.0, 4.0, -1.0), boxes=boxes, models=platform, self_box=0)
    assert [int(e["entity"]) for _, e in hits] == [abi.RT_ENTITY_MODEL, abi.RT_ENTITY_BOX] and lo[2] == 6.0 and hi[1] == 74.0
    assert hits[0][1]["axis"] == 2 and hits[1][1]["axis"] == 1 and hits[1][1]["index"] == 1
    _, _, alone = ctx.move_box_entities(player[0], player[1], (0.0, 4.0, -1.0), boxes=boxes, models=platform)
    assert alone[0][1]["kind"] == abi.RT_SWEEP_EMBEDDED and alone[0][1]["index"] == 0 and len(alone) == 1
