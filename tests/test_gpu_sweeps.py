"""Box sweeps on the GPU: every field of every hit equals the restatement (tests/sweep_ref.py) bit for bit, on the input sets whose
conditions tests/test_sweep_contract.py asserts — the procedural region, a scrolled window, region 512, an arbitrary-minefield
world, partial workgroups — and the call contract: the asynchronous call, records outside the validated domain, ordering against
rt_edit_voxels, the refusals, tile-split contexts and another RtKernel."""
import ctypes as C

import numpy as np
import pytest
import torch

from raytrace_amd import abi, render, world
from tests import adversarial_worlds as aw
from tests import scenes
from tests import sweep_ref as sr
from tests import test_sweep_contract as tc

pytestmark = pytest.mark.gpu


def _ctx(mats, mine, R=256, **kw):
    """A context with the region resident."""
    ctx = render.Context(render.make_config(64, 40, region=R, **kw))
    ctx.upload_world(mats, mine)
    return ctx


def _same(got, want):
    """GPU hit records against the restatement's, byte for byte."""
    assert got.dtype.itemsize == want.dtype.itemsize == 64 and len(got) == len(want)
    for i in range(len(want)):
        assert got[i].tobytes() == want[i].tobytes(), (i, got[i], want[i])


def _device(sweeps):
    """(sweeps, hits) device tensors of a float32[N, 3, 3] batch; the hits are filled with 0xEE bytes."""
    recs = render.make_sweeps(sweeps)
    dev = torch.from_numpy(recs.view(np.uint8).reshape(-1, 48).copy()).cuda()
    hits = torch.full((recs.size, 64), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return dev, hits


def _records(hits):
    return hits.cpu().numpy().view(render.SWEEP_HIT_DTYPE).reshape(-1)


@pytest.fixture(scope="module")
def terrain(procedural_region):
    """The procedural region at lr = 0 with the 4096-sweep batch and the restatement's hits, computed once."""
    mats, mine = procedural_region
    occ = sr.Occupancy(mats, mine, (0, 0, 0), 256)
    sweeps = tc.surface_sweeps(occ, **tc.TERRAIN_BATCH)
    return mats, mine, occ, sweeps, sr.sweep_batch(occ, sweeps)


def test_terrain_batch_and_partial_workgroups(terrain):
    mats, mine, occ, sweeps, want = terrain
    with _ctx(mats, mine) as ctx:
        _same(ctx.sweep_boxes(sweeps), want)
        for n in (1, 255, 257):
            _same(ctx.sweep_boxes(sweeps[:n]), want[:n])
        assert ctx.sweep_boxes(sweeps[:0]).size == 0


def test_scrolled_window():
    lr = (48, -16, 32)
    mats, mine = world.toroidal_region(lr)
    occ = sr.Occupancy(mats, mine, lr, 256)
    sweeps = tc.surface_sweeps(occ, 2048, 43)
    want = sr.sweep_batch(occ, sweeps)
    kinds = np.bincount(want["kind"], minlength=4)
    assert kinds[sr.FREE] > 400 and kinds[sr.BLOCKED] > 400 and kinds[sr.EMBEDDED] > 50
    with _ctx(mats, mine) as ctx:
        _same(ctx.sweep_boxes(sweeps, lr), want)


def test_region_512(native_built):
    R = 512
    mats, mine = world.generate_region(world.DEFAULT_SEED, region=R)
    occ = sr.Occupancy(mats, mine, (0, 0, 0), R)
    sweeps = tc.surface_sweeps(occ, 1024, 47)
    want = sr.sweep_batch(occ, sweeps)
    kinds = np.bincount(want["kind"], minlength=4)
    assert kinds[sr.FREE] > 200 and kinds[sr.BLOCKED] > 200 and kinds[sr.EMBEDDED] > 20
    assert (want["texel"].max(axis=0) >= 256).all()          # texels beyond what region 256 addresses
    with _ctx(mats, mine, R=R) as ctx:
        _same(ctx.sweep_boxes(sweeps), want)


def test_arbitrary_minefield_world():
    """Minefield values 0..30 that bound no distance (the fuzz scenes' world): only the byte 0 is occupied, whatever the rest says."""
    mats, mine, _, _ = aw.arbitrary_world(256, seed=3)
    occ = sr.Occupancy(mats, mine, (0, 0, 0), 256)
    sweeps = tc.scene_sweeps(occ, 1024, 9)
    want = sr.sweep_batch(occ, sweeps)
    kinds = np.bincount(want["kind"], minlength=4)
    assert kinds[sr.FREE] > 200 and kinds[sr.BLOCKED] > 100 and kinds[sr.EMBEDDED] > 20
    with _ctx(mats.reshape(-1), mine.reshape(-1)) as ctx:
        _same(ctx.sweep_boxes(sweeps), want)


def test_async_equals_sync_and_marks_out_of_domain_records(terrain):
    """The asynchronous call on device buffers gives the synchronous call's bytes; with 8 records outside the validated domain it
    gives RT_SWEEP_INVALID for exactly those and the right hits for the rest, and the synchronous call rejects that batch and
    leaves `hits` untouched."""
    mats, mine, occ, sweeps, want = terrain
    n = 777
    bad = sweeps[:n].copy()
    bad[3, 0, 0] = np.nan                                    # a NaN, an inf, hi <= lo, an extent of 9, a motion of 65, a coordinate of 2^23
    bad[100, 2, 1] = np.inf
    bad[255, 1, 2] = bad[255, 0, 2]
    bad[256, 1, 0] = bad[256, 0, 0] + np.float32(9.0)
    bad[300, 2, 2] = 65.0
    bad[511, 0, 1], bad[511, 1, 1] = 2.0 ** 23, 2.0 ** 23 + 1
    bad[640, 1, 1] = -np.inf
    bad[776, 2, 0] = np.nan
    which = [3, 100, 255, 256, 300, 511, 640, 776]
    want_bad = sr.sweep_batch(occ, bad)
    assert sorted(np.flatnonzero(want_bad["kind"] == sr.INVALID)) == which
    good = np.setdiff1d(np.arange(n), which)
    assert want_bad[good].tobytes() == want[:n][good].tobytes()
    with _ctx(mats, mine) as ctx:
        dev, hits = _device(sweeps[:n])
        ctx.sweep_boxes_async(dev, hits)
        dev_bad, hits_bad = _device(bad)
        ctx.sweep_boxes_async(dev_bad, hits_bad)
        ctx.sync()
        _same(_records(hits), want[:n])
        _same(_records(hits_bad), want_bad)
        recs = render.make_sweeps(bad)
        out = np.full(n * 64, 0x5A, dtype=np.uint8)
        lr = (C.c_int32 * 3)(0, 0, 0)
        rc = ctx._lib.rt_sweep_boxes(ctx.handle, recs.ctypes.data_as(C.c_void_p), n, lr, out.ctypes.data_as(C.c_void_p))
        assert rc == abi.RT_ERR_INVALID_ARG and (out == 0x5A).all()
        for i in which:                                      # each of them alone is rejected too
            with pytest.raises(render.RtError) as e:
                ctx.sweep_boxes(bad[i:i + 1])
            assert e.value.code == abi.RT_ERR_INVALID_ARG
        _same(ctx.sweep_boxes(sweeps[:n]), want[:n])         # a rejected call changed nothing


def test_refusals(terrain):
    mats, mine, occ, sweeps, want = terrain
    lib = render._lib.amd()
    lr = (C.c_int32 * 3)(0, 0, 0)
    recs = render.make_sweeps(sweeps[:4])
    out = np.full(4 * 64, 0x5A, dtype=np.uint8)
    p_in, p_out = recs.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    with render.Context(render.make_config(64, 40)) as ctx:  # no world resident
        assert lib.rt_sweep_boxes(ctx.handle, p_in, 4, lr, p_out) == abi.RT_ERR_NOT_READY
        assert lib.rt_sweep_boxes(ctx.handle, p_in, 0, lr, p_out) == abi.RT_OK
    with _ctx(mats, mine) as ctx:
        h = ctx.handle
        assert lib.rt_sweep_boxes(h, None, 0, None, None) == abi.RT_OK
        assert lib.rt_sweep_boxes_async(h, None, 0, None, None) == abi.RT_OK
        for fn in (lib.rt_sweep_boxes, lib.rt_sweep_boxes_async):
            assert fn(h, p_in, (1 << 24) + 1, lr, p_out) == abi.RT_ERR_INVALID_ARG
            assert fn(h, None, 4, lr, p_out) == abi.RT_ERR_INVALID_ARG
            assert fn(h, p_in, 4, None, p_out) == abi.RT_ERR_INVALID_ARG
            assert fn(h, p_in, 4, lr, None) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_sweep_boxes_async(h, p_in, 4, lr, p_out) == abi.RT_ERR_INVALID_ARG      # host addresses
        buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        base = buf.data_ptr()
        assert lib.rt_sweep_boxes_async(h, C.c_void_p(base + 4), 1, lr, C.c_void_p(base + 1024)) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_sweep_boxes_async(h, C.c_void_p(base), 1, lr, C.c_void_p(base + 1032)) == abi.RT_ERR_INVALID_ARG
        ctx.sync()
        assert not buf.any().item() and (out == 0x5A).all()
        _same(ctx.sweep_boxes(sweeps[:4]), want[:4])


def test_an_edit_between_two_sweeps_needs_no_sync(terrain):
    """A sweep that is FREE, rt_edit_voxels placing a block in its path, the same sweep again — all enqueued without a host wait: the
    first answer is FREE, the second BLOCKED at that block."""
    mats, mine, occ, sweeps, want = terrain
    for i in range(len(want)):
        s = sweeps[i:i + 1]
        if want[i]["kind"] != sr.FREE or abs(s[0, 2, 0]) < 1.0 or tc.has_aligned_face(s[0]):
            continue
        face = s[0, 1, 0] if s[0, 2, 0] > 0 else s[0, 0, 0]
        half = s[0, 2] * np.float32(0.5)                     # a voxel the box overlaps half way: the one its leading x face is in
        v = (int(np.floor(face + half[0])), int(np.floor(s[0, 0, 1] + half[1])), int(np.floor(s[0, 0, 2] + half[2])))
        texel = occ.texel(v)
        if texel is not None:
            break
    assert not occ.occupied(v)
    word = 0x00ABCDEF
    mine2 = occ.minefield.copy()
    mats2 = occ.materials.copy()
    mine2[texel[2], texel[1], texel[0]] = 0
    mats2[texel[2], texel[1], texel[0]] = word
    after = sr.sweep_batch(sr.Occupancy(mats2, mine2, (0, 0, 0), 256), s)
    assert after[0]["kind"] in (sr.BLOCKED, sr.EMBEDDED) and tuple(after[0]["texel"]) == texel and after[0]["material"] == word
    with _ctx(mats, mine) as ctx:
        dev, hits_a = _device(s)
        _, hits_b = _device(s)
        ctx.sweep_boxes_async(dev, hits_a)
        ctx.edit_voxels([texel], [word], [1])                # no host wait between the sweeps and the edit
        ctx.sweep_boxes_async(dev, hits_b)
        ctx.sync()
        _same(_records(hits_a), want[i:i + 1])
        _same(_records(hits_b), after)
        _same(ctx.sweep_boxes(s), after)


def test_move_and_slide_down_the_staircase(native_built):
    mats, mine = world.region_from_ids(scenes.staircase_ids())
    occ = sr.Occupancy(mats, mine, (0, 0, 0), 256)
    lo = np.float32([-3.7, 10.2, tc.surface_heights(occ)[138, 124] + 0.5])
    hi = lo + tc.PLAYER
    glo, ghi = lo.copy(), hi.copy()
    blocked = 0
    with _ctx(mats, mine) as ctx:
        for _ in range(24):
            lo, hi, want = sr.move_and_slide(occ, lo, hi, (-0.9, 0.1, -1.3))
            glo, ghi, got = ctx.move_and_slide(glo, ghi, (-0.9, 0.1, -1.3))
            assert len(got) == len(want)
            for g, w in zip(got, sr.pack(want)):
                assert g.tobytes() == w.tobytes(), (g, w)
            assert np.float32(lo).tobytes() == glo.tobytes() and np.float32(hi).tobytes() == ghi.tobytes()
            blocked += sum(w["kind"] == sr.BLOCKED for w in want)
    assert blocked >= 12 and lo[2] < -4     # (a walker on a step is stopped by it every tick)


def test_tile_contexts_and_other_kernels_answer_the_same(terrain):
    mats, mine, occ, sweeps, want = terrain
    n = 600
    for kw in (dict(tile_world=2, tile_rank=1), dict(kernel=abi.RT_KERNEL_PERSISTENT), dict(kernel=abi.RT_KERNEL_MEGA)):
        with _ctx(mats, mine, **kw) as ctx:
            _same(ctx.sweep_boxes(sweeps[:n]), want[:n])
