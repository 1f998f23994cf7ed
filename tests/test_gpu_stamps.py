"""The voxel stamps on the GPU (rt_stamp_*, rt_edit_stamps), against the numpy restatement of tests/stamp_edits.py and the oracle: the
touched chunks byte for byte (rt_read_box) and the nibble maps (RT_SELFTEST_SCENE_MAPS) after stamp batches at R = 256 and 512, on the
generated world and on arbitrary minefield values (which show the chunks that were rebuilt); capture and undo; equivalence with
rt_edit_voxels; frames and picks on the pasted world; stream ordering against frames in flight and on a caller's stream; the
accumulation reset and the boxes kept for a history that goes on; rejections, ids and device_bytes."""
import ctypes as C

import numpy as np
import pytest

from raytrace_amd import abi, render, world
from oracle import pyoracle as po
from tests import edit_history_ref as er
from tests import shape_edits as se
from tests import stamp_edits as st
from tests.test_gpu_accumulation import _peek
from tests.test_gpu_edit_history import _ctx as _history_ctx, _frame as _history_frame
from tests.test_gpu_parity import _compare
from tests.test_gpu_shape_edits import _arbitrary_region

pytestmark = pytest.mark.gpu

MAPS = abi.RT_SELFTEST_SCENE_MAPS
CACHE = abi.RT_FLAG_CACHE_PRIMARY
W, H = 64, 64
POSE = dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.25, sun=0.3)


def _u(seed=3, **kw):
    p = dict(POSE)
    p.update(kw)
    return po.camera_uniforms(p["origin"], p["heading"], p["pitch"], p["sun"], seed)


def _ctx(region, noise=None, R=256, **kw):
    ctx = render.Context(render.make_config(W, H, region=R, **kw))
    ctx.upload_world(*region)
    if noise is not None:
        ctx.upload_noise(noise)
    return ctx


@pytest.fixture(scope="module")
def regions(procedural_region):
    made = {("generated", 256): procedural_region}

    def get(kind, R):
        if (kind, R) not in made:
            made[(kind, R)] = world.generate_region(world.DEFAULT_SEED, region=R) if kind == "generated" else _arbitrary_region(R)
        return made[(kind, R)]
    return get


# ---- stamps -----------------------------------------------------------------------------------------------------------------------
def _random_stamp(E, seed, absent=0.3):
    """States drawn at random (about `absent` of them ABSENT, the rest AIR or SOLID alike) and words with no order in them."""
    rng = np.random.default_rng(seed)
    ex, ey, ez = E
    r = rng.random((ez, ey, ex))
    state = np.where(r < absent, st.ABSENT, np.where(r < absent + (1 - absent) / 2, st.AIR, st.SOLID)).astype(np.uint8)
    mats = rng.integers(1, 2 ** 32, size=state.shape, dtype=np.uint64).astype(np.uint32)
    return mats, state


def _tree():
    """A trunk with a crown, 9 x 9 x 12: everything else of its box is ABSENT."""
    state = np.zeros((12, 9, 9), np.uint8)
    state[:7, 4, 4] = st.SOLID
    state[6:12, 1:8, 1:8] = st.SOLID
    state[7:11, 0, 3:6] = state[7:11, 8, 3:6] = state[7:11, 3:6, 0] = state[7:11, 3:6, 8] = st.SOLID
    mats = np.where(state != 0, 0x5000 + np.arange(state.size, dtype=np.uint32).reshape(state.shape), 0xDEAD).astype(np.uint32)
    return mats, state


def _solid(E, word):
    ex, ey, ez = E
    return np.full((ez, ey, ex), word, np.uint32), np.full((ez, ey, ex), st.SOLID, np.uint8)


class Stamps:
    """The stamps of one context beside their numpy copies: `model` maps an id to (materials, state)."""

    def __init__(self, ctx):
        self.ctx, self.model = ctx, {}

    def create(self, pair):
        sid = self.ctx.stamp_create(*pair)
        assert sid != 0 and sid not in self.model and self.ctx.stamp_info(sid) == st.extent_of(pair[1])
        self.model[sid] = pair
        return sid

    def paste(self, mats, mine, places):
        """The batch on the context and on the model's region; returns the touched chunks."""
        places = st.batch(places)
        assert st.PLACE_DTYPE == render.STAMP_PLACE_DTYPE
        touched = st.apply_stamps(mats, mine, self.model, places)
        self.ctx.edit_stamps(places)
        return touched


def _check_chunks(ctx, mats, mine, chunks, what):
    for (cx, cy, cz) in chunks:
        gm, gf = ctx.read_box((64 * cx, 64 * cy, 64 * cz), (64, 64, 64))
        sl = (slice(64 * cz, 64 * cz + 64), slice(64 * cy, 64 * cy + 64), slice(64 * cx, 64 * cx + 64))
        assert np.array_equal(gf, mine[sl]), "%s: chunk %s: minefield differs at %d voxels" % (what, (cx, cy, cz), int(np.count_nonzero(gf != mine[sl])))
        assert np.array_equal(gm, mats[sl]), "%s: chunk %s: materials differ at %d voxels" % (what, (cx, cy, cz), int(np.count_nonzero(gm != mats[sl])))
    assert ctx.selftest(MAPS) == 0, what


def _check_region(ctx, mats, mine, what):
    R = mine.shape[0]
    gm, gf = ctx.read_box((0, 0, 0), (R, R, R))
    assert np.array_equal(gf, mine), "%s: minefield differs at %d voxels" % (what, int(np.count_nonzero(gf != mine)))
    assert np.array_equal(gm, mats), "%s: materials differ at %d voxels" % (what, int(np.count_nonzero(gm != mats)))
    assert ctx.selftest(MAPS) == 0, what


def _surface(mine, x, y):
    """The highest occupied texel of column (x, y), or 100 where it has none."""
    z = np.flatnonzero(mine[:, y, x] == 0)
    return int(z[-1]) if z.size else 100


def _random_places(ids, model, R, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        out.append(st.place(ids[int(rng.integers(0, len(ids)))], rng.integers(-30, R + 10, size=3), int(rng.integers(0, 48)), int(rng.integers(0, 3))))
    return out


def _sequence(ctx, mats, mine, kind, big=True):
    """The batches in the order they are applied: the smallest that can go wrong.  (mats, mine) is the model's region, changed in place."""
    R = mine.shape[0]
    far = R - 1
    s = Stamps(ctx)
    one = s.create(_solid((1, 1, 1), 0x11))
    odd = s.create((np.arange(1, 106, dtype=np.uint32).reshape(7, 3, 5), _random_stamp((5, 3, 7), 1, 0.2)[1]))
    long65 = s.create(_random_stamp((65, 4, 3), 2))
    long70 = s.create(_random_stamp((70, 2, 9), 3))
    tree = s.create(_tree())
    paint = s.create(_solid((20, 20, 20), 0xA2))
    rand = [s.create(_random_stamp(E, 10 + k)) for k, E in enumerate([(3, 3, 3), (17, 5, 2), (2, 33, 4), (8, 8, 8), (1, 6, 40), (64, 1, 1)])]

    def run(name, places, expect=None):
        before = mine.copy() if isinstance(expect, str) else None
        touched = s.paste(mats, mine, places)
        _check_chunks(ctx, mats, mine, touched, name)
        if expect == "untouched":
            assert touched == [] and np.array_equal(before, mine), name
        elif expect is not None:
            assert len(touched) == expect, name
        return touched

    run("a 1 x 1 x 1 stamp", [st.place(one, (5, 6, 7))], 1)
    assert mats[7, 6, 5] == 0x11 and mine[7, 6, 5] == 0
    run("5 x 3 x 7 in all 48 orientations side by side", [st.place(odd, (4 + 10 * (o % 24), 40 + 70 * (o // 24), _surface(mine, 4 + 10 * (o % 24), 40 + 70 * (o // 24)) - 3), o)
                                                       for o in range(48)])
    run("65 x 4 x 3: across a 64-bit row word of the stamp, every stride", [st.place(long65, (60, 120, 60), 0), st.place(long65, (100, 130, 62), 1),
                                                                             st.place(long65, (150, 60, 70), 2 << 3 | 1), st.place(long65, (160, 70, 60), 4 << 3 | 6),
                                                                             st.place(long65, (30, 10, 20), 5 << 3 | 7)])
    run("70 long across a chunk corner, along x, y and z", [st.place(long70, (60, 63, 60), 0), st.place(long70, (190, 60, 126), 2 << 3 | 2),
                                                           st.place(long70, (126, 190, 60), 5 << 3)])
    spots = [(20, 200), (63, 63), (64, 128), (130, 190), (200, 20)]
    run("trees on the terrain: ABSENT voxels, where = AIR", [st.place(tree, (x - 4, y - 4, _surface(mine, x, y) + 1 - 2 * (i & 1)), 8 * (i % 6) | (i & 3), st.WHERE_AIR)
                                                            for i, (x, y) in enumerate(spots)])
    run("paint: where = SOLID", [st.place(paint, (100, 100, _surface(mine, 110, 110) - 10), 0, st.WHERE_SOLID)])
    run("clipped at every face", [st.place(odd, (-2, 100, 100), 3), st.place(odd, (R - 2, 100, 100), 12), st.place(odd, (100, -1, 100), 21),
                                  st.place(odd, (100, R - 1, 100), 30), st.place(odd, (100, 100, -2), 39), st.place(odd, (100, 100, R - 3), 47)], 6)
    run("two overlapping placements in one call: the last wins", [st.place(long70, (40, 200, 90), 0), st.place(paint, (50, 195, 85), 0)])
    run("300 random placements of 6 random stamps", _random_places(rand, s.model, R, 300, R))
    run("wholly outside", [st.place(odd, (R, 0, 0)), st.place(odd, (-5, 0, 0)), st.place(tree, (0, -12, 0), 8), st.place(paint, (10, 10, -4 * R)),
                           st.place(long70, (4 * R, 4 * R, 4 * R), 47)], "untouched")
    _check_region(ctx, mats, mine, "the sequence")
    if big:
        whole = s.create(_random_stamp((256, 256, 256), 99, 0.1))
        run("a 256^3 stamp over the whole region", [st.place(whole, (0, 0, 0), 5 << 3 | 2)], 64)
        _check_region(ctx, mats, mine, "the whole region")
        sm, ss = st.oriented(s.model[whole][0], 42), st.oriented(s.model[whole][1], 42)
        assert np.array_equal(mine == 0, np.where(ss == st.ABSENT, mine == 0, ss == st.SOLID)) and np.array_equal(mats[ss != 0], sm[ss != 0])
    return s


@pytest.mark.parametrize("kind", ["generated", "arbitrary"])
def test_touched_chunks_and_maps_after_stamp_batches(regions, kind):
    mats, mine = (a.copy() for a in regions(kind, 256))
    with _ctx((mats, mine)) as ctx:
        assert ctx.selftest(MAPS) == 0
        _sequence(ctx, mats, mine, kind)


def test_a_sequence_at_512_for_the_brick_map(regions):
    R = 512
    mats, mine = (a.copy() for a in regions("arbitrary", R))
    with _ctx((mats, mine), R=R) as ctx:
        s = Stamps(ctx)
        big = s.create(_random_stamp((256, 100, 70), 7))
        tree = s.create(_tree())
        for name, places in (("a tree on a chunk corner", [st.place(tree, (252, 316, 380), 9, st.WHERE_AIR)]),
                             ("a large stamp turned, and one clipped at the far corner", [st.place(big, (100, 130, 200), 3 << 3 | 5), st.place(big, (400, 450, 470), 0)]),
                             ("wholly outside", [st.place(big, (R, 0, 0))])):
            touched = s.paste(mats, mine, places)
            assert (touched == []) == (name == "wholly outside")
            _check_chunks(ctx, mats, mine, touched, name)
        _check_region(ctx, mats, mine, "R = 512")


# ---- capture ------------------------------------------------------------------------------------------------------------------
def test_capture_equals_the_model_and_is_ordered_with_the_edits(procedural_region):
    mats, mine = (a.copy() for a in procedural_region)
    lo, ext = (37, 80, 60), (91, 70, 83)
    with _ctx(procedural_region) as ctx:
        first, skipped = ctx.stamp_capture(lo, ext), ctx.stamp_capture(lo, ext, abi.RT_STAMP_SKIP_AIR)
        want, want_skipped = st.capture(mats, mine, lo, ext), st.capture(mats, mine, lo, ext, st.SKIP_AIR)
        assert set(np.unique(want[1]).tolist()) == {st.AIR, st.SOLID}                 # the box holds ground and sky
        # an edit enqueued behind the captures, and a capture behind the edit: nothing is synchronised in between
        shapes = se.batch([se.sphere((160, 230, 200), 60 * 60, 0x31, 0), se.box((40, 85, 70), (90, 90, 150), 0x32, 1)])
        ctx.edit_shapes(shapes)
        after = ctx.stamp_capture(lo, ext)
        assert ctx.stamp_info(after) == ext and len({first, skipped, after}) == 3
        se.apply_shapes(mats, mine, shapes)
        want_after = st.capture(mats, mine, lo, ext)
        assert not np.array_equal(want_after[1], want[1])
        for sid, (wm, ws) in ((first, want), (skipped, want_skipped), (after, want_after)):
            gm, gs = ctx.stamp_read(sid)
            assert np.array_equal(gs, ws) and np.array_equal(gm, wm)
        assert not want_skipped[0][want_skipped[1] == st.ABSENT].any() and (want_skipped[1] != st.AIR).all()
        # a capture changes nothing the renderer reads
        _check_region(ctx, mats, mine, "after the captures")
        # the single-array reads
        only_m, only_s = np.empty_like(want[0]), np.empty_like(want[1])
        lib = render._lib.amd()
        assert lib.rt_stamp_read(ctx.handle, first, only_m.ctypes.data_as(C.c_void_p), None) == abi.RT_OK and np.array_equal(only_m, want[0])
        assert lib.rt_stamp_read(ctx.handle, first, None, only_s.ctypes.data_as(C.c_void_p)) == abi.RT_OK and np.array_equal(only_s, want[1])


def test_undo_restores_the_region_byte_for_byte(procedural_region):
    mats, mine = procedural_region
    lo, ext = (70, 50, 90), (100, 120, 90)
    with _ctx(procedural_region) as ctx:
        saved = ctx.stamp_capture(lo, ext)
        crater = se.batch([se.sphere((240, 220, 270), 80 * 80, 0, 0), se.sphere((240, 220, 270), 84 * 84, 0x666, 1, se.SOLID)])
        ctx.edit_shapes(crater)
        m2, f2 = mats.copy(), mine.copy()
        se.apply_shapes(m2, f2, crater)
        assert not np.array_equal(f2, mine)
        _check_chunks(ctx, m2, f2, [(1, 1, 1), (2, 2, 2)], "the crater")
        ctx.edit_stamps([render.stamp_place(saved, lo)])
        _check_region(ctx, mats, mine, "after the undo")


def test_a_captured_stamp_pasted_turned_elsewhere(regions):
    mats, mine = (a.copy() for a in regions("arbitrary", 256))
    lo, ext = (10, 20, 30), (40, 9, 66)
    with _ctx((mats, mine)) as ctx:
        s = Stamps(ctx)
        sid = ctx.stamp_capture(lo, ext, abi.RT_STAMP_SKIP_AIR)
        s.model[sid] = st.capture(mats, mine, lo, ext, st.SKIP_AIR)
        touched = s.paste(mats, mine, [st.place(sid, (150, 100, 60), 3 << 3 | 4), st.place(sid, (60, 180, 200), 4 << 3 | 3, st.WHERE_AIR)])
        assert len(touched) >= 6
        _check_chunks(ctx, mats, mine, touched, "captured and turned")
        _check_region(ctx, mats, mine, "captured and turned")


# ---- equivalence --------------------------------------------------------------------------------------------------------------
def test_stamps_equal_the_enumerated_voxel_edits(regions):
    """Two contexts on the same arbitrary world: in every chunk these placements touch they select a voxel, so rt_edit_voxels with
    one record per selected voxel rebuilds the same chunks."""
    mats, mine = regions("arbitrary", 256)
    with _ctx((mats, mine)) as a, _ctx((mats, mine)) as b:
        s = Stamps(a)
        tree, odd, bar = s.create(_tree()), s.create(_random_stamp((5, 3, 7), 4, 0.0)), s.create(_random_stamp((70, 2, 9), 5, 0.0))
        places = st.batch([st.place(tree, (100, 100, 100), 21, st.WHERE_AIR), st.place(odd, (126, 62, 190), 44), st.place(tree, (103, 98, 99), 2, st.WHERE_SOLID),
                           st.place(bar, (60, 60, 60), 19), st.place(odd, (-1, -1, 60), 17), st.place(bar, (200, 250, 250), 1, st.WHERE_AIR)])
        xyz, words, solid, touched = st.enumerate_records(mats, mine, s.model, places)
        assert sorted(set(map(tuple, (xyz >> 6).tolist()))) == touched and len(touched) >= 8
        a.edit_stamps(places)
        b.edit_voxels(xyz, words, solid)
        (am, af), (bm, bf) = a.read_box((0, 0, 0), (256, 256, 256)), b.read_box((0, 0, 0), (256, 256, 256))
        assert np.array_equal(af, bf) and np.array_equal(am, bm) and not np.array_equal(af, mine)
        assert a.selftest(MAPS) == 0


# ---- frames and queries ---------------------------------------------------------------------------------------------------------
def _scene_stamps():
    """(stamp, place arguments): a wall in front of the default camera, a pit in the ground ahead of it and a slab overhead."""
    word = po.lib().rt_oracle_pack_material(200, 120, 60, 0)
    pit = np.zeros((30, 30, 30), np.uint32), np.full((30, 30, 30), st.AIR, np.uint8)
    return [(_solid((20, 1, 15), word), ((88, 38, 223), 0, st.WHERE_ALL)), (pit, ((84, 56, 136), 0, st.WHERE_ALL)),
            (_solid((1, 20, 60), word), ((68, 8, 248), 5 << 3, st.WHERE_AIR))]


def _paste_scene(ctx):
    ids = [ctx.stamp_create(*pair) for pair, _ in _scene_stamps()]
    ctx.edit_stamps([render.stamp_place(sid, *args) for sid, (_, args) in zip(ids, _scene_stamps())])


@pytest.fixture(scope="module")
def pasted_256(procedural_region):
    m2, f2 = (a.copy() for a in procedural_region)
    model = {k + 1: pair for k, (pair, _) in enumerate(_scene_stamps())}
    places = st.batch([st.place(k + 1, *args) for k, (_, args) in enumerate(_scene_stamps())])
    assert len(st.apply_stamps(m2, f2, model, places)) >= 3
    return m2, f2


@pytest.mark.parametrize("spp", [1, 2])
def test_frames_see_the_stamps(procedural_region, blue_noise, pasted_256, spp):
    u = _u()
    cpu, _ = po.render(*pasted_256, blue_noise, u, W, H, spp, 3)
    old, _ = po.render(*procedural_region, blue_noise, u, W, H, spp, 3)
    assert any(not np.array_equal(old[k], cpu[k]) for k in cpu)       # the pose does look at the stamps
    with _ctx(procedural_region, blue_noise, spp=spp, depth=3) as ctx:
        _paste_scene(ctx)
        ctx.draw_frame(u)
        ctx.sync()
        _compare(ctx.readback_all(), cpu)


def test_picks_see_the_stamps(procedural_region, pasted_256):
    u = _u()
    xy = np.array([(W // 2, H // 2), (W // 2 + 1, H // 2), (3, H - 3), (W // 2, 5), (10, 20)])
    with _ctx(procedural_region) as ctx, _ctx(pasted_256) as given:
        before = ctx.pick_pixels(u, xy)
        _paste_scene(ctx)
        after = ctx.pick_pixels(u, xy)
        assert after.tobytes() == given.pick_pixels(u, xy).tobytes() and after.tobytes() != before.tobytes()


# ---- ordering ---------------------------------------------------------------------------------------------------------------
def test_frames_in_flight_see_the_region_of_their_call(procedural_region, blue_noise, pasted_256):
    u = _u()
    with _ctx(procedural_region, blue_noise, spp=3, depth=2, flags=CACHE | abi.RT_FLAG_FRAMES_IN_FLIGHT_2) as ctx:
        ids = [ctx.stamp_create(*pair) for pair, _ in _scene_stamps()]
        ctx.draw_frame(u)
        first = {b: ctx.device_ptr(b) for b in range(abi.RT_BUF_FINAL_BGRA8)}
        ctx.edit_stamps([render.stamp_place(sid, *args) for sid, (_, args) in zip(ids, _scene_stamps())])
        ctx.draw_frame(u)
        assert first != {b: ctx.device_ptr(b) for b in range(abi.RT_BUF_FINAL_BGRA8)}
        ctx.sync()
        second = ctx.readback_all()
        before = _peek(first, W, H)
    _compare(before, po.render(*procedural_region, blue_noise, u, W, H, 3, 2)[0])
    _compare(second, po.render(*pasted_256, blue_noise, u, W, H, 3, 2)[0])


def test_caller_stream_orders_a_paste_between_frames(procedural_region, blue_noise, pasted_256):
    import torch
    import bench
    u = _u()
    s = torch.cuda.Stream(device=0)
    with _ctx(procedural_region, blue_noise, spp=2, depth=2, flags=CACHE) as ctx:
        ctx.set_stream(s.cuda_stream)
        ctx.draw_frame(u)
        first = {}
        for b in range(abi.RT_BUF_FINAL_BGRA8):      # copies enqueued on s before the paste
            dt, ch = abi.BUFFER_FORMATS[b]
            t = torch.as_tensor(bench._DevArray(ctx.device_ptr(b), W * H * ch * np.dtype(dt).itemsize), device=torch.device("cuda", 0))
            with torch.cuda.stream(s):
                first[b] = t.clone()
        _paste_scene(ctx)
        ctx.draw_frame(u)
        ctx.sync()
        s.synchronize()
        second = ctx.readback_all()
        before = {}
        for b, t in first.items():
            dt, ch = abi.BUFFER_FORMATS[b]
            before[abi.BUFFER_NAMES[b]] = t.cpu().numpy().view(dt).reshape((H, W, ch) if ch > 1 else (H, W))
        ctx.set_stream(0)
    _compare(before, po.render(*procedural_region, blue_noise, u, W, H, 2, 2)[0])
    _compare(second, po.render(*pasted_256, blue_noise, u, W, H, 2, 2)[0])


def test_stamps_shapes_and_voxel_edits_apply_in_call_order(procedural_region):
    """Three kinds of change across one chunk, each undoing part of the one before: the staging sets are shared and used in turn."""
    mats, mine = procedural_region
    m2, f2 = mats.copy(), mine.copy()
    xyz = np.stack(np.meshgrid(np.arange(80, 120), np.arange(90, 110), np.arange(70, 100), indexing="ij"), axis=-1).reshape(-1, 3)
    with _ctx(procedural_region) as ctx:
        s = Stamps(ctx)
        block, hole = s.create(_solid((64, 64, 37), 0x51)), s.create((np.zeros((25, 25, 25), np.uint32), np.full((25, 25, 25), st.AIR, np.uint8)))
        s.paste(m2, f2, [st.place(block, (64, 64, 64))])
        ctx.edit_voxels(xyz, np.full(len(xyz), 0x53, np.uint32), np.zeros(len(xyz), bool))
        from tests import voxel_edits as ve
        ve.apply_edits(m2, f2, xyz, np.full(len(xyz), 0x53, np.uint32), np.zeros(len(xyz), bool))
        s.paste(m2, f2, [st.place(hole, (85, 85, 80), 0, st.WHERE_SOLID)])
        shape = se.batch([se.box((64, 64, 64), (127, 127, 70), 0x54, 1, se.AIR)])
        ctx.edit_shapes(shape)
        se.apply_shapes(m2, f2, shape)
        s.paste(m2, f2, [st.place(block, (70, 60, 95), 2 << 3)])
        _check_region(ctx, m2, f2, "call order")


# ---- accumulation and history ---------------------------------------------------------------------------------------------------
def test_a_touching_paste_restarts_the_accumulation_and_no_other(procedural_region, blue_noise, pasted_256):
    seed, spp = 11, 1
    with _ctx(procedural_region, blue_noise, spp=spp, depth=2, flags=CACHE | abi.RT_FLAG_ACCUMULATE) as ctx:
        ids = [ctx.stamp_create(*pair) for pair, _ in _scene_stamps()]
        outside = [render.stamp_place(ids[0], (256, 0, 0)), render.stamp_place(ids[1], (0, -30, 0))]
        ctx.draw_frame(_u(seed))
        ctx.draw_frame(_u(seed + 1))
        assert ctx.accumulation() == (2, 2)
        ctx.edit_stamps([])                                           # count == 0
        ctx.edit_stamps(outside)                                      # no chunk is touched
        captured = ctx.stamp_capture((0, 0, 0), (9, 9, 9))            # a capture resets nothing
        ctx.draw_frame(_u(seed + 2))
        assert ctx.accumulation() == (3, 3)
        ctx.edit_stamps([render.stamp_place(sid, *args) for sid, (_, args) in zip(ids, _scene_stamps())])
        ctx.draw_frame(_u(seed + 3))
        assert ctx.accumulation() == (1, 1)
        ctx.sync()
        got = ctx.readback_all()
        ctx.stamp_destroy(captured)
        ctx.edit_stamps(outside)
        ctx.draw_frame(_u(seed + 4))
        assert ctx.accumulation() == (2, 2)
        # a chunk that is touched though nothing in it is selected restarts the sum as well
        ctx.edit_stamps([render.stamp_place(ids[0], (0, 0, 250), 0, abi.RT_WHERE_SOLID)])
        ctx.draw_frame(_u(seed + 5))
        assert ctx.accumulation() == (1, 1)
    _compare(got, po.render(*pasted_256, blue_noise, _u(seed + 3), W, H, 1, 2)[0])


def _walk_stamps(ctx, walk, s, places):
    """The placements on the context and on edit_history_ref's Walk: the restatement's world, and its pending boxes put into the
    history's set by rt_edit_voxels' rule (a call that touches nothing leaves it alone; more than sixteen empty and mark it)."""
    if not walk.owned:
        walk.mats, walk.mine, walk.owned = walk.mats.copy(), walk.mine.copy(), True
    s.paste(walk.mats, walk.mine, places)
    h, new = walk.h, st.pending_boxes(s.model, st.batch(places), walk.R)
    if new and h.radius == 0:
        h.valid = False
    elif new and not h.overflowed:
        if len(h.boxes) + len(new) > er.MAX_BOXES:
            h.boxes, h.overflowed = [], True
        else:
            h.boxes += new
    assert ctx.edit_boxes_pending() == h.pending()


def test_a_kept_history_takes_one_box_per_placement(procedural_region, blue_noise):
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, er.RADIUS)
    ops = er.main_ops()
    modes = []
    with _history_ctx(procedural_region, blue_noise) as ctx:
        s = Stamps(ctx)
        # the pillar of the main sequence lying on its side in the stamp (10 x 3 x 3), stood up by the placement; a dent beside it
        pillar = s.create(_solid((er.PILLAR[5], er.PILLAR[3], er.PILLAR[4]), er.WORD))
        dent = s.create((np.zeros((3, 3, 3), np.uint32), np.full((3, 3, 3), st.AIR, np.uint8)))
        outside = [st.place(pillar, (256, 0, 0)), st.place(dent, (40, -3, 41))]
        batch = [st.place(pillar, er.PILLAR[:3], 3 << 3), st.place(dent, (103, 135, 139))] + outside
        assert st.placed_extent((10, 3, 3), 3 << 3) == er.PILLAR[3:]
        for k, op in enumerate(ops):
            if op[0] == "edit":
                _walk_stamps(ctx, walk, s, outside)                                 # nothing is touched: nothing waits
                assert ctx.edit_boxes_pending() == (0, False)
                _walk_stamps(ctx, walk, s, batch)
                assert ctx.edit_boxes_pending() == (2, False)
                lo, hi = walk.h.boxes[1]
                assert lo.tolist() == [103, 135, 139] and hi.tolist() == [105, 137, 141]
            else:
                _history_frame(ctx, walk, op[1], "frame %d" % k)
                modes.append(walk.h.mode)
        assert modes == ["restart", "moved", "moved", "moved", "moved_boxes", "moved", "moved", "still"]
        assert ctx.accumulation() == (8, 8)


def test_seventeen_placements_overflow_and_the_frame_restarts(procedural_region, blue_noise):
    walk = er.Walk(procedural_region, blue_noise, er.SW, er.SH, er.RADIUS)
    ops = er.frames((0, 1))
    with _history_ctx(procedural_region, blue_noise) as ctx:
        s = Stamps(ctx)
        one = s.create(_solid((1, 1, 1), er.WORD))
        singles = [st.place(one, (90 + 4 * (i % 4), 124 + 4 * (i // 4), 143)) for i in range(17)]
        outside = [st.place(one, (256, 0, 0)), st.place(one, (0, -1, 0))]
        for k, op in enumerate(ops):
            _history_frame(ctx, walk, op[1], "frame %d" % k)
        _walk_stamps(ctx, walk, s, singles[:10])
        _walk_stamps(ctx, walk, s, singles[10:16] + outside)
        assert ctx.edit_boxes_pending() == (16, False)
        _history_frame(ctx, walk, er.pose(2, step=2), "sixteen boxes")
        assert walk.h.mode == "moved_boxes"
        _walk_stamps(ctx, walk, s, singles)
        assert ctx.edit_boxes_pending() == (0, True)
        _walk_stamps(ctx, walk, s, singles[:2])                                      # (an overflowed set takes no more)
        assert ctx.edit_boxes_pending() == (0, True)
        _history_frame(ctx, walk, er.pose(3, step=3), "after the overflow")
        assert walk.h.mode == "restart" and ctx.accumulation() == (1, 1)


def test_rt_bench_pastes_stamps_before_every_frame(native_built):
    """rt_bench --edit-stamp N: the four edit timing fields of --edits, two launches per call, and the count in the JSON line."""
    import json
    import os
    import subprocess
    from tests.conftest import ROOT
    exe = os.path.join(ROOT, "raytrace_amd", "rt_bench")
    r = subprocess.run([exe, "--width", "64", "--height", "64", "--frames", "6", "--edit-stamp", "8"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["edit_stamp"] == 8 and j["edits"] == 0 and j["frames"] == 6 and j["edit_launches_per_call"] == 2.0
    assert j["edit_device_ms_per_call"] > 0 and j["edit_wall_ms_per_call"] >= j["edit_host_ms_per_call"] > 0
    bad = subprocess.run([exe, "--edit-stamp", "0"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--edit-stamp" in bad.stderr


# ---- rejections, ids, device_bytes ------------------------------------------------------------------------------------------------
def test_rejections_change_nothing_and_ids_end_with_destroy(procedural_region, blue_noise):
    mats, mine = procedural_region
    lib = render._lib.amd()
    ptr = lambda a: a.ctypes.data_as(C.POINTER(abi.RtStampPlace))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    i3 = lambda *v: (C.c_int32 * 3)(*v)
    out = C.c_uint32(0)
    pair = _random_stamp((5, 3, 7), 8)
    with render.Context(render.make_config(W, H)) as ctx:                        # no world: stamps can be made, not captured or placed
        sid = ctx.stamp_create(*pair)
        with pytest.raises(render.RtError) as e:
            ctx.edit_stamps([render.stamp_place(sid, (1, 1, 1))])
        assert e.value.code == abi.RT_ERR_NOT_READY
        with pytest.raises(render.RtError) as e:
            ctx.stamp_capture((0, 0, 0), (4, 4, 4))
        assert e.value.code == abi.RT_ERR_NOT_READY
        ctx.edit_stamps([])                                                      # count == 0 asks for nothing, not even a world
        gm, gs = ctx.stamp_read(sid)
        assert np.array_equal(gs, pair[1]) and np.array_equal(gm, np.where(pair[1] != 0, pair[0], 0))    # ABSENT words read as 0
    with _history_ctx(procedural_region, blue_noise) as ctx:
        base = ctx.info().device_bytes
        s = Stamps(ctx)
        sid = s.create(pair)
        assert ctx.info().device_bytes == base + 5 * 105
        big = s.create(_solid((256, 256, 2), 1))
        assert ctx.info().device_bytes == base + 5 * 105 + 5 * 256 * 256 * 2
        ctx.stamp_destroy(big)
        del s.model[big]
        assert ctx.info().device_bytes == base + 5 * 105
        m2, f2 = mats.copy(), mine.copy()
        good = st.batch([st.place(sid, (3, 4, 5), 7)])
        s.paste(m2, f2, good)
        assert ctx.edit_boxes_pending() == (1, False)
        base = ctx.info().device_bytes - 5 * 105                                 # (the first batch made the staging set)

        def spoil(**kw):
            p = good[0].copy()
            for k, v in kw.items():
                p[k] = v
            return p
        bads = [spoil(stamp=0), spoil(stamp=big), spoil(stamp=sid + 1), spoil(stamp=sid ^ (1 << 10)), spoil(orient=48), spoil(orient=255), spoil(where=3),
                spoil(reserved0=(1, 0)), spoil(reserved0=(0, 1)), spoil(reserved=(1, 0, 0)), spoil(reserved=(0, 0, 1 << 31)),
                spoil(at=(4 * 256 + 1, 0, 0)), spoil(at=(0, 0, -4 * 256 - 1))]
        for k, bad in enumerate(bads):
            assert not st.valid(bad, 256, set(s.model)), k
            for batch in (st.batch([bad]), st.batch([good[0], bad]), st.batch([bad, good[0]])):
                with pytest.raises(render.RtError) as e:
                    ctx.edit_stamps(batch)
                assert e.value.code == abi.RT_ERR_INVALID_ARG, k
        many = np.repeat(good, 4097)
        assert lib.rt_edit_stamps(ctx.handle, ptr(many), 4097) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_edit_stamps(ctx.handle, None, 1) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_edit_stamps(ctx.handle, None, 0) == abi.RT_OK
        # create and capture
        state3 = pair[1].copy()
        state3[3, 1, 2] = 3
        for ext, m, f in ((i3(0, 3, 7), pair[0], pair[1]), (i3(5, 257, 7), pair[0], pair[1]), (i3(5, 3, -1), pair[0], pair[1]), (i3(5, 3, 7), pair[0], state3)):
            assert lib.rt_stamp_create(ctx.handle, ext, vp(m), vp(f), C.byref(out)) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_stamp_create(ctx.handle, i3(5, 3, 7), None, vp(pair[1]), C.byref(out)) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_stamp_create(ctx.handle, i3(5, 3, 7), vp(pair[0]), None, C.byref(out)) == abi.RT_ERR_INVALID_ARG
        assert lib.rt_stamp_create(ctx.handle, i3(5, 3, 7), vp(pair[0]), vp(pair[1]), None) == abi.RT_ERR_INVALID_ARG
        for lo, ext, flags in ((i3(-1, 0, 0), i3(4, 4, 4), 0), (i3(253, 0, 0), i3(4, 4, 4), 0), (i3(0, 0, 0), i3(4, 257, 4), 0), (i3(0, 0, 0), i3(4, 0, 4), 0),
                               (i3(0, 0, 256), i3(1, 1, 1), 0), (i3(0, 0, 0), i3(4, 4, 4), 2)):
            assert lib.rt_stamp_capture(ctx.handle, lo, ext, flags, C.byref(out)) == abi.RT_ERR_INVALID_ARG
        assert out.value == 0 and ctx.info().device_bytes == base + 5 * 105
        for bad_id in (0, big, sid + 1):
            assert lib.rt_stamp_info(ctx.handle, bad_id, i3(0, 0, 0)) == abi.RT_ERR_INVALID_ARG
            assert lib.rt_stamp_read(ctx.handle, bad_id, None, None) == abi.RT_ERR_INVALID_ARG
            assert lib.rt_stamp_destroy(ctx.handle, bad_id) == abi.RT_ERR_INVALID_ARG
        assert ctx.edit_boxes_pending() == (1, False)
        _check_region(ctx, m2, f2, "after the rejections")
        # the limits themselves are accepted: 4096 placements, at = +-4R, a capture against the far corner
        edge = st.batch([st.place(sid, (-1024, 1024, 0), 47), st.place(sid, (252, 254, 250), 0, st.WHERE_AIR)])
        s.paste(m2, f2, np.concatenate([np.repeat(good, 4094), edge]))
        far = ctx.stamp_capture((0, 255, 0), (256, 1, 256))
        want = st.capture(m2, f2, (0, 255, 0), (256, 1, 256))
        gm, gs = ctx.stamp_read(far)
        assert np.array_equal(gs, want[1]) and np.array_equal(gm, want[0])
        _check_region(ctx, m2, f2, "the limits")
        # a placement enqueued before its stamp is destroyed still reads it
        s.paste(m2, f2, [st.place(sid, (100, 100, 200), 20)])
        ctx.stamp_destroy(sid)
        with pytest.raises(render.RtError) as e:
            ctx.edit_stamps(good)
        assert e.value.code == abi.RT_ERR_INVALID_ARG
        with pytest.raises(render.RtError):
            ctx.stamp_destroy(sid)
        _check_region(ctx, m2, f2, "destroyed after its placement")
        again = ctx.stamp_create(*pair)
        assert again != sid and again != big and again != 0


def test_the_1025th_live_stamp_is_rejected(native_built):
    one = np.ones((1, 1, 1), np.uint32), np.full((1, 1, 1), st.SOLID, np.uint8)
    with render.Context(render.make_config(W, H)) as ctx:
        ids = [ctx.stamp_create(*one) for _ in range(1024)]
        assert len(set(ids)) == 1024 and 0 not in ids
        with pytest.raises(render.RtError) as e:
            ctx.stamp_create(*one)
        assert e.value.code == abi.RT_ERR_INVALID_ARG
        ctx.stamp_destroy(ids[7])
        new = ctx.stamp_create(*one)
        assert new not in ids
