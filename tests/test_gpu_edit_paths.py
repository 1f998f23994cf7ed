"""What the four kinds of chunk edit share on the host — rt_edit_voxels, rt_edit_shapes, rt_edit_stamps and rt_deposit_particles —
tested across kinds: the two staging sets they use in turn (with a set that grows while the other's transfer is pending) and the one
set of pending boxes of a context that keeps its history.  The per-kind tests pin each kind alone; here every call is of another
kind than the one before.  The world is compared with the restatements (voxel_edits, shape_edits, stamp_edits,
deposit_particles_ref) applied in call order, bit for bit through rt_read_box, and the nibble maps with RT_SELFTEST_SCENE_MAPS."""
import numpy as np
import pytest

from raytrace_amd import abi, render
from tests import deposit_particles_ref as ref
from tests import deposit_particles_sets as sets
from tests import edit_history_ref as er
from tests import shape_edits as se
from tests import stamp_edits as st
from tests import voxel_edits as ve
from tests.test_gpu_deposit_particles import _dev, _host, _p, _same
from tests.test_gpu_edit_history import _ctx as _history_ctx

pytestmark = pytest.mark.gpu

MAPS = abi.RT_SELFTEST_SCENE_MAPS
W, H, R = 64, 40, 256
ROW_Y, FLOOR_Z = 40, 128                                  # the row of texels the calls fight over: on the floor of sets.world()
HOLE = (np.zeros((1, 1, 2), np.uint32), np.full((1, 1, 2), st.AIR, np.uint8))      # a stamp: two texels of air along x


def _row(x0, x1):
    """The texels (x0..x1, ROW_Y, FLOOR_Z) as xyz rows."""
    return np.array([(x, ROW_Y, FLOOR_Z) for x in range(x0, x1 + 1)], dtype=np.int64)


def _resting(x0, x1, material0):
    """One particle at rest in each texel of _row(x0, x1) (lr = 0: world voxel = texel - R / 2)."""
    return sets.resting(_row(x0, x1) - R // 2, material0=material0)


def _ops(hole):
    """Six calls on the row, every one undoing or blocking part of the one before it; the last one's 10 000 records of 8 bytes do not
    fit the 64 KiB an edit set starts with, and its block lies across the chunk boundary x = 64."""
    z, y, x = np.mgrid[FLOOR_Z:FLOOR_Z + 25, ROW_Y:ROW_Y + 10, 39:79]
    big = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    assert len(big) == 10000 and len(big) * 8 > 64 << 10 and big[:, 0].min() < 64 <= big[:, 0].max()
    return [
        ("voxels", _row(30, 33), np.zeros(4, np.uint32), np.zeros(4, bool)),                           # cleared: already air
        ("deposit", ref.params((20, 30, 120), (100, 70, 135)), _resting(30, 37, 0xA000)),            # eight chunks; fills 30..37
        ("shapes", se.batch([se.box((32, ROW_Y, FLOOR_Z), (35, ROW_Y, FLOOR_Z), 0x77, 0)])),          # carves 32..35
        ("deposit", ref.params((30, 36, 126), (45, 44, 130)), _resting(34, 39, 0xB000)),             # fills 34, 35, 38, 39; 36, 37 are taken
        ("stamps", [st.place(hole, (38, ROW_Y, FLOOR_Z))]),                                            # clears 38, 39
        ("voxels", big, 0x5000 + np.arange(len(big), dtype=np.uint32), np.ones(len(big), bool)),       # fills 39 and on
    ]


def _restate(world, ops, model):
    """The calls on a copy of the world, in order -> (mats, mine) of the chunks they can reach, and (states, counts) per deposit."""
    mats, mine = world[0].copy(), world[1].copy()
    deposits = []
    for kind, *a in ops:
        if kind == "voxels":
            ve.apply_edits(mats, mine, *a)
        elif kind == "shapes":
            se.apply_shapes(mats, mine, a[0])
        elif kind == "stamps":
            st.apply_stamps(mats, mine, model, st.batch(a[0]))
        else:
            s, _, c, _ = ref.deposit(mats, mine, a[0], a[1])
            deposits.append((s, c))
    return mats[64:192, :128, :128].copy(), mine[64:192, :128, :128].copy(), deposits


def test_four_kinds_take_turns_over_the_two_sets_and_one_grows():
    world = sets.world()
    ctx = render.Context(render.make_config(W, H, spp=1, region=R))
    try:
        ctx.upload_world(world[0].reshape(-1), world[1].reshape(-1))
        hole = ctx.stamp_create(*HOLE)
        ops, model = _ops(hole), {hole: HOLE}
        assert [op[0] for op in ops] == ["voxels", "deposit", "shapes", "deposit", "stamps", "voxels"]
        want_mats, want_mine, want_deposits = _restate(world, ops, model)
        # every two consecutive calls write the same chunk, and the other order of the two leaves another world
        for i in range(len(ops) - 1):
            swapped = ops[:i] + [ops[i + 1], ops[i]] + ops[i + 2:]
            assert not np.array_equal(_restate(world, swapped, model)[1], want_mine), "calls %d and %d commute" % (i, i + 1)
        # the deposits' device arrays first (_dev synchronises the device), so that nothing waits between the six calls
        tensors = [(_dev(op[2]), _dev(np.zeros(1, ref.COUNT_DTYPE))) for op in ops if op[0] == "deposit"]
        waiting = iter(tensors)
        for kind, *a in ops:                                           # no sync in between
            if kind == "voxels":
                ctx.edit_voxels(*a)
            elif kind == "shapes":
                ctx.edit_shapes(a[0])
            elif kind == "stamps":
                ctx.edit_stamps(st.batch(a[0]))
            else:
                t_s, t_c = next(waiting)
                ctx.deposit_particles_async(_p(a[0]), t_s, None, t_c)
        ctx.sync()
        got_mats, got_mine = ctx.read_box((0, 0, 64), (128, 128, 128))
        assert np.array_equal(got_mine, want_mine), "minefield differs at %d voxels" % int(np.count_nonzero(got_mine != want_mine))
        assert np.array_equal(got_mats, want_mats), "materials differ at %d voxels" % int(np.count_nonzero(got_mats != want_mats))
        for k, ((t_s, t_c), (want_s, want_c)) in enumerate(zip(tensors, want_deposits)):
            _same(_host(t_s, ref.STATE_DTYPE), want_s, "deposit %d: states" % k)
            _same(_host(t_c, ref.COUNT_DTYPE), want_c.reshape(1), "deposit %d: counts" % k)
        assert ctx.selftest(MAPS) == 0
    finally:
        ctx.destroy()


# ---- one set of pending boxes for the four kinds -------------------------------------------------------------------------------------
OUTSIDE = ((300, 10, 10), (310, 20, 20))                               # a box beyond the region: no bounding box
NOTHING = sets.nothing_case()                                   # candidates that deposit nothing: the box still waits


def _voxels(*xyz):
    xyz = np.array(xyz, dtype=np.int64)
    return ("voxels", xyz, np.full(len(xyz), er.WORD, np.uint32), np.ones(len(xyz), bool))


def _shapes(*corners):
    return ("shapes", se.batch([se.box(c, tuple(v + 1 for v in c), er.WORD) for c in corners] + [se.box(*OUTSIDE)]))


def _stamps(*at):
    return ("stamps", list(at) + [(256, 0, 0)])


def _deposit(lo=(60, 60, 120), hi=(75, 75, 135)):
    return ("deposit", ref.params(lo, hi))


def _call(ctx, op, one, t_states):
    """One call on the context -> the boxes it brings, by the restatements: a box per touched chunk, per shape or placement that has a
    bounding box, and one per deposit whose clipped box is not empty."""
    kind, a = op[0], op[1:]
    if kind == "voxels":
        ctx.edit_voxels(*a)
        return len(er.chunk_boxes(a[0], R))
    if kind == "shapes":
        ctx.edit_shapes(a[0])
        return len(se.pending_boxes(a[0], R))
    if kind == "stamps":
        places = st.batch([st.place(one, at) for at in a[0]])
        ctx.edit_stamps(places)
        return len(st.pending_boxes({one: (np.zeros((1, 1, 1), np.uint32), np.full((1, 1, 1), st.SOLID, np.uint8))}, places, R))
    ctx.deposit_particles_async(_p(a[0]), t_states)
    return 0 if ref.clipped_box(a[0], R) is None else 1


FILL = [_voxels((10, 10, 10), (100, 10, 10)), _shapes((5, 5, 5), (70, 5, 5)), _stamps((20, 20, 20), (30, 30, 30)), _deposit(), _deposit(*OUTSIDE),
        _voxels((10, 10, 10), (11, 10, 10), (10, 100, 10), (10, 10, 100)), _shapes((5, 5, 5), (6, 6, 6), (7, 7, 7), (200, 8, 8)), _stamps((40, 40, 40)),
        _deposit((-10, 30, 120), (20, 50, 140))]
ONE_MORE = dict(voxels=_voxels((10, 10, 10)), shapes=_shapes((5, 5, 5)), stamps=_stamps((20, 20, 20)), deposit=_deposit())


@pytest.mark.parametrize("kind", list(ONE_MORE))
def test_the_four_kinds_fill_one_pending_set_and_any_of_them_overflows_it(procedural_region, blue_noise, kind):
    with _history_ctx(procedural_region, blue_noise, W, H) as ctx:
        one = ctx.stamp_create(np.full((1, 1, 1), er.WORD, np.uint32), np.full((1, 1, 1), st.SOLID, np.uint8))
        t_states = _dev(NOTHING["states"])
        ctx.draw_frame(er.pose(0))
        ctx.draw_frame(er.pose(1))
        assert ctx.accumulation() == (2, 2) and ctx.edit_boxes_pending() == (0, False)
        total, brought = 0, []
        for op in FILL:
            brought.append(_call(ctx, op, one, t_states))
            total += brought[-1]
            assert ctx.edit_boxes_pending() == (total, False), (op[0], brought)
        assert brought == [2, 2, 2, 1, 0, 3, 4, 1, 1] and total == er.MAX_BOXES == 16
        assert _call(ctx, ONE_MORE[kind], one, t_states) == 1
        assert ctx.edit_boxes_pending() == (0, True)
        for op in ONE_MORE.values():                                   # (an overflowed set takes no more, whatever the kind)
            _call(ctx, op, one, t_states)
            assert ctx.edit_boxes_pending() == (0, True)
        ctx.draw_frame(er.pose(2))
        assert ctx.edit_boxes_pending() == (0, False)                  # the frame consumed the overflow ...
        assert ctx.accumulation() == (1, 1) and (ctx.read_history() == 1).all()      # ... and restarted
        assert ctx.selftest(MAPS) == 0
