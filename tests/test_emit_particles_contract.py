"""The rules of rt_emit_particles without a GPU: what tests/emit_particles_ref.py computes against brute force over every voxel, the
order, the density filter and its independence of the window, the emitted boxes, the debris recipe through
tests/particle_step_ref.py, the emitter table, and what the named cases of tests/emit_particles_sets.py hold."""
import numpy as np
import pytest

from raytrace_amd import world as rw
from tests import emit_particles_ref as ref
from tests import emit_particles_sets as sets
from tests import particle_step_ref as psr
from tests import scenes
from tests import shape_edits as se
from tests import sweep_ref as sr

R = 256
f32 = np.float32


def _region(ids):
    mats, mine = rw.region_from_ids(ids)
    return mats.reshape(R, R, R), mine.reshape(R, R, R)


def _brute_count(mine, e):
    """Selected voxels of one emitter at density 256, from the membership rule over every voxel of the region."""
    z, y, x = np.meshgrid(*(np.arange(R, dtype=np.int64),) * 3, indexing="ij", sparse=True)
    a, b = e["a"].astype(np.int64), e["b"].astype(np.int64)
    if e["kind"] == se.BOX:
        m = (x >= a[0]) & (x <= b[0]) & (y >= a[1]) & (y <= b[1]) & (z >= a[2]) & (z <= b[2])
    else:
        m = (2 * x + 1 - a[0]) ** 2 + (2 * y + 1 - a[1]) ** 2 + (2 * z + 1 - a[2]) ** 2 <= b[0]
    return int((m & (mine == 0)).sum())


SHAPES = [se.box((30, 40, 100), (93, 103, 131)), se.sphere((3, 129, 253), 49), se.sphere((257, 255, 250), 400), se.box((9, 18, 101), (13, 21, 103)), se.box((-5, 250, 120), (6, 300, 130)),
          se.sphere((20, 20, 200), 0), se.box((300, 10, 10), (310, 20, 20))]


@pytest.mark.parametrize("ids", [scenes.random_blocks_ids, scenes.floor_ids], ids=["random blocks", "floor"])
def test_n_equals_a_brute_force_count_over_every_voxel(ids):
    mats, mine = _region(ids())
    total = 0
    for s in SHAPES:
        e = sets._e(s, density=256)
        N, _, cur = ref.emit(mats, mine, ref.batch([e]), (0, 0, 0), np.zeros(8192, ref.STATE_DTYPE), 8192, np.zeros((), ref.CURSOR_DTYPE))
        assert N == _brute_count(mine, e) == int(cur["emitted"]) + int(cur["dropped"]) and int(cur["emitted"]) == min(N, 8192)
        total += N
    assert total > 100


def test_order_density_window_and_boxes():
    mats, mine = sets.world()
    for s in (sets.SPHERE, sets.BIG, sets.BOX543):
        e = sets._e(s, density=256)
        xyz = ref.select(mine, e, (0, 0, 0))
        keys = ref.order_key(xyz)
        assert len(keys) > 10 and all(a < b for a, b in zip(keys, keys[1:]))          # strictly increasing
        assert len(xyz) == _brute_count(mine, e)                                    # density 256 keeps all
        few = ref.select(mine, sets._e(s, density=37), (0, 0, 0))
        all_, some = {tuple(v) for v in xyz.tolist()}, {tuple(v) for v in few.tolist()}
        assert some < all_ and (len(some) > 0 or len(all_) < 40)
    # the hash takes world coordinates: a world voxel keeps its texel, (v + R/2) mod R, wherever the window sits, so a window moved
    # by d that still holds the block selects the same voxels of it; one moved so far that the block's texels hold other world
    # voxels (v + R) selects by those
    e = sets._e(sets.BIG, density=37)
    here = ref.select(mine, e, (0, 0, 0))
    there = ref.select(mine, e, (16, -32, 48))
    assert len(here) > 50 and here.tolist() == there.tolist()
    assert ref.world_voxels(here, (0, 0, 0), R).tolist() == ref.world_voxels(there, (16, -32, 48), R).tolist()
    far = ref.select(mine, e, (16 + R, -32, 48))
    assert (ref.world_voxels(far, (16 + R, -32, 48), R)[:, 0] >= R - 128).all() and far.tolist() != here.tolist()
    # other texels, the same world voxels: the block in a region of edge 512 sits 128 texels further along every axis (texel =
    # v + R/2); the shape moved with it selects the same world voxels, in the same order
    big = np.full((512, 512, 512), 6, np.uint8)
    big[128:384, 128:384, 128:384] = mine
    moved = sets._e(se.box((70 + 128, 70 + 128, 110 + 128), (81 + 128, 81 + 128, 117 + 128)), density=37)
    wide = ref.select(big, moved, (0, 0, 0))
    assert (wide - 128).tolist() == here.tolist() and ref.world_voxels(wide, (0, 0, 0), 512).tolist() == ref.world_voxels(here, (0, 0, 0), R).tolist()
    # every emitted box lies inside its voxel's cell, at the largest half too and far from the origin
    for lr, half in (((0, 0, 0), 0.5), ((2 ** 22 - R, -(2 ** 22 - R), 40), 0.5), (sets.LR_SEAM, 0.125)):
        e = sets._e(sets.BIG, half=half)
        states, texels, _ = ref.particles(mats, mine, ref.batch([e]), lr)
        v = ref.world_voxels(texels, lr, R).astype(np.float64)
        assert len(states) == 1152
        assert (states["lo"] >= v).all() and (states["hi"] <= v + 1).all() and (states["lo"] <= states["hi"]).all()
        assert (np.abs(states["lo"]) <= 2.0 ** 22).all() and (np.abs(states["hi"]) <= 2.0 ** 22).all()
        assert np.isfinite(states["velocity"]).all() and (states["life"] >= 0.5).all() and (states["life"] <= 2.5).all()


def test_the_debris_recipe_keeps_the_steps_closing_property():
    mats, mine = (a.copy() for a in sets.world())
    blast = se.sphere((121, 121, 245), 81, material=0, solid=0)
    e = ref.batch([sets._e(blast, density=96, speed=9.0, spread=2.0, life_min=1.0)])
    states, _, _ = ref.particles(mats, mine, e, (0, 0, 0))
    assert 40 <= len(states) <= 200
    kw = dict(dt=1.0 / 60.0, accel=(0.0, 0.0, -32.0), restitution=0.5, friction=0.75, rest_speed=0.25, sweeps=3)
    # without the carve every particle sits in an occupied voxel: the first tick kills them all
    out, _, _ = psr.step(sr.Occupancy(mats, mine, (0, 0, 0), R), psr.Params(**kw), states)
    assert ((out["flags"] & psr.DEAD) != 0).all()
    se.apply_shapes(mats, mine, se.batch([blast]))
    occ = sr.Occupancy(mats, mine, (0, 0, 0), R)
    history = psr.run(occ, psr.Params(**kw), states, 20)                           # raises LiveParticleEmbedded otherwise
    first = history[0]
    assert all(len(h) > 0 and h[0]["kind"] != sr.EMBEDDED for h in first[2])       # from the first tick
    assert not (history[-1][0]["flags"] & (psr.DEAD | psr.INVALID)).any()


def test_the_emitter_table_and_the_windows():
    table, expected, names = sets.emitter_table()
    got = [ref.valid(e, R) for e in table]
    assert got == expected.tolist(), [n for n, g, w in zip(names, got, expected) if g != w]
    assert expected.sum() >= 15 and (~expected).sum() >= 20
    assert [ref.window_valid(lr, R) for lr, _ in sets.WINDOWS] == [ok for _, ok in sets.WINDOWS]


def test_the_named_cases_hold_what_their_names_say():
    mats, mine = sets.world()
    cases = sets.cases()
    N = {}
    for name, c in cases.items():
        cur = np.zeros((), ref.CURSOR_DTYPE)
        cur["next"] = c["next"]
        ring = np.zeros(c["capacity"], ref.STATE_DTYPE)
        N[name], ring, cur = ref.emit(mats, mine, c["emitters"], c["lr"], ring, c["max_emit"], cur)
        assert (N[name] == 0) == c["empty"], name
        assert all(ref.valid(e, R) for e in c["emitters"]) and ref.window_valid(c["lr"], R), name
        if not c["empty"]:
            assert N[name] >= 1, name
    assert not ref.brick_boxes(cases["empty sphere"]["emitters"], R)[0] and not ref.brick_boxes(cases["outside"]["emitters"], R)[0]
    assert ref.brick_boxes(cases["air"]["emitters"], R)[1] > 0                      # a bounding box, and nothing solid in it
    # the sphere is clipped by the face x = 0, crosses a brick and a chunk edge and has lost voxels to the shaft and gained the block
    xyz = ref.select(mine, cases["sphere"]["emitters"][0], (0, 0, 0))
    assert xyz[:, 0].min() == 0 and {63, 64} <= set(xyz[:, 1].tolist()) and {127, 128} <= set(xyz[:, 2].tolist())
    assert N["one voxel"] == 1 and 1 <= N["box 5x4x3"] < 60
    # the seam: both halves emit, and the world coordinates on the two sides of y's seam lie R apart
    _, texels, who = ref.particles(mats, mine, cases["seam"]["emitters"], sets.LR_SEAM)
    assert set(who.tolist()) == {0, 1}
    v = ref.world_voxels(texels, sets.LR_SEAM, R)
    assert v[:, 1].max() - v[:, 1].min() > R - 16 and set(texels[who == 1][:, 0].tolist()) <= {0, 1}
    # the overlap: some voxel twice, the first emitter's before the second's
    _, texels, who = ref.particles(mats, mine, cases["overlap"]["emitters"], (0, 0, 0))
    both = {tuple(t) for t in texels[who == 0].tolist()} & {tuple(t) for t in texels[who == 1].tolist()}
    assert len(both) >= 4 and (np.diff(who) >= 0).all()
    assert N["density 37"] < N["density 256"] == 1152 and N["256 tiny"] >= 200
    assert N["wrap"] == 60 and 60 + N["wrap"] > 64                                 # wraps
    assert N["cut"] > cases["cut"]["max_emit"]
    assert cases["next beyond"]["next"] >= cases["next beyond"]["capacity"]
