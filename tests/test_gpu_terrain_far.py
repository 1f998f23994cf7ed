"""rt_generate_world / rt_generate_slice far from the origin: whole regions at the edges of int32 and at unaligned windows a billion
voxels out, for seeds at the ends of uint64; the one known window whose terrain reaches chunk layer cz = 2; z at both ends of int32
and around the deep rule; slabs streamed up to 2^31 and down to -2^31; and boxes of 512^3 and 1024^3 regions there.  Every region
equals the host generator's byte for byte.  The host generator itself is held against the numpy restatement on the same inputs, and
those inputs keep the height before truncation 2^20 ULPs from an integer (tests/test_terrain_ref.py), so a differing byte is a bug
of the kernels and not rounding."""
import numpy as np
import pytest

from raytrace_amd import abi, render, world
from tests import terrain_ref as tr
from tests.test_gpu_terrain_gen import _same, _whole

pytestmark = pytest.mark.gpu

MAPS = abi.RT_SELFTEST_SCENE_MAPS
GRASS, DIRT, ROCK = (tr.material_word(i) for i in (tr.GRASS_ID, tr.DIRT_ID, tr.ROCK_ID))


def _same_far(got, want, lo, R, seed, t0=(0, 0, 0)):
    """_same, and where the box (at texel t0 of the window at lo) differs: the first differing voxel in world coordinates with its
    column's height and value before truncation."""
    what = ""
    bad = (got[1] != want[1]) | (got[0] != want[0])
    if bad.any():
        k = np.unravel_index(np.argmax(bad), bad.shape)       # [z, y, x]
        v = [int(lo[a] + ((t0[a] + int(k[2 - a]) - lo[a] - R // 2) % R)) for a in range(3)]
        h, before = tr.terrain_height(v[0], v[1], seed)
        what = ("(window %s seed %#x: %d voxels differ, the first at world (%d, %d, %d): minefield %d for %d, material %#x for %#x; "
                "column height %d, value before truncation %r)"
                % (tuple(lo), seed, int(np.count_nonzero(bad)), v[0], v[1], v[2], got[1][k], want[1][k], got[0][k], want[0][k],
                   int(h), float(before)))
    _same(got, want, what)


def _region(lo, seed, R=256):
    return world.toroidal_region(tuple(v + R // 2 for v in lo), seed, region=R)


@pytest.fixture(scope="module")
def ctx256(native_built):
    with render.Context(render.make_config(64, 64)) as ctx:
        yield ctx


def _generate(ctx, seed, lo):
    ctx.generate_world(seed, lo)
    assert ctx.selftest(MAPS) == 0


@pytest.mark.parametrize("xy,seed", tr.REGION_CASES, ids=["%d,%d-%#x" % (x, y, s) for (x, y), s in tr.REGION_CASES])
def test_whole_regions_far_out(ctx256, xy, seed):
    lo = (xy[0], xy[1], -128)
    _generate(ctx256, seed, lo)
    _same_far(_whole(ctx256, 256), _region(lo, seed), lo, 256, seed)


def test_the_tall_window_rolls_materials_in_chunk_layer_2(ctx256):
    (x, y), seed = tr.TALL
    lo = (x, y, 0)
    _generate(ctx256, seed, lo)
    got = _whole(ctx256, 256)
    _same_far(got, _region(lo, seed), lo, 256, seed)
    # window z 0..256 sits at texels 128..255, 0..127: world z >= 128 is texel z < 128
    top_mats, top_mine = got[0][:128], got[1][:128]
    solid = top_mine == 0
    assert solid.any()
    assert np.all(np.isin(top_mats[solid], [DIRT, ROCK])) and np.all(top_mats[~solid] == 0)
    assert (top_mats == DIRT).any() and (top_mats == ROCK).any()


@pytest.mark.parametrize("case,lo_z", tr.Z_CASES, ids=[str(z) for _, z in tr.Z_CASES])
def test_z_at_the_ends_and_around_the_deep_rule(ctx256, case, lo_z):
    (x, y), seed = case
    lo = (x, y, lo_z)
    _generate(ctx256, seed, lo)
    got = _whole(ctx256, 256)
    if lo_z == 2 ** 31 - 256:
        assert np.all(got[1] == 6) and np.all(got[0] == 0)
    elif lo_z == -2 ** 31:
        assert np.all(got[1] == 0) and np.all(got[0] == GRASS)
    else:
        # chunk layer -1 is solid grass whatever the heights say; it ends inside a 64-texel block of this window
        deep = (lo_z + ((np.arange(256) - lo_z - 128) % 256)) < 0
        assert 0 < deep.sum() < 256 and (deep.sum() % 64) != 0
        assert np.all(got[1][deep] == 0) and np.all(got[0][deep] == GRASS)
    _same_far(got, _region(lo, seed), lo, 256, seed)


def _slabs(ctx, seed, lo, axis, step, count):
    """generate_world at lo, then `count` slabs that move the window by `step` (+16 or -16) along `axis`; after each the region is
    the host's at the moved window.  Returns the last window."""
    lo = list(lo)
    _generate(ctx, seed, lo)
    _same_far(_whole(ctx, 256), _region(lo, seed), lo, 256, seed)
    for _ in range(count):
        slab = list(lo)
        slab[axis] = lo[axis] + 256 if step > 0 else lo[axis] - 16
        ctx.generate_slice(seed, axis, slab)
        assert ctx.selftest(MAPS) == 0
        lo[axis] += step
        _same_far(_whole(ctx, 256), _region(lo, seed), lo, 256, seed)
    return lo


def test_x_slabs_up_to_the_end_of_int32(ctx256):
    """Slabs at lo_x + 256, + 272, + 288 and + 304: the last one ends exactly at 2^31."""
    lo = _slabs(ctx256, tr.SLAB_SEED, tr.SLAB_LO, 0, 16, tr.SLAB_X_STEPS)
    assert lo[0] + 256 == 2 ** 31


def test_y_slabs_down_to_the_start_of_int32(ctx256):
    lo = _slabs(ctx256, tr.SLAB_SEED, tr.SLAB_LO, 1, -16, tr.SLAB_Y_STEPS)
    assert lo[1] == -2 ** 31


@pytest.mark.parametrize("step", [16, -16])
def test_z_slabs_far_out(ctx256, step):
    _slabs(ctx256, tr.SLAB_SEED, tr.SLAB_LO, 2, step, 1)


def _expected_box(cs, lo, R, t0, size):
    """The texel box (t0, size) of the window at lo, from whole chunks of the host's ChunkStorage."""
    v = tr.box_world_coords(lo, R, t0, size)
    want = (np.zeros(size[::-1], np.uint32), np.zeros(size[::-1], np.uint8))
    for cz in np.unique(v[2] // 64):
        for cy in np.unique(v[1] // 64):
            for cx in np.unique(v[0] // 64):
                m, f = cs.borrow_packed_chunk_data(cx, cy, cz)
                sel = [np.nonzero(v[a] // 64 == c)[0] for a, c in enumerate((cx, cy, cz))]
                loc = np.ix_(*[v[a][sel[a]] % 64 for a in (2, 1, 0)])
                want[0][np.ix_(sel[2], sel[1], sel[0])] = m[loc]
                want[1][np.ix_(sel[2], sel[1], sel[0])] = f[loc]
    return want


@pytest.mark.parametrize("R", [512, 1024])
def test_large_regions_far_out_by_boxes(R, native_built):
    with render.Context(render.make_config(64, 64, region=R)) as ctx:
        for i, (lo, seed) in enumerate(tr.box_windows(R)):
            _generate(ctx, seed, lo)
            cs = world.ChunkStorage("", seed)
            try:
                kinds = set()
                for c in tr.box_chunks(lo, R):
                    assert all(lo[a] <= 64 * c[a] and 64 * c[a] + 64 <= lo[a] + R for a in range(3)), c
                    want = cs.borrow_packed_chunk_data(*c)
                    t0 = tuple((64 * c[a] + R // 2) % R for a in range(3))
                    _same_far(ctx.read_box(t0, (64, 64, 64)), want, lo, R, seed, t0)
                    kinds.add("deep" if c[2] < 0 else "air" if np.all(want[1] == 6) else "surface" if (want[1] == 0).any() else "other")
                assert kinds >= {"deep", "air", "surface"}
                if i == 1:
                    for t0, size in tr.wrap_boxes(lo, R):
                        v = tr.box_world_coords(lo, R, t0, size)
                        assert np.any(np.diff(v[0]) < 0) and np.any(np.diff(v[1]) < 0)     # across the wrap
                        _same_far(ctx.read_box(t0, size), _expected_box(cs, lo, R, t0, size), lo, R, seed, t0)
            finally:
                cs.close()
