"""The host terrain generator (raytrace_amd/host/world.cpp) against its numpy restatement (tests/terrain_ref.py) far from the origin,
at the edges of int32 and for seeds at the ends of uint64; and the margin condition that lets the GPU tests demand equal bytes: over
every column they compare, the height before truncation stays 2^20 ULPs away from an integer."""
import numpy as np
import pytest

from raytrace_amd import world
from tests import terrain_ref as tr

pytestmark = pytest.mark.usefixtures("native_built")


def _chunk_columns(lo, n=256):
    """Chunk coordinates, per axis, of the chunk columns under the window [lo, lo + n)."""
    return [range(v // 64, (v + n - 1) // 64 + 1) for v in lo]


def _assert_host_heightmaps(lo, seed):
    """world.heightmap of every chunk column under the window equals the restatement; returns the restated heights and values of
    those whole chunk columns with the world coordinates of their first column."""
    cxs, cys = _chunk_columns(lo)
    x = 64 * cxs[0] + np.arange(64 * len(cxs))
    y = 64 * cys[0] + np.arange(64 * len(cys))
    want, v = tr.terrain_height(x[None, :], y[:, None], seed)
    for j, cy in enumerate(cys):
        for i, cx in enumerate(cxs):
            got = world.heightmap(cx, cy, seed)
            ref = want[64 * j:64 * j + 64, 64 * i:64 * i + 64]
            assert np.array_equal(got, ref), "chunk column (%d, %d): %d heights differ" % (cx, cy, np.count_nonzero(got != ref))
    return want, v, x[0], y[0]


def test_hashes_against_worked_values():
    """splitmix64's published first outputs for state 0 (mix64(k * golden) is output k + 1), and wrap-around on negative input."""
    assert int(tr.mix64(np.uint64(0))) == 0xE220A8397B1DCDAF
    assert int(tr.mix64(np.uint64(0x9E3779B97F4A7C15))) == 0x6E789E6AA1B965F4
    a = tr.hash3(2 ** 64 - 1, np.array([-1, -2 ** 31]), np.array([2 ** 31 - 1, -1]), np.array([0, -7]))
    b = tr.hash3(2 ** 64 - 1, np.array([2 ** 64 - 1, 2 ** 64 - 2 ** 31], dtype=np.uint64), np.array([2 ** 31 - 1, 2 ** 64 - 1], dtype=np.uint64),
                 np.array([0, 2 ** 64 - 7], dtype=np.uint64))
    assert a.dtype == np.uint64 and np.array_equal(a, b) and a[0] != a[1]


def test_ulps_to_integer():
    v = np.array([10.0, 10.5, np.nextafter(64.0, 0.0), np.nextafter(64.0, 100.0), 127.75])
    assert np.array_equal(tr.ulps_to_integer(v), [0.0, 2.0 ** 48, 1.0, 1.0, 2.0 ** 44])


@pytest.mark.parametrize("seed", tr.SEEDS, ids=lambda s: "%#x" % s)
def test_host_heightmaps_equal_the_restatement(seed):
    for lo in tr.WINDOWS:
        _assert_host_heightmaps(lo, seed)


@pytest.mark.parametrize("seed", [tr.SEEDS[2], tr.SEEDS[4]], ids=lambda s: "%#x" % s)
def test_host_chunks_equal_the_restatement(seed):
    cs = world.ChunkStorage("", seed)
    try:
        for k, lo in enumerate(tr.WINDOWS):
            cxs, cys = _chunk_columns(lo)
            # the far corner of the window, and one more column that moves with the window
            for cx, cy in {(cxs[-1], cys[0]), (cxs[k % len(cxs)], cys[-1 - k % 2])}:
                h = tr.heightmap(cx, cy, seed)[0]
                for cz in (-1, 0, 1, 2):
                    mats, mine = cs.borrow_packed_chunk_data(cx, cy, cz)
                    want = tr.chunk(cx, cy, cz, seed, heights=h)
                    assert np.array_equal(mine, want[1]), (cx, cy, cz)
                    assert np.array_equal(mats, want[0]), (cx, cy, cz, int(np.count_nonzero(mats != want[0])))
    finally:
        cs.close()


def test_material_words_equal_the_host_table():
    for i in (tr.GRASS_ID, tr.DIRT_ID, tr.ROCK_ID):
        assert tr.material_word(i) == world.material_pack(i)


def test_margin_condition_over_the_columns_the_gpu_tests_compare():
    """No compared column's value before truncation comes within 2^20 ULPs of an integer, so a pow a few ULPs off cannot change a
    height: a byte that differs between device and host on these inputs is a bug."""
    worst = (np.inf, None)
    lowest, highest, columns = 10 ** 9, -10 ** 9, 0
    for what, seed, xs, ys in tr.gpu_columns():
        h, v = tr.terrain_height(xs[None, :], ys[:, None], seed)
        u = tr.ulps_to_integer(v)
        assert np.all(np.isfinite(v))
        k = np.unravel_index(np.argmin(u), u.shape)
        if u[k] < worst[0]:
            worst = (float(u[k]), "%s seed %#x column (%d, %d) value %r" % (what, seed, xs[k[1]], ys[k[0]], float(v[k])))
        lowest, highest, columns = min(lowest, int(h.min())), max(highest, int(h.max())), columns + h.size
    print("minimum margin %.3g ULPs at %s; heights %d..%d over %d columns" % (worst[0], worst[1], lowest, highest, columns))
    assert worst[0] >= tr.MARGIN_ULPS, worst
    assert highest < 160


def test_the_tall_window():
    """Seed 7 at (75355856, -1484678736): the one known window whose columns reach chunk layer cz = 2 (z >= 128), where the material
    roll runs in a third chunk layer; no column anywhere in the census reaches 160."""
    (x, y), seed = tr.TALL
    hc, vc, x0, y0 = _assert_host_heightmaps((x, y), seed)
    h, v = (a[y - y0:y - y0 + 256, x - x0:x - x0 + 256] for a in (hc, vc))
    tall = int(np.count_nonzero(h >= 128))
    print("columns with height >= 128: %d, maximum %d, margin %.3g ULPs" % (tall, h.max(), tr.ulps_to_integer(v).min()))
    assert tall >= 100 and h.max() < 160
    # a chunk of layer 2 that holds solid voxels equals the restatement, materials included
    j, i = np.unravel_index(np.argmax(h), h.shape)
    cx, cy = (x + i) // 64, (y + j) // 64
    cs = world.ChunkStorage("", seed)
    try:
        mats, mine = cs.borrow_packed_chunk_data(cx, cy, 2)
    finally:
        cs.close()
    want = tr.chunk(cx, cy, 2, seed)
    assert np.count_nonzero(mine == 0) > 0
    assert np.array_equal(mine, want[1]) and np.array_equal(mats, want[0])
    assert set(np.unique(mats[mine == 0]).tolist()) <= {tr.material_word(tr.DIRT_ID), tr.material_word(tr.ROCK_ID)}
