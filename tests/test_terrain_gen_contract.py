"""The contract behind rt_generate_world / rt_generate_slice, checked on the CPU: both functions are declared and exported; the
minefield of a generated chunk is a function of its heights alone (the rule k_terrain_fill uses, restated in numpy against
pack_into); and the window -> texel mapping restated against world.toroidal_region and the host TerrainUploadManager."""
import os
import re

import numpy as np
import pytest

from raytrace_amd import _lib, world
from tests import terrain_ref
from tests.conftest import ROOT

pytestmark = pytest.mark.usefixtures("native_built")

GRASS, DIRT, ROCK = (world.material_pack(i) for i in (2, 5, 6))


def test_both_functions_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)
    lib = _lib.amd()
    for name in ("rt_generate_world", "rt_generate_slice"):
        assert re.search(r"\bint %s\s*\(RtContext\* ctx, uint64_t seed," % name, text), name
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name)


def minefield_from_heights(h, cz):
    """Rule (b): solid = deep || z < h; an empty voxel takes the first L in 1..6 whose aligned 2^L cube is occupied, i.e. whose
    footprint's max height exceeds the cube's lowest z (6 when none is).  h: int[64 y, 64 x] heights of the chunk column."""
    oz = 64 * cz
    if oz + 64 < 12:
        return np.zeros((64, 64, 64), np.uint8)
    z = oz + np.arange(64)[:, None, None]
    out = np.where(z < h[None], 0, 6).astype(np.uint8)
    for L in range(5, 0, -1):   # lowest level last: it wins
        s = 1 << L
        m = h.reshape(64 // s, s, 64 // s, s).max(axis=(1, 3)).repeat(s, 0).repeat(s, 1)
        occupied = m[None] > (z & ~(s - 1))
        out = np.where((out != 0) & occupied, L, out).astype(np.uint8)
    return out


CHUNKS = [(-2, -2, -1), (0, 0, -1),            # deep
          (1, -1, 4), (-2, 1, 3),             # all air
          (-1, -2, 0), (0, 1, 0), (1, 0, 1), (-2, 0, 1), (3, 2, 2), (0, -1, 2)]   # cut by the surface


@pytest.mark.parametrize("seed", [world.DEFAULT_SEED, 0xFEEDFACE12345678])
def test_minefield_is_a_function_of_the_heights(seed):
    cs = world.ChunkStorage("", seed)
    try:
        for cx, cy, cz in CHUNKS:
            h = world.heightmap(cx, cy, seed)
            mats, mine = cs.borrow_packed_chunk_data(cx, cy, cz)
            want = minefield_from_heights(h, cz)
            assert np.array_equal(mine, want), (cx, cy, cz)
            ids = np.where(mine == 0, 2, 0).astype(np.uint8)          # any solid id: pack_into only sees solidity
            assert np.array_equal(world.pack_chunk(ids)[1], want), (cx, cy, cz)
            # materials: grass in a deep chunk, air 0, material_for_height (restated in tests/terrain_ref.py) elsewhere
            z = 64 * cz + np.arange(64)[:, None, None] + np.zeros((64, 64, 64), int)
            solid = mine == 0
            assert np.all(mats[~solid] == 0)
            if 64 * cz + 64 < 12:
                assert np.all(mats == GRASS)
            else:
                assert np.all(mats[solid & (z < 20)] == GRASS) and np.all(mats[solid & (z >= 160)] == ROCK)
                ids = terrain_ref.material_for_height(seed, 64 * cx + np.arange(64)[None, None, :], 64 * cy + np.arange(64)[None, :, None], z)
                words = np.zeros(7, np.uint32)
                words[[2, 5, 6]] = GRASS, DIRT, ROCK
                assert np.array_equal(mats[solid], words[ids][solid])
    finally:
        cs.close()


@pytest.mark.parametrize("cz", [-1, 0, 1])
def test_chunks_around_z_12(cz):
    """The deep-chunk rule (oz + 64 < 12) around the lowest surface height (heights are >= 10)."""
    cs = world.ChunkStorage("", world.DEFAULT_SEED)
    try:
        for cx, cy in ((0, 0), (-1, 2), (5, -3)):
            h = world.heightmap(cx, cy)
            assert h.min() >= 10
            assert np.array_equal(cs.borrow_packed_chunk_data(cx, cy, cz)[1], minefield_from_heights(h, cz))
    finally:
        cs.close()


def region_of_window(lo, seed, R, cs):
    """The texel mapping restated: texel t on axis a holds world voxel v = lo[a] + ((t - lo[a] - R/2) mod R)."""
    mats = np.zeros((R, R, R), np.uint32)
    mine = np.zeros((R, R, R), np.uint8)
    t = np.arange(R)
    v = [lo[a] + ((t - lo[a] - R // 2) % R) for a in range(3)]
    chunks = [np.unique(va // 64) for va in v]
    for cz in chunks[2]:
        for cy in chunks[1]:
            for cx in chunks[0]:
                m, f = cs.borrow_packed_chunk_data(cx, cy, cz)
                sel = [np.nonzero(v[a] // 64 == c)[0] for a, c in enumerate((cx, cy, cz))]
                loc = [v[a][sel[a]] - 64 * c for a, c in enumerate((cx, cy, cz))]
                ix = np.ix_(sel[2], sel[1], sel[0])
                mats[ix] = m[np.ix_(loc[2], loc[1], loc[0])]
                mine[ix] = f[np.ix_(loc[2], loc[1], loc[0])]
    return mats, mine


@pytest.mark.parametrize("lo", [(-128, -128, -128), (-112, 48, -144), (16, -80, 32)])
def test_window_to_texel_mapping_matches_toroidal_region(lo):
    cs = world.ChunkStorage("", world.DEFAULT_SEED)
    try:
        got = region_of_window(lo, world.DEFAULT_SEED, 256, cs)
    finally:
        cs.close()
    want = world.toroidal_region(tuple(l + 128 for l in lo))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if lo == (-128, -128, -128):
        reg = world.generate_region(world.DEFAULT_SEED)
        assert np.array_equal(got[0], reg[0]) and np.array_equal(got[1], reg[1])


def test_a_streamer_request_is_the_window_of_its_slab():
    """next_window of a HostTerrainUploadManager request: applying the restated window of every request reproduces the manager's
    own region, so rt_generate_slice on these windows can replay a move list."""
    R = 256
    t = world.HostTerrainUploadManager()
    cs = world.ChunkStorage("", world.DEFAULT_SEED)
    try:
        assert t.next_window() is None
        mats, mine = world.generate_region(world.DEFAULT_SEED)
        for axis, inc in [(0, 1), (2, 0), (0, 1), (1, 0), (1, 0), (2, 1), (0, 0)]:
            (t.request_increase if inc else t.request_decrease)(axis)
        while t.pending():
            axis, lo = t.next_window()
            assert all(v % 16 == 0 for v in lo)
            full = region_of_window(lo, world.DEFAULT_SEED, R, cs)
            off = (lo[axis] + R // 2) % R
            sl = [slice(None)] * 3
            sl[2 - axis] = slice(off, off + 16)
            mats[tuple(sl)], mine[tuple(sl)] = full[0][tuple(sl)], full[1][tuple(sl)]
            t.setup_next_request()
        gm, gf = t.region()
        assert np.array_equal(gm, mats) and np.array_equal(gf, mine)
    finally:
        cs.close()
        t.close()
