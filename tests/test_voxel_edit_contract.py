"""rt_edit_voxels / rt_read_box on the CPU: the ABI (record layout, exports, the header's contract) and the numpy restatement of the
edit rule in tests/voxel_edits.py, held against pack_into (the procedural region) and against the oracle's pack_chunk."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytrace_amd import _lib, abi
from oracle import pyoracle as po
from tests import voxel_edits as ve
from tests.conftest import ROOT

pytestmark = pytest.mark.usefixtures("native_built")


def _header():
    return open(os.path.join(ROOT, "include", "rt_abi.h")).read()


def test_voxel_edit_record_layout():
    assert C.sizeof(abi.RtVoxelEdit) == 16
    offsets = {name: getattr(abi.RtVoxelEdit, name).offset for name, _ in abi.RtVoxelEdit._fields_}
    assert offsets == {"x": 0, "y": 2, "z": 4, "solid": 6, "material": 8, "reserved": 12}
    assert ve.edit_records(np.zeros((1, 3)), [0], [0]).dtype.itemsize == 16
    body = _header().split("typedef struct RtVoxelEdit {")[1].split("} RtVoxelEdit;")[0]
    fields = re.findall(r"\b(uint16_t|uint32_t)\s+([a-z_, ]+);", body)
    assert fields == [("uint16_t", "x, y, z"), ("uint16_t", "solid"), ("uint32_t", "material"), ("uint32_t", "reserved")]


def test_edit_functions_are_exported_and_declared():
    lib = _lib.amd()
    text = _header()
    for name in ("rt_edit_voxels", "rt_read_box"):
        assert hasattr(lib, name), name
        assert name in _lib.ABI_SYMBOLS
        assert re.search(r"\bint %s\(RtContext\* ctx," % name, text), name
    assert abi.RT_SELFTEST_SCENE_MAPS == int(re.search(r"#define RT_SELFTEST_SCENE_MAPS (\d+)", text).group(1)) == 2


def test_abi_history_names_the_edit_functions():
    """The edit functions are additive within ABI 1.3 (tests/test_abi.py pins the minor version); the history says so."""
    text = _header()
    assert int(re.search(r"#define RT_ABI_VERSION_MINOR (\d+)", text).group(1)) == 3
    assert _lib.amd().rt_abi_version() == (1 << 16) | 3
    assert "Additive, same minor version: RtVoxelEdit, rt_edit_voxels, rt_read_box, RT_SELFTEST_SCENE_MAPS" in text
    # the accumulation flag lists the edits among what restarts it
    acc = text.split("#define RT_FLAG_ACCUMULATE")[1].split("*/")[0]
    assert "rt_edit_voxels" in acc


def test_header_states_the_edit_semantics():
    doc = _header().split("int rt_edit_voxels(")[0].split("typedef struct RtVoxelEdit")[1]
    for needle in ("last edit of a voxel wins", "No other material word changes", "whole minefield rebuilt with pack_into's",
                   "current minefield value == 0", "raytrace.comp:146", "6 everywhere", "Chunks without an edit are",
                   "not touched", "pack_into-consistent", "nibble-map words that cover the touched chunks",
                   "count > 2^24", "RT_ERR_INVALID_ARG", "RT_ERR_NOT_READY", "count == 0 is a no-op", "Edits and slabs apply in call order",
                   "resets RT_FLAG_ACCUMULATE", "pinned"):
        assert needle in " ".join(doc.replace("*", " ").split()), needle


def test_chunk_minefield_on_random_chunks_equals_pack_chunk():
    rng = np.random.default_rng(5)
    cases = [np.zeros((64, 64, 64), bool), np.ones((64, 64, 64), bool)]
    one = np.zeros((64, 64, 64), bool)
    one[63, 0, 37] = True
    cases.append(one)
    for p in (0.0005, 0.01, 0.2, 0.7):
        cases.append(rng.random((64, 64, 64)) < p)
    blobs = np.zeros((64, 64, 64), bool)
    blobs[10:20, 40:44, 3:9] = True
    blobs[50:, :, 60:] = True
    cases.append(blobs)
    packed = rng.integers(0, 2 ** 32, size=64 ** 3, dtype=np.uint64).astype(np.uint32)
    for occ in cases:
        _, want = po.pack_chunk(occ.astype(np.uint8), packed)
        assert np.array_equal(ve.chunk_minefield(occ).reshape(-1), want)


def test_edits_that_change_nothing_are_the_identity_on_a_pack_into_region(procedural_region):
    """Re-stating every chunk's own occupancy (an edit of every chunk that writes a voxel's word and solidity back) rebuilds the
    procedural region's minefield exactly: the per-chunk rule IS pack_into's."""
    mats, mine = procedural_region
    m2, f2 = mats.copy(), mine.copy()
    rng = np.random.default_rng(1)
    pts = rng.integers(0, 256, size=(3000, 3))
    pts = np.concatenate([pts, [(64 * cx, 64 * cy, 64 * cz) for cz in range(4) for cy in range(4) for cx in range(4)]])
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    touched = ve.apply_edits(m2, f2, pts, mats[z, y, x], mine[z, y, x] == 0)
    assert len(touched) == 64
    assert np.array_equal(f2, mine) and np.array_equal(m2, mats)
    assert ve.apply_edits(m2, f2, np.zeros((0, 3), int), [], []) == []
    assert np.array_equal(f2, mine)


def test_edited_chunks_equal_pack_chunk_of_the_edited_occupancy():
    """A region of arbitrary minefield values: edited chunks become pack_chunk's minefield of (value == 0, overridden by the edits'
    solid flags), material words change only at edited voxels (the last edit of each), untouched chunks keep every byte."""
    rng = np.random.default_rng(9)
    R = 256
    mine = rng.integers(0, 31, size=(R, R, R), dtype=np.uint8)
    mine[0:64, 0:64, 64:128] = 0                  # a full chunk
    mine[64:128, 0:64, 0:64] = 6                  # an empty one
    mats = rng.integers(0, 2 ** 32, size=(R, R, R), dtype=np.uint64).astype(np.uint32)
    pts = np.concatenate([rng.integers(0, R, size=(4000, 3)),
                          rng.integers(0, 64, size=(500, 3)) + (64, 0, 0),      # into the full chunk
                          rng.integers(0, 64, size=(500, 3)) + (0, 0, 64),      # into the empty chunk
                          [(5, 5, 5)] * 3])                                     # duplicates: the last wins
    words = rng.integers(0, 2 ** 32, size=len(pts), dtype=np.uint64).astype(np.uint32)
    solid = rng.random(len(pts)) < 0.5
    solid[-3:] = (True, True, False)
    m2, f2 = mats.copy(), mine.copy()
    ve.apply_edits(m2, f2, pts, words, solid)
    assert m2[5, 5, 5] == words[-1] and f2[5, 5, 5] != 0
    for cz in range(4):
        for cy in range(4):
            for cx in range(4):
                box = (slice(64 * cz, 64 * cz + 64), slice(64 * cy, 64 * cy + 64), slice(64 * cx, 64 * cx + 64))
                sel = np.all((pts >> 6) == (cx, cy, cz), axis=1)
                if not sel.any():
                    assert np.array_equal(f2[box], mine[box]) and np.array_equal(m2[box], mats[box])
                    continue
                occ = mine[box] == 0
                words_c = mats[box].copy()
                for (x, y, z), w, s in zip(pts[sel] - (64 * cx, 64 * cy, 64 * cz), words[sel], solid[sel]):   # batch order
                    occ[z, y, x] = s
                    words_c[z, y, x] = w
                _, want = po.pack_chunk(occ.astype(np.uint8), words_c)
                assert np.array_equal(f2[box].reshape(-1), want), (cx, cy, cz)
                assert np.array_equal(m2[box], words_c), (cx, cy, cz)
