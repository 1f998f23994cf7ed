"""The host half of rt_detach_voxels that needs no context (raytrace_amd/csrc/api/detach_check.hpp), run by
tests/detach_voxels_main.cpp as a program of its own under the address and undefined-behaviour sanitizers, over the parameter table
the contract test judges with the restatement: verdicts, the clipped boxes with the stamp's extent and the chunk lists, the scratch
size, the argument refusals, and the largest box (5 x 5 x 5 chunks).  Nothing sanitized is loaded into this process."""
import os
import subprocess

import numpy as np

from tests import detach_voxels_ref as ref
from tests import detach_voxels_sets as sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "detach_voxels_main.cpp")
BASE = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
HEAD, CHUNK = 288, 64 * 64 * 2                               # words of the scratch's head and of one bitmap of a chunk


def _build(exe):
    """With the sanitizers (their runtimes linked into the program where the compiler has the archives); without them where it has
    no runtime at all: the comparison with the restatement runs either way."""
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []):
        r = subprocess.run(BASE + extra + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            return extra, r
    raise AssertionError("detach_voxels_main.cpp does not compile:\n" + r.stderr[-4000:])


def _scratch(n):
    return HEAD + (n + 3) // 4 * 4 + 3 * CHUNK * n


def test_the_host_checks_and_plans_match_the_restatement_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "detach_voxels_main")
    flags, _ = _build(exe)
    table, expected, names = sets.params_table()
    for logr, R, rows, verdicts in ((8, 256, table, expected.tolist()),
                                    (9, 512, np.array([r for r, _ in sets.EXTENT_ROWS], dtype=ref.DETACH_DTYPE), [ok for _, ok in sets.EXTENT_ROWS])):
        records = str(tmp_path / ("records%d.bin" % logr))
        rows.tofile(records)
        r = subprocess.run([exe, records, str(logr)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, "flags %s\n%s\n%s" % (" ".join(flags), r.stdout[-2000:], r.stderr[-6000:])
        lines = r.stdout.splitlines()
        out = dict(line.split(" ", 1) for line in lines if line.startswith(("records ", "verdicts ")))
        want = [ref.valid(p, R) for p in rows]
        assert int(out["records"]) == rows.size
        got = [c == "1" for c in out["verdicts"]]
        assert got == want, [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert got == verdicts
        # the plans: the clipped box, the stamp's extent, its chunks, the staging bytes and the scratch words
        plans = dict(line[5:].split(": ", 1) for line in lines if line.startswith("plan "))
        assert sorted(int(k) for k in plans) == [i for i, ok in enumerate(want) if ok]
        seen_empty = seen_many = 0
        nl = logr - 6
        for i, line in plans.items():
            bb = ref.clipped_box(rows[int(i)], R)
            if bb is None:
                assert line == "empty"
                seen_empty += 1
                continue
            ids = [((cz << nl) + cy << nl) + cx for cx, cy, cz in ref.box_chunks(bb)]
            assert ids == sorted(ids)
            nc = [(int(bb[1][k]) >> 6) - (int(bb[0][k]) >> 6) + 1 for k in range(3)]
            ext = [int(bb[1][k]) - int(bb[0][k]) + 1 for k in range(3)]
            assert line == "box %s extent %d %d %d chunks %d %d %d need %d scratch %d ids%s (%d)" % (
                " ".join(str(int(v)) for v in list(bb[0]) + list(bb[1])), ext[0], ext[1], ext[2], nc[0], nc[1], nc[2], (4 * len(ids) + 15) // 16 * 16,
                _scratch(len(ids)), "".join(" %d" % c for c in ids[:128]), len(ids)), i
            seen_many += len(ids) == 64
        if logr == 8:
            assert seen_empty == 2 and seen_many >= 1
    args = dict(line[5:].split(": ", 1) for line in lines if line.startswith("args "))
    assert args == {"query": "ok", "null params": "null params", "capture": "ok", "capture without stamp_out": "RT_DETACH_CAPTURE needs stamp_out",
                    "unknown flag": "unknown flag bit"}
    assert [line for line in lines if line.startswith(("largest", "one more"))] == ["largest: valid 1 extent 256 chunks 125 scratch %d" % _scratch(125),
                                                                                  "one more: valid 0"]
