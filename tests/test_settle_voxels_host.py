"""The host half of rt_settle_voxels that needs no context (raytrace_amd/csrc/api/settle_check.hpp), run by
tests/settle_voxels_main.cpp as a program of its own under the address and undefined-behaviour sanitizers, over the parameter table
the contract test judges with the restatement: verdicts, the clipped boxes with their columns, heights and chunk lists, the argument
refusals, and the whole region at R = 1024 (no texel limit).  Nothing sanitized is loaded into this process."""
import os
import subprocess

from tests import settle_voxels_ref as ref
from tests import settle_voxels_sets as sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "settle_voxels_main.cpp")
BASE = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build(exe):
    """With the sanitizers (their runtimes linked into the program where the compiler has the archives); without them where it has
    no runtime at all: the comparison with the restatement runs either way."""
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []):
        r = subprocess.run(BASE + extra + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            return extra, r
    raise AssertionError("settle_voxels_main.cpp does not compile:\n" + r.stderr[-4000:])


def test_the_host_checks_and_plans_match_the_restatement_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "settle_voxels_main")
    flags, _ = _build(exe)
    table, expected, names = sets.params_table()
    records = str(tmp_path / "records.bin")
    table.tofile(records)
    r = subprocess.run([exe, records, "8"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "flags %s\n%s\n%s" % (" ".join(flags), r.stdout[-2000:], r.stderr[-6000:])
    lines = r.stdout.splitlines()
    out = dict(line.split(" ", 1) for line in lines if not line.startswith(("args ", "plan ", "whole ")))
    want = [ref.valid(p, 256) for p in table]
    assert int(out["records"]) == table.size
    got = [c == "1" for c in out["verdicts"]]
    assert got == want, [n for n, g, w in zip(names, got, want) if g != w]
    assert got == expected.tolist()
    # the plans: the clipped box, its columns and height, its chunks, the staging bytes and the scratch words
    plans = dict(line[5:].split(": ", 1) for line in lines if line.startswith("plan "))
    assert sorted(int(k) for k in plans) == [i for i, ok in enumerate(want) if ok]
    seen_empty = seen_many = 0
    heights = set()
    for i, line in plans.items():
        p = table[int(i)]
        bb = ref.clipped_box(p, 256)
        if bb is None:
            assert line == "empty"
            seen_empty += 1
            continue
        chunks = ref.box_chunks(bb)
        ids = [(cz * 4 + cy) * 4 + cx for cx, cy, cz in chunks]
        assert ids == sorted(ids)
        nc = [(int(bb[1][k]) >> 6) - (int(bb[0][k]) >> 6) + 1 for k in range(3)]
        ext = [int(bb[1][k]) - int(bb[0][k]) + 1 for k in range(3)]
        height = ext[int(p["axis"])]
        assert line == "box %s columns %d height %d chunks %d %d %d need %d scratch %d ids%s (%d)" % (
            " ".join(str(int(v)) for v in list(bb[0]) + list(bb[1])), ext[0] * ext[1] * ext[2] // height, height, nc[0], nc[1], nc[2],
            (4 * len(ids) + 15) // 16 * 16, len(ids) + 4, "".join(" %d" % c for c in ids[:64]), len(ids)), names[int(i)]
        seen_many += len(ids) == 8
        if names[int(i)].startswith("axis "):
            heights.add(height)
    assert seen_empty == 2 and seen_many >= 1 and heights == {31, 36, 41}
    args = dict(line[5:].split(": ", 1) for line in lines if line.startswith("args "))
    assert args == {"params": "ok", "null params": "null params"}
    assert [line for line in lines if line.startswith("whole ")] == ["whole 1024: valid 1 columns %d height 1024 chunks 4096 scratch 4100" % (1 << 20)]
