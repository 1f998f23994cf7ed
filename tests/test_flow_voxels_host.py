"""The host half of rt_flow_voxels that needs no context (raytrace_amd/csrc/api/flow_check.hpp), run by tests/flow_voxels_main.cpp as a
program of its own under the address and undefined-behaviour sanitizers, over the parameter table the contract test judges with the
restatement: verdicts, the clipped boxes with their chunk lists, tiles, state cells, launches and scratch words, the argument refusals,
the clipped extent's limit at regions above 256 and the largest box (256^3 cells off the chunk grid).  Nothing sanitized is loaded into
this process."""
import os
import subprocess

from tests import flow_voxels_ref as ref
from tests import flow_voxels_sets as sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "flow_voxels_main.cpp")
BASE = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build(exe):
    """With the sanitizers (their runtimes linked into the program where the compiler has the archives); without them where it has
    no runtime at all: the comparison with the restatement runs either way."""
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []):
        r = subprocess.run(BASE + extra + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            return extra, r
    raise AssertionError("flow_voxels_main.cpp does not compile:\n" + r.stderr[-4000:])


def test_the_host_checks_and_plans_match_the_restatement_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "flow_voxels_main")
    flags, _ = _build(exe)
    table, expected, names = sets.params_table()
    records = str(tmp_path / "records.bin")
    table.tofile(records)
    extents = tmp_path / "extents.txt"
    extents.write_text("".join("%d %d %d %d %d %d %d\n" % (tuple(lo) + tuple(hi) + (logr,)) for lo, hi, logr, _ in sets.extent_table()))
    r = subprocess.run([exe, records, "8", str(extents)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "flags %s\n%s\n%s" % (" ".join(flags), r.stdout[-2000:], r.stderr[-6000:])
    lines = r.stdout.splitlines()
    out = dict(line.split(" ", 1) for line in lines if line.startswith(("records ", "verdicts ")))
    want = [ref.valid(p, 256) for p in table]
    assert int(out["records"]) == table.size
    got = [c == "1" for c in out["verdicts"]]
    assert got == want, [n for n, g, w in zip(names, got, want) if g != w]
    assert got == expected.tolist() and True in got and False in got            # both verdicts occur
    # the plans: the clipped box, its chunks, the staging bytes, the tiles, the state cells, the launches per G and the scratch words
    plans = dict(line[5:].split(": ", 1) for line in lines if line.startswith("plan "))
    assert sorted(int(k) for k in plans) == [i for i, ok in enumerate(want) if ok]
    seen_empty = seen_many = 0
    for i, line in plans.items():
        p = table[int(i)]
        pl = [ref.plan(p, 256, g) for g in sets.GROUPS]
        if pl[0] is None:
            assert line == "empty"
            seen_empty += 1
            continue
        ids = [(cz * 4 + cy) * 4 + cx for cx, cy, cz in ref.box_chunks(pl[0]["box"])]
        assert ids == sorted(ids) and len(ids) == pl[0]["nchunks"]
        q = pl[0]
        assert line == "box %s ext %d %d %d chunks %d %d %d need %d tiles %d %d %d = %d cells %d launches %d %d %d %d scratch %d ids%s (%d)" % (
            " ".join(str(int(v)) for v in list(q["box"][0]) + list(q["box"][1])), *q["ext"], *q["nc"], q["need"], *q["tiles"], q["ntiles"], q["cells"],
            *[x["launches"] for x in pl], q["scratch"], "".join(" %d" % c for c in ids[:64]), len(ids)), names[int(i)]
        seen_many += len(ids) == 8
    assert seen_empty == 2 and seen_many >= 1
    args = dict(line[5:].split(": ", 1) for line in lines if line.startswith("args "))
    assert args == {"params": "ok", "null params": "null params"}
    verdicts = [line for line in lines if line.startswith("extent ")]
    assert verdicts == ["extent %d" % ok for _, _, _, ok in sets.extent_table()] and {"extent 0", "extent 1"} == set(verdicts)
    big = ref.plan(ref.params((10, 10, 10), (265, 265, 265), ticks=256, **sets.MASK), 512, 4)
    assert [line for line in lines if line.startswith("largest")] == ["largest: valid 1 chunks 125 tiles 2048 cells %d launches 256 64 scratch %d" % (1 << 24, big["scratch"])]
    assert big["scratch"] == 512 + (1 << 23) and big["ntiles"] == 2048
