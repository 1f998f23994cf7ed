"""The host half of rt_deposit_particles that needs no context (raytrace_amd/csrc/api/deposit_check.hpp), run by
tests/deposit_particles_main.cpp as a program of its own under the address and undefined-behaviour sanitizers, over the parameter
table the contract test judges with the restatement: verdicts, the clipped boxes with their texel counts and chunk lists, the 2^24
limit at 2^24 and at 2^24 + 1, the overlap refusals, the argument refusals and the window bounds.  Nothing sanitized is loaded into
this process."""
import os
import subprocess

from tests import deposit_particles_ref as ref
from tests import deposit_particles_sets as sets
from tests import emit_particles_sets as es

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "deposit_particles_main.cpp")
BASE = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build(exe):
    """With the sanitizers (their runtimes linked into the program where the compiler has the archives); without them where it has
    no runtime at all: the comparison with the restatement runs either way."""
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []):
        r = subprocess.run(BASE + extra + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            return extra, r
    raise AssertionError("deposit_particles_main.cpp does not compile:\n" + r.stderr[-4000:])


def test_the_host_checks_and_plans_match_the_restatement_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "deposit_particles_main")
    flags, _ = _build(exe)
    table, expected, names = sets.params_table()
    records = str(tmp_path / "records.bin")
    table.tofile(records)
    limits = ["%d,%s" % (logr, ",".join(str(v) for v in lo + hi)) for logr, lo, hi in sets.LIMIT_BOXES]
    r = subprocess.run([exe, records, "8"] + limits, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "flags %s\n%s\n%s" % (" ".join(flags), r.stdout[-2000:], r.stderr[-6000:])
    lines = r.stdout.splitlines()
    out = dict(line.split(" ", 1) for line in lines if not line.startswith(("args ", "plan ", "limit ")))
    want = [ref.valid(p, 256) for p in table]
    assert int(out["records"]) == table.size
    got = [c == "1" for c in out["verdicts"]]
    assert got == want, [n for n, g, w in zip(names, got, want) if g != w]
    assert got == expected.tolist()
    # the plans: the clipped box, its texels, its chunks, the staging bytes and the scratch words
    plans = dict(line[5:].split(": ", 1) for line in lines if line.startswith("plan "))
    assert sorted(int(k) for k in plans) == [i for i, ok in enumerate(want) if ok]
    seen_empty = seen_many = False
    for i, line in plans.items():
        bb = ref.clipped_box(table[int(i)], 256)
        if bb is None:
            assert line == "empty"
            seen_empty = True
            continue
        chunks = ref.box_chunks(bb)
        ids = [(cz * 4 + cy) * 4 + cx for cx, cy, cz in chunks]
        assert ids == sorted(ids)
        nc = [(int(bb[1][k]) >> 6) - (int(bb[0][k]) >> 6) + 1 for k in range(3)]
        texels = ref.box_texels(bb)
        assert line == "box %s texels %d chunks %d %d %d need %d scratch %d ids%s (%d)" % (
            " ".join(str(int(v)) for v in list(bb[0]) + list(bb[1])), texels, nc[0], nc[1], nc[2], (4 * len(ids) + 15) // 16 * 16,
            texels + len(ids) + 4, "".join(" %d" % c for c in ids[:64]), len(ids)), names[int(i)]
        seen_many |= len(ids) == 8
    assert seen_empty and seen_many
    # the limit: 2^24 texels pass, 2^24 + 1 do not
    got_limits = [line.split(": ", 1)[1] for line in lines if line.startswith("limit ")]
    want_limits = []
    for logr, lo, hi in sets.LIMIT_BOXES:
        bb = ref.clipped_box(ref.params(lo, hi), 1 << logr)
        want_limits.append("valid 1 texels %d allowed %d chunks %d" % (ref.box_texels(bb), ref.box_texels(bb) <= ref.MAX_TEXELS, len(ref.box_chunks(bb))))
    assert got_limits == want_limits
    assert [w.split()[3] for w in want_limits[:2]] == [str(1 << 24), str((1 << 24) + 1)] and [w.split()[5] for w in want_limits] == ["1", "0", "0"]
    assert out["windows"] == "".join("1" if ok else "0" for _, ok in es.WINDOWS)
    assert [ref.window_valid(lr, 256) for lr, _ in es.WINDOWS] == [ok for _, ok in es.WINDOWS]
    args = dict(line[5:].split(": ", 1) for line in lines if line.startswith("args "))
    for name in ("fine", "no draw no counts", "empty", "at the limit", "draw behind states", "counts ends at states"):
        assert args[name] == "ok", name
    assert args["null params"] == args["null params empty"] == "null params" and args["null states"] == "null states"
    assert "2^20" in args["count beyond"]
    for name in ("draw in states", "draw touches the last state", "states in draw", "counts in states", "counts in draw", "counts over the start of states"):
        assert "overlap" in args[name], name
