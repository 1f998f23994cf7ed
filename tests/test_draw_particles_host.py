"""The host's own validity test of RtParticle records (raytrace_amd/csrc/api/particles_check.hpp), run by
tests/draw_particles_main.cpp as a program of its own under the address and undefined-behaviour sanitizers, over the record table the
contract test judges with the restatement.  Nothing sanitized is loaded into this process."""
import os
import subprocess

from tests import draw_particles_ref as ref
from tests import draw_particles_sets as sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "draw_particles_main.cpp")
BASE = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build(exe):
    """With the sanitizers (their runtimes linked into the program where the compiler has the archives); without them where it has
    no runtime at all: the comparison with the restatement runs either way."""
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []):
        r = subprocess.run(BASE + extra + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            return extra, r
    raise AssertionError("draw_particles_main.cpp does not compile:\n" + r.stderr[-4000:])


def test_the_validity_check_matches_the_restatement_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "draw_particles_main")
    flags, _ = _build(exe)
    table, expected, names = sets.record_table()
    records = str(tmp_path / "records.bin")
    table.tofile(records)
    r = subprocess.run([exe, records, str(sets.TABLE_LIGHTS)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "flags %s\n%s\n%s" % (" ".join(flags), r.stdout[-2000:], r.stderr[-6000:])
    out = dict(line.split(" ", 1) for line in r.stdout.splitlines() if not line.startswith("args "))
    want = ref.valid(table, sets.TABLE_LIGHTS)
    assert int(out["records"]) == table.size
    got = [c == "1" for c in out["verdicts"]]
    assert got == want.tolist(), [n for n, g, w in zip(names, got, want) if g != w]
    assert got == expected.tolist()
    assert int(out["first_invalid"]) == int(np_first_false(want)) and out["prefixes"] == "1"
    args = dict(line[5:].split(": ", 1) for line in r.stdout.splitlines() if line.startswith("args "))
    assert args["fine"] == args["empty"] == args["count at the limit"] == "ok"
    assert args["null uniforms"] == "null uniforms" and args["null particles"] == args["null lights"] == "null pointer"
    assert "2^20 particles" in args["count beyond"] and "2^20 lights" in args["lights beyond"] and "at least one light" in args["no lights"]


def np_first_false(mask):
    bad = [i for i, ok in enumerate(mask.tolist()) if not ok]
    return bad[0] if bad else len(mask)
