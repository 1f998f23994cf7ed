"""The host half of the navigation fields that needs no context (raytrace_amd/csrc/api/nav_check.hpp), run by
tests/nav_field_main.cpp as a program of its own under the address and undefined-behaviour sanitizers, over the tables of
tests/nav_field_sets.py: the builds' verdicts, the box test, the launch plans — the largest field (256^3) and others — the samples'
verdicts and the store.  Nothing sanitized is loaded into this process."""
import os
import subprocess

from tests import nav_field_ref as ref
from tests import nav_field_sets as sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "nav_field_main.cpp")
BASE = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SAMPLES = [(0, 1, 1), (0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1 << 20, 0, 0), ((1 << 20) + 1, 0, 0)]


def _build(exe):
    """With the sanitizers (their runtimes linked into the program where the compiler has the archives); without them where it has
    no runtime at all: the comparison with the restatement runs either way."""
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []):
        r = subprocess.run(BASE + extra + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            return extra, r
    raise AssertionError("nav_field_main.cpp does not compile:\n" + r.stderr[-4000:])


def test_the_host_checks_and_plans_match_the_restatement_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "nav_field_main")
    flags, _ = _build(exe)
    builds, boxes, plans = sets.build_table(), sets.box_table(), sets.plan_table()
    lines, want = [], []
    for b in builds:
        lines.append("build %d %d %d %d %d %d %d %d %d %d" % (b[:5] + tuple(b[5]) + b[6:]))
        want.append("build %d" % ref.build_verdict(*b))
    for lo, ext, logr in boxes:
        lines.append("box %d %d %d %d %d %d %d" % (tuple(lo) + tuple(ext) + (logr,)))
        want.append("box %d" % (all(1 <= e <= 256 for e in ext) and ref.box_inside(lo, ext, 1 << logr)))
    for ext, max_dist, levels in plans:
        lines.append("plan %d %d %d %d %d" % (tuple(ext) + (max_dist, levels)))
        tx, ty, halves, bitmap, scratch, block, launches = ref.plan(ext, max_dist, levels)
        want.append("plan %d %d %d %d %d %d %d tiles %d" % (tx, ty, halves, bitmap, scratch, block, launches, tx * ty))
    for count, a_null, s_null in SAMPLES:
        lines.append("sample %d %d %d" % (count, a_null, s_null))
        want.append("sample %d" % (count > 1 << 20 or (count > 0 and (a_null or s_null))))
    want += ["null params 1", "store 64 zero 0 full 1", "reuse 1 1 1 live 64 cells 60"]
    table = tmp_path / "table.txt"
    table.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(table)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "flags %s\n%s\n%s" % (" ".join(flags), r.stdout[-2000:], r.stderr[-6000:])
    got = r.stdout.splitlines()
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:5]
    # the tables say what they are meant to: both verdicts occur, the largest field is planned, its launches are the most there are
    assert {w for w in want if w.startswith("build")} == {"build 0", "build 1"} and {w for w in want if w.startswith("box")} == {"box 0", "box 1"}
    assert ref.plan((256, 256, 256), 4096, 8) == (16, 16, 16, 524288, 4112 + 5 * 524288, 4 * (4112 + 5 * 524288) + 3 * 256 ** 3, 513)
    assert ref.plan((256, 256, 256), 4096, 1)[6] == 4097 and ref.plan((16, 16, 1), 7, 8)[6] == 1 and ref.plan((16, 16, 1), 8, 8)[6] == 2
