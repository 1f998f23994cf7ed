"""The host's own validity test of RtParticleState records and RtParticleStep parameters
(raytrace_amd/csrc/api/particle_step_check.hpp), run by tests/particle_step_main.cpp as a program of its own under the address and
undefined-behaviour sanitizers, over the tables the contract test judges with the restatement.  Nothing sanitized is loaded into
this process."""
import os
import subprocess

import numpy as np

from raytrace_amd import abi, render
from tests import particle_step_ref as ref
from tests import particle_step_sets as sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "particle_step_main.cpp")
BASE = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build(exe):
    """With the sanitizers (their runtimes linked into the program where the compiler has the archives); without them where it has
    no runtime at all: the comparison with the restatement runs either way."""
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []):
        r = subprocess.run(BASE + extra + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            return extra, r
    raise AssertionError("particle_step_main.cpp does not compile:\n" + r.stderr[-4000:])


def _param_records():
    """The parameter table as RtParticleStep records (built field by field: make_particle_step would refuse the bad ones)."""
    rows = sets.params_table()
    recs = np.zeros(len(rows), dtype=np.dtype(abi.RtParticleStep))
    for i, (_, kw, _) in enumerate(rows):
        recs[i]["dt"], recs[i]["accel"], recs[i]["damping"], recs[i]["restitution"] = kw["dt"], kw["accel"], kw["damping"], kw["restitution"]
        recs[i]["friction"], recs[i]["rest_speed"], recs[i]["sweeps"] = kw["friction"], kw["rest_speed"], kw["sweeps"]
    return recs, rows


def test_the_validity_checks_match_the_restatement_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "particle_step_main")
    flags, _ = _build(exe)
    table, verdicts, names = sets.record_table()
    params, rows = _param_records()
    records, pfile = str(tmp_path / "records.bin"), str(tmp_path / "params.bin")
    table.tofile(records)
    params.tofile(pfile)
    r = subprocess.run([exe, records, pfile], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "flags %s\n%s\n%s" % (" ".join(flags), r.stdout[-2000:], r.stderr[-6000:])
    out = dict(line.split(" ", 1) for line in r.stdout.splitlines() if not line.startswith("args "))
    assert int(out["records"]) == table.size
    want = ["x" if ref.inactive(s) else ("v" if ref.valid(s) else "i") for s in table]
    got = list(out["verdicts"])
    assert got == want, [n for n, g, w in zip(names, got, want) if g != w]
    assert got == [dict(valid="v", invalid="i", inactive="x")[v] for v in verdicts]
    assert int(out["first_invalid"]) == want.index("i") and out["prefixes"] == "1"
    got = [c == "1" for c in out["params"]]
    assert got == [ref.params_valid(ref.Params(**kw)) for _, kw, _ in rows] == [ok for _, _, ok in rows], \
        [name for (name, _, ok), g in zip(rows, got) if g != ok]
    args = dict(line[5:].split(": ", 1) for line in r.stdout.splitlines() if line.startswith("args "))
    for fine in ("fine", "in place", "no draw", "empty", "count at the limit", "out just behind in", "draw just in front of in"):
        assert args[fine] == "ok", fine
    assert args["null params"] == args["null in"] == args["null out"] == "null pointer"
    assert "2^20 particles" in args["count beyond"]
    assert args["out one record into in"] == args["in one record into out"] == "in and out overlap without being equal"
    assert args["draw inside in"] == args["draw reaches into out"] == "draw overlaps in or out"


def test_make_particle_step_refuses_what_the_host_check_refuses():
    import pytest
    for name, kw, ok in sets.params_table():
        if ok:
            p = render.make_particle_step(**kw)
            assert (p.sweeps, np.float32(p.dt)) == (kw["sweeps"], np.float32(kw["dt"])), name
        else:
            with pytest.raises(ValueError):
                render.make_particle_step(**kw)
