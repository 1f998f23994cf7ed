"""The host's own checks of rt_sweep_entities' arguments (raytrace_amd/csrc/api/sweep_entities_check.hpp), run by
tests/sweep_entities_main.cpp as a program of its own under the address and undefined-behaviour sanitizers, over tables the
restatements judge.  Nothing sanitized is loaded into this process."""
import os
import subprocess

import numpy as np

from tests import entity_query_ref as eq
from tests import sweep_entities_ref as ref
from tests import sweep_entities_sets as sets
from tests import sweep_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sweep_entities_main.cpp")
BASE = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-mfma"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
f32 = np.float32


def _build(exe):
    """With the sanitizers (their runtimes linked into the program where the compiler has the archives); without them where it has
    no runtime at all: the comparison with the restatements runs either way."""
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []):
        r = subprocess.run(BASE + extra + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            return extra, r
    raise AssertionError("sweep_entities_main.cpp does not compile:\n" + r.stderr[-4000:])


def sweep_table():
    """Sweeps inside the domain, on its edges and outside it, with every value of the reserved words."""
    stamps = sets.stamps_by_id()
    good = sets.seeded(24, 24, 6, 0, sorted(stamps), stamps)["sweeps"]
    good["reserved0"], good["reserved1"], good["reserved2"] = np.arange(24), 0xFFFFFFFF, 7
    bad, which = sets.invalid(good)
    edge = ref.make_sweeps([[4194296.0, 0, 0], [-4194304.0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]],
                           [[4194304.0, 1, 1], [-4194296.0, 1, 1], [8, 8, 8], [np.nextafter(f32(8), f32(9)), 1, 1], [1, 1, 1], [1, 1, 1]],
                           [[64, -64, 0], [0, 0, 0], [-0.0, 0, 0], [0, 0, 0], [np.nextafter(f32(64), f32(65)), 0, 0], [0, -np.inf, 0]])
    return np.concatenate([good[:5], bad, edge])


def box_table():
    b = sets.boxes_of([[0, 0, 0]] * 8, [[1, 1, 1]] * 8)
    b["hi"][1, 0] = 0.0                            # flat
    b["lo"][2, 1] = np.nan
    b["hi"][3, 2] = np.inf
    b["lo"][4], b["hi"][4] = -4194304.0, 4194304.0
    b["hi"][5, 0] = np.nextafter(f32(4194304.0), f32(np.inf))
    b["lo"][6, 2], b["hi"][6, 2] = 2.0, 1.0        # inside out
    return b


def test_the_argument_checks_match_the_restatements_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "sweep_entities_main")
    flags, _ = _build(exe)
    sweeps, boxes = sweep_table(), box_table()
    fs, fb = str(tmp_path / "sweeps.bin"), str(tmp_path / "boxes.bin")
    sweeps.tofile(fs)
    boxes.tofile(fb)
    r = subprocess.run([exe, fs, fb], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "flags %s\n%s\n%s" % (" ".join(flags), r.stdout[-2000:], r.stderr[-6000:])
    out = dict(line.split(" ", 1) for line in r.stdout.splitlines() if not line.startswith("args "))
    want = ["1" if sr.in_domain(s["lo"], s["hi"], s["motion"]) else "0" for s in sweeps]
    assert list(out["sweeps"]) == want and want.count("0") >= 8 and want.count("1") >= 8
    assert int(out["first_invalid_sweep"]) == want.index("0")
    want = ["1" if ref.box_valid(b["lo"], b["hi"]) else "0" for b in boxes]
    assert list(out["boxes"]) == want == list("10001001")
    assert int(out["first_invalid_box"]) == 1 and out["prefixes"] == "1"
    # the models' record rule, judged by the entity queries' restatement of it
    stamps = {1: sets.stamp_arrays((3, 11, 4), 3, 1.0)}
    models = sets.models_of(1, [[1.5, -2.0, 0.25]] * 8, 0.5, 13)
    models["orient"][1], models["scale"][2], models["scale"][3], models["reserved"][4], models["reserved0"][5, 1] = 48, 1.0 / 512.0, 65.0, 1, 1
    models["origin"][6, 2] = 4194304.0
    models["origin"][7, 0], models["scale"][7] = -4194304.0, 64.0
    assert list(out["models"]) == ["1" if eq.model_valid(m, stamps) else "0" for m in models] == list("10000001")
    args = dict(line[5:].split(": ", 1) for line in r.stdout.splitlines() if line.startswith("args "))
    for fine in ("fine", "no entities", "empty", "empty with entities", "counts at the limits"):
        assert args[fine] == "ok", fine
    assert "2^24 sweeps" in args["sweeps beyond"] and "4096 boxes" in args["boxes beyond"] and "4096 models" in args["models beyond"]
    assert args["null sweeps"] == args["null lr"] == args["null hits"] == args["null boxes"] == args["null models"] == "null pointer"
