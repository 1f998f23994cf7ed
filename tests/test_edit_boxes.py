"""The boxes rt_edit_voxels records for RtConfig.edit_radius (rta::edit_chunk_boxes, raytrace_amd/csrc/api/edit_binning.hpp) on the
CPU: tests/edit_boxes_main.cpp runs that header against a brute-force model, as a program of its own under the address and
undefined-behaviour sanitizers; and tests/edit_history_ref.chunk_boxes, the restatement the GPU tests use, against the same words."""
import os
import subprocess

import numpy as np

from tests import edit_history_ref as er
from tests.test_edit_binning import BASE, SANITIZE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "edit_boxes_main.cpp")


def test_edit_chunk_boxes_match_the_brute_force_model(tmp_path):
    exe = str(tmp_path / "edit_boxes_main")
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []):
        r = subprocess.run(BASE + extra + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            break
    else:
        raise AssertionError("edit_boxes_main.cpp does not compile:\n" + r.stderr[-4000:])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "flags %s\n%s\n%s" % (" ".join(extra), r.stdout[-2000:], r.stderr[-6000:])
    assert "all cases match the model" in r.stdout


def test_the_restatement_makes_the_same_boxes():
    boxes = er.chunk_boxes([(126, 10, 10), (129, 12, 11), (127, 9, 13), (128, 9, 13), (5, 200, 70), (5, 200, 70)], 256)
    got = [(tuple(int(v) for v in lo), tuple(int(v) for v in hi)) for lo, hi in boxes]
    assert got == [((126, 9, 10), (127, 10, 13)), ((128, 9, 11), (129, 12, 13)), ((5, 200, 70), (5, 200, 70))]   # chunks 1, 2, then (0, 3, 1)
    lo, hi = er.world_box((np.array([2, 30, 40]), np.array([4, 32, 49])), (3, -2, 0), 512)
    assert lo.tolist() == [-253.0, -226.0, -216.0] and hi.tolist() == [259.0, -223.0, -206.0]        # cut by the seam in x
    lo, hi = er.world_box((np.array([97, 132, 142]), np.array([99, 134, 151])), (0, 0, 0), 256)
    assert lo.tolist() == [-31.0, 4.0, 14.0] and hi.tolist() == [-28.0, 7.0, 24.0]
