"""The host half of the voxel-model entities (raytrace_amd/csrc/api/draw_stamps.hpp: a record's verdict, the high corner, the device
record with its packed strides and extents) on the CPU: tests/draw_stamps_main.cpp runs that header against a brute-force model, as a
program of its own under the address and undefined-behaviour sanitizers.  No GPU, no library, nothing loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "draw_stamps_main.cpp")
BASE = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build(exe):
    """With the sanitizers (their runtimes linked into the program where the compiler has the archives); without them where it has
    no runtime at all: the comparison with the model runs either way."""
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []):
        r = subprocess.run(BASE + extra + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            return extra, r
    raise AssertionError("draw_stamps_main.cpp does not compile:\n" + r.stderr[-4000:])


def test_draw_stamps_host_matches_the_brute_force_model(tmp_path):
    exe = str(tmp_path / "draw_stamps_main")
    flags, _ = _build(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "flags %s\n%s\n%s" % (" ".join(flags), r.stdout[-2000:], r.stderr[-6000:])
    assert "all cases match the model" in r.stdout
