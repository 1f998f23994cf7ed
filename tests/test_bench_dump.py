"""bench.py --dump-outputs (the last timed step's planes, for comparing two builds output for output) and --steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402
from raytrace_amd import abi  # noqa: E402

GATHERED = [abi.RT_BUF_LIGHTING_RGBA16, abi.RT_BUF_DEPTH_R16UI, abi.RT_BUF_NORMAL_R8UI, abi.RT_BUF_ALBEDO_RGBA8,
            abi.RT_BUF_EMISSION_RGBA8, abi.RT_BUF_FOG_RGBA8]


def _planes(W, H, seed, flat=False):
    """Planes as bench.py holds them on rank 0: [H,W(,C)] from a context's readback, or the flat bytes of the gathered frame."""
    rng = np.random.default_rng(seed)
    out = {}
    for b in GATHERED:
        dt, ch = abi.BUFFER_FORMATS[b]
        a = rng.integers(0, np.iinfo(dt).max + 1, size=(H, W) + ((ch,) if ch > 1 else ()), dtype=dt)
        out[b] = a.reshape(-1).view(np.uint8) if flat else a
    return out


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_of_a_small_frame_is_the_whole_frame(tmp_path):
    planes = _planes(40, 24, 1)
    bench.dump_outputs(str(tmp_path), planes)
    got = _load(tmp_path)
    assert sorted(got) == sorted(abi.BUFFER_NAMES[b] for b in GATHERED)
    for b in GATHERED:
        a = got[abi.BUFFER_NAMES[b]]
        ch = abi.BUFFER_FORMATS[b][1]
        assert a.dtype == np.float32 and a.shape == (40 * 24, ch)
        assert np.array_equal(a, planes[b].reshape(-1, ch).astype(np.float32))
    # the flat byte planes of a gathered frame dump to the same arrays
    bench.dump_outputs(str(tmp_path / "flat"), _planes(40, 24, 1, flat=True))
    for name, a in _load(tmp_path / "flat").items():
        assert np.array_equal(a, got[name]), name


def test_dump_of_a_headline_frame_is_a_fixed_sample_under_64_mb(tmp_path):
    W, H = 1920, 1080
    planes = _planes(W, H, 2)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), planes)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    idx = a["pixel_index"]
    assert idx.dtype == np.float64 and idx.shape == (bench.DUMP_MAX_PIXELS,)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < W * H
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    pix = idx.astype(np.int64)
    for p in GATHERED:
        ch = abi.BUFFER_FORMATS[p][1]
        assert np.array_equal(a[abi.BUFFER_NAMES[p]], planes[p].reshape(-1, ch)[pix].astype(np.float32))
    # a later, unsampled dump into the same directory leaves no stale index behind
    bench.dump_outputs(str(tmp_path / "a"), _planes(40, 24, 3))
    assert "pixel_index" not in _load(tmp_path / "a")


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, "bench.py", "--steps", "0"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_dumps_the_frame_its_last_timed_step_drew(tmp_path, procedural_region, blue_noise):
    """Two runs with the same arguments dump the same planes, and they are the frame a context renders for those arguments."""
    from raytrace_amd import render
    W, H, spp, depth = 200, 120, 4, 3
    common = ["--gpus", "1", "--width", str(W), "--height", str(H), "--spp", str(spp), "--depth", str(depth), "--steps", "3",
              "--warmup", "1", "--no-cpu-baseline", "--no-reference-frame"]
    dumps = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, "bench.py"] + common + ["--dump-outputs", str(tmp_path / d)], cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        dumps.append(_load(tmp_path / d))
    assert sorted(dumps[0]) == sorted(abi.BUFFER_NAMES[b] for b in GATHERED)
    for name in dumps[0]:
        assert np.array_equal(dumps[0][name], dumps[1][name]), name
    mats, mine = procedural_region
    p = render.DEFAULT_POSE
    u = render.camera_uniforms(p["origin"], p["heading"], p["pitch"], p["sun_angle"], seed=1)
    cfg = render.make_config(W, H, spp=spp, depth=depth, flags=abi.RT_FLAG_CACHE_PRIMARY | abi.RT_FLAG_FRAMES_IN_FLIGHT_2)
    with render.Context(cfg) as ctx:
        ctx.upload_world(mats, mine)
        ctx.upload_noise(blue_noise)
        ctx.draw_frame(u)
        ctx.sync()
        for b in GATHERED:
            ch = abi.BUFFER_FORMATS[b][1]
            assert np.array_equal(dumps[0][abi.BUFFER_NAMES[b]], ctx.readback(b).reshape(-1, ch).astype(np.float32)), abi.BUFFER_NAMES[b]
