"""A frame whose prepass inputs are unchanged reuses its slot's prepass: the primary ray reads no noise, so what the prepass leaves in
a frame slot depends on every live uniform but the seed, and on the world.  One long-lived context runs a session — a still camera
with changing seeds, camera changes, a voxel edit, an uploaded and a generated slab, a denoise in place, a sun and an lr change — and
every frame must equal the same session's frame with RT_PREPASS_REUSE=0 and the oracle's, while RtTiming::other_launches shows that
the prepass was skipped on exactly the frames where that is allowed.  Counting and accumulating contexts never reuse."""
import numpy as np
import pytest

from raytrace_amd import abi, render, world
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH, R = 136, 72, 2, 2, 256
CACHE = abi.RT_FLAG_CACHE_PRIMARY
KERNEL = abi.RT_KERNEL_PATHS       # (RT_KERNEL_DEFAULT would draw frames this small on k_frame, which has no prepass)
OTHER_SEED = world.DEFAULT_SEED + 1

CAMERAS = {
    "A": dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.1, sun=0.3, lr=(0, 0, 0)),
    "B": dict(origin=(-24.0, -126.0, 96.0), heading=np.pi / 2 + 0.1, pitch=-0.15, sun=0.3, lr=(0, 0, 0)),
    "C": dict(origin=(-24.0, -126.0, 96.0), heading=np.pi / 2 + 0.1, pitch=-0.15, sun=0.7, lr=(0, 0, 0)),      # B under another sun
    "D": dict(origin=(-24.0, -126.0, 96.0), heading=np.pi / 2 + 0.1, pitch=-0.15, sun=0.7, lr=(16, 0, 0)),     # C through a scrolled window
}
# the session: a camera name draws a frame (seeds count up from 1), anything else is the call of that name
SESSION = ["A", "A", "A", "A", "B", "B", "B", "edit", "B", "B", "B", "slice", "B", "B", "B", "generate", "B", "B", "B",
           "denoise", "B", "B", "B", "C", "C", "C", "D", "D", "D"]


def _u(cam, seed):
    p = CAMERAS[cam]
    return po.camera_uniforms(p["origin"], p["heading"], p["pitch"], p["sun"], seed, p["lr"])


def _expected_reuse(nslots):
    """Per frame of SESSION: does the library's rule allow it to skip the prepass?  A slot remembers the camera of its last prepass;
    a world change forgets every slot's, a denoise the current slot's."""
    held, cur, n, out = [None] * nslots, 0, 0, []
    for op in SESSION:
        if op in CAMERAS:
            cur = n % nslots
            out.append(held[cur] == op)
            held[cur] = op
            n += 1
        elif op == "denoise":
            held[cur] = None
        else:
            held = [None] * nslots
    return out


def _visible_texel(ctx, u):
    """A solid voxel the camera of `u` sees, through the library's own pick."""
    xy = [(W // 2, H // 4), (W // 2, H // 2), (W // 4, H // 8), (W // 2, 2)]
    hits = ctx.pick_pixels(u, xy)
    solid = [h for h in hits if int(h["kind"]) == abi.RT_HIT_SOLID]
    assert solid, "no pick of %s hit terrain" % (xy,)
    return tuple(int(v) for v in solid[0]["texel"])


def _run_session(scene, noise, nslots):
    """-> per frame: (planes, other_launches, the region [z, y, x] the frame was drawn over)."""
    mats, mine = scene
    m3, f3 = mats.reshape(R, R, R), mine.reshape(R, R, R)
    flags = CACHE | abi.RT_FLAG_TIMING_ALL | (abi.RT_FLAG_FRAMES_IN_FLIGHT_2 if nslots == 2 else 0)
    frames, seed = [], 0
    with render.Context(render.make_config(W, H, spp=SPP, depth=DEPTH, kernel=KERNEL, flags=flags)) as ctx:
        assert ctx.info().frames_in_flight == nslots
        ctx.upload_world(mats, mine)
        ctx.upload_noise(noise)
        region = (m3, f3)
        for op in SESSION:
            if op in CAMERAS:
                seed += 1
                ctx.draw_frame(_u(op, seed))
                ctx.sync()
                frames.append((ctx.readback_all(), int(ctx.timing().other_launches), region))
                continue
            if op == "edit":        # a 4^3 hole round a voxel camera B sees
                x, y, z = _visible_texel(ctx, _u("B", seed))
                box = [(a, b, c) for a in range(max(x - 2, 0), min(x + 2, R)) for b in range(max(y - 2, 0), min(y + 2, R))
                       for c in range(max(z - 2, 0), min(z + 2, R))]
                ctx.edit_voxels(box, np.zeros(len(box), np.uint32), np.zeros(len(box), np.uint8))
            elif op == "slice":     # a slab of foreign terrain where the cameras look (tests/test_gpu_overlap.py)
                ctx.upload_slice(1, 96, np.roll(m3[:, 16:32, :], 24, axis=0), np.roll(f3[:, 16:32, :], 24, axis=0))
            elif op == "generate":  # the next slab, of another world
                ctx.generate_slice(OTHER_SEED, 1, (-R // 2, 112 - R // 2, -R // 2))
            elif op == "denoise":
                ctx.denoise(True)
                continue
            region = ctx.read_box((0, 0, 0), (R, R, R))
    return frames


_sessions = {}


def _session(scene, noise, nslots, reuse, monkeypatch):
    if (nslots, reuse) not in _sessions:
        if not reuse:
            monkeypatch.setenv("RT_PREPASS_REUSE", "0")
        _sessions[(nslots, reuse)] = _run_session(scene, noise, nslots)
        monkeypatch.delenv("RT_PREPASS_REUSE", raising=False)
    return _sessions[(nslots, reuse)]


_oracle_frames = []


def _oracle(noise, frames):
    """The oracle's frames of the session, over the regions the (never reusing) run read back after every world change."""
    if not _oracle_frames:
        cams = [op for op in SESSION if op in CAMERAS]
        for i, (cam, (_, _, (m3, f3))) in enumerate(zip(cams, frames)):
            _oracle_frames.append(po.render(m3.reshape(-1), f3.reshape(-1), noise, _u(cam, i + 1), W, H, SPP, DEPTH)[0])
    return _oracle_frames


def _same(a, b, what):
    for name in b:
        assert np.array_equal(a[name], b[name], equal_nan=True), "%s: plane %s differs at %d values" % (
            what, name, int(np.count_nonzero(a[name] != b[name])))


@pytest.mark.parametrize("nslots", [1, 2])
def test_a_session_with_reuse_draws_the_frames_of_one_without(procedural_region, blue_noise, nslots, monkeypatch):
    plain = _session(procedural_region, blue_noise, nslots, False, monkeypatch)
    reused = _session(procedural_region, blue_noise, nslots, True, monkeypatch)
    want = _oracle(blue_noise, _session(procedural_region, blue_noise, 1, False, monkeypatch))
    cams = [op for op in SESSION if op in CAMERAS]
    assert len(plain) == len(reused) == len(want) == len(cams)
    # the world changes are visible to the cameras (else their frames would not show a stale prepass)
    for op in ("edit", "slice", "generate"):
        k = sum(1 for o in SESSION[:SESSION.index(op)] if o in CAMERAS)
        assert not np.array_equal(want[k]["depth_r16"], want[k - 1]["depth_r16"]), op
    for k, cam in enumerate(cams):
        _same(plain[k][0], want[k], "frame %d (%s), RT_PREPASS_REUSE=0, against the oracle" % (k, cam))
        _same(reused[k][0], plain[k][0], "frame %d (%s) against RT_PREPASS_REUSE=0" % (k, cam))


@pytest.mark.parametrize("nslots", [1, 2])
def test_the_prepass_is_skipped_exactly_where_allowed(procedural_region, blue_noise, nslots, monkeypatch):
    plain = _session(procedural_region, blue_noise, nslots, False, monkeypatch)
    reused = _session(procedural_region, blue_noise, nslots, True, monkeypatch)
    saved = [p[1] - r[1] for p, r in zip(plain, reused)]
    assert saved == [1 if e else 0 for e in _expected_reuse(nslots)]
    assert sum(saved) == {1: 17, 2: 10}[nslots]


@pytest.mark.parametrize("nslots", [1, 2])
def test_counting_contexts_count_every_frames_prepass(procedural_region, blue_noise, nslots):
    """RT_FLAG_COUNTERS: three frames of one camera and seed count three times one frame's rays."""
    flags = CACHE | abi.RT_FLAG_COUNTERS | (abi.RT_FLAG_FRAMES_IN_FLIGHT_2 if nslots == 2 else 0)
    counts = {}
    for n in (1, 3):
        with render.Context(render.make_config(W, H, spp=SPP, depth=DEPTH, kernel=KERNEL, flags=flags)) as ctx:
            ctx.upload_world(*procedural_region)
            ctx.upload_noise(blue_noise)
            for _ in range(n):
                ctx.draw_frame(_u("A", 9))
            ctx.sync()
            counts[n] = ctx.counters().as_dict()
    assert counts[1]["rays_primary"] == W * H
    assert counts[3] == {k: 3 * v for k, v in counts[1].items()}


@pytest.mark.parametrize("nslots", [1, 2])
def test_accumulating_contexts_run_every_prepass(procedural_region, blue_noise, nslots):
    """RT_FLAG_ACCUMULATE: three still frames of two samples are the oracle's frame of six (tests/test_gpu_accumulation.py) — the
    prepass of an accumulating frame adds the sky pixels' light to the running sum, so it is never skipped."""
    flags = CACHE | abi.RT_FLAG_ACCUMULATE | (abi.RT_FLAG_FRAMES_IN_FLIGHT_2 if nslots == 2 else 0)
    with render.Context(render.make_config(W, H, spp=SPP, depth=DEPTH, kernel=KERNEL, flags=flags)) as ctx:
        ctx.upload_world(*procedural_region)
        ctx.upload_noise(blue_noise)
        for k in range(3):
            ctx.draw_frame(_u("A", 1 + k * SPP))
        assert ctx.accumulation() == (3, 3 * SPP)
        ctx.sync()
        got = ctx.readback_all()
    _same(got, po.render(*procedural_region, blue_noise, _u("A", 1), W, H, 3 * SPP, DEPTH)[0], "three still frames")
