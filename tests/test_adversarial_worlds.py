"""The inputs of tests/test_gpu_adversarial_worlds.py, checked on the CPU: the two world builders (tests/adversarial_worlds.py) are
what they claim to be, the frames the GPU tests draw really fetch every minefield value 0..30 from the bricks and read every
albedo code, and the oracle agrees with the second restatements (tests/shader_trace.py, tests/shader_post.py) on these inputs —
so that the GPU's agreement with the oracle there means something."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import adversarial_worlds as aw
from tests import synthetic_planes as sp_planes

pytestmark = pytest.mark.usefixtures("native_built")

# the frames tests/test_gpu_adversarial_worlds.py draws at region 256: (pose index, W, H, spp, depth)
FRAMES_256 = [(0, 40, 29, 1, 0), (1, 37, 22, 2, 2), (2, 48, 40, 1, 4), (3, 45, 33, 3, 5), (4, 32, 24, 2, 8), (0, 24, 19, 1, 9)]


@pytest.fixture(scope="module")
def arbitrary256(native_built):
    return aw.arbitrary_world(256)


@pytest.fixture(scope="module")
def pyramid256(native_built):
    return aw.pyramid_world(256)


@pytest.mark.parametrize("R", [256, 512])
def test_pyramid_world_is_pack_into_without_the_chunk_cap(R):
    """Capped at 6 the region-wide pyramid IS pack_into's per-chunk minefield (an aligned cube of edge <= 64 lies inside one chunk);
    above 6 it holds the values the palette worlds never have, in whole uniform coarse cubes."""
    mats, pyr, mine = aw.pyramid_world(R)
    assert np.array_equal(np.minimum(pyr, 6), mine)
    logr = R.bit_length() - 1
    assert pyr.max() == logr - 1 and (pyr == 7).sum() > 0
    # the defining property, on a sample of empty voxels: the cube of edge 2^v is occupied, the one of edge 2^(v-1) is not
    rng = np.random.default_rng(R)
    solid = pyr == 0
    for _ in range(200):
        z, y, x = (int(c) for c in rng.integers(0, R, size=3))
        v = int(pyr[z, y, x])
        if v == 0:
            continue
        s = 1 << v
        assert solid[z // s * s:(z // s + 1) * s, y // s * s:(y // s + 1) * s, x // s * s:(x // s + 1) * s].any()
        if v > 1:
            s >>= 1
            assert not solid[z // s * s:(z // s + 1) * s, y // s * s:(y // s + 1) * s, x // s * s:(x // s + 1) * s].any()
    # uniform coarse cubes (edge R/64) holding 7: the nibble map's uniform fast path above the palette's range
    e = R // 64
    c = pyr.reshape(64, e, 64, e, 64, e)
    cmin, cmax = c.min(axis=(1, 3, 5)), c.max(axis=(1, 3, 5))
    assert ((cmin == cmax) & (cmin == 7)).sum() > 100


@pytest.mark.parametrize("R", [256, 512])
def test_arbitrary_world_covers_the_encodings(R):
    mats, mine, kinds, vals = aw.arbitrary_world(R)
    assert mine.max() == 30
    e = R // 64
    c = mine.reshape(64, e, 64, e, 64, e)
    cmin, cmax = c.min(axis=(1, 3, 5)), c.max(axis=(1, 3, 5))
    uni = cmin == cmax
    assert np.array_equal(uni, kinds == aw.KIND_UNIFORM)
    counts = np.bincount(cmin[uni], minlength=31)
    assert counts.min() > 20, counts                                   # every uniform value 0..30
    for v in (6, 7, 14, 15, 16, 30):
        assert counts[v] > 1000 if R == 256 else counts[v] > 500, (v, counts)
    mixed = kinds == aw.KIND_MIXED
    assert (cmax[mixed] >= 15).all() and (cmin[mixed] == 0).mean() > 0.5
    # "uniform 1 except one solid voxel": exactly one 0 per cube, at every offset of a 4^3 brick and in every brick of the cube
    odd = kinds == aw.KIND_ODD
    assert (cmin[odd] == 0).all() and (cmax[odd] == 1).all()
    assert ((c == 0).sum(axis=(1, 3, 5))[odd] == 1).all()
    zs, ys, xs = np.nonzero((mine == 0) & np.broadcast_to(odd[:, None, :, None, :, None], c.shape).reshape(R, R, R))
    assert len(set(((zs & 3) * 16 + (ys & 3) * 4 + (xs & 3)).tolist())) == 64
    assert len(set((((zs % e) >> 2) * 16 + ((ys % e) >> 2) * 4 + ((xs % e) >> 2)).tolist())) == (e // 4) ** 3
    # material words: all 32 bits, every 7-bit albedo code in every channel among the solid voxels, and solid voxels with word 0
    words = mats[mine == 0]
    assert (words >> 21).max() > 0 and (words == 0).sum() > 100
    for s in (14, 7, 0):
        assert len(np.unique((words >> s) & 0x7F)) == 128


def test_frames_fetch_every_minefield_value_and_read_every_albedo_code(arbitrary256, pyramid256, blue_noise):
    """The oracle's fetch histogram (per value: fetched from a 4^3 brick of one value, or from a mixed one) over the frames the
    GPU tests draw on the arbitrary world: every value 0..30 is fetched, 0..15 from uniform bricks (15 is the nibble map's
    "mixed" code: a uniform 15 brick takes the byte path), 15..30 from mixed bricks too.  The primary albedo planes hold at least
    100 of the 128 codes per channel (UNORM8 of code / 127 is injective, so the code can be read back)."""
    mats, mine = arbitrary256[:2]
    hist = np.zeros((2, 32), dtype=np.uint64)
    codes = [set(), set(), set()]
    for pose, W, H, spp, depth in FRAMES_256:
        u = aw.pose_uniforms(po, aw.POSES[pose], 256)
        planes, cn, h = po.fetch_histogram(mats, mine, blue_noise, u, W, H, spp, depth)
        hist += h
        hit = planes["normal_r8"] != 16
        assert cn.hits > 0 and hit.mean() > 0.3, (pose, hit.mean())
        for ch in range(3):
            codes[ch] |= set(planes["albedo_rgba8"][..., ch][hit].tolist())
    uniform, mixed = hist[1], hist[0]
    assert (uniform + mixed)[:31].min() > 0 and hist[:, 31].sum() == 0
    assert uniform[:16].min() > 0, uniform
    assert mixed[15:31].min() > 0, mixed
    want = {int(np.rint(np.float32(np.float32(k) / np.float32(127)) * np.float32(255))) for k in range(128)}
    assert len(want) == 128
    for ch in range(3):
        assert codes[ch] <= want and len(codes[ch]) >= 100, (ch, len(codes[ch]))
    # the pyramid world's sky: 7 fetched from uniform bricks
    mats, pyr, _ = pyramid256
    u = aw.pose_uniforms(po, dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=0.0, sun=0.0, lr=(0, 0, 0)), 256)
    _, _, h = po.fetch_histogram(mats, pyr, blue_noise, u, 40, 30, 1, 2)
    assert h[1][7] > 1000 and h[:, 8:].sum() == 0


def _same_ray(h, r, what):
    assert bool(h.limit_exit) == r["limit"], what
    assert h.normal == r["normal"] and h.iterations == r["iterations"], (what, h.normal, r["normal"], h.iterations, r["iterations"])
    got = np.array(list(h.position[:]) + [h.distance], dtype=np.float32).view(np.uint32)
    want = np.array(r["position"] + [r["distance"]], dtype=np.float32).view(np.uint32)
    assert (got == want).all(), (what, h.position[:], r["position"], h.distance, r["distance"])
    if r["limit"]:
        return
    assert bool(h.air) == r["air"], what
    if not r["air"]:
        assert h.packed_material == r["packed_material"], what
        assert (np.array(h.albedo[:], dtype=np.float32).view(np.uint32) == np.array(r["albedo"], dtype=np.float32).view(np.uint32)).all(), what


def test_oracle_trace_ray_against_the_second_restatement(arbitrary256, pyramid256):
    """po.trace_ray against tests/shader_trace.py, bit for bit, on both worlds: rays that start on values 15..30 (step sizes up
    to 2^29), on the pyramid's 7s, from outside the region, through a scrolled window (lr != 0), and from anywhere."""
    from tests import shader_trace as st
    rng = np.random.default_rng(31)

    def rand_dir():
        d = rng.normal(size=3)
        return tuple((d / np.linalg.norm(d)).astype(np.float32))

    def start_on(mine, lo, hi, n):
        cand = np.argwhere((mine >= lo) & (mine <= hi))
        pick = cand[rng.integers(0, len(cand), size=n)]
        return [tuple(float(np.float32(p[2 - a] - 128 + rng.random())) for a in range(3)) for p in pick]

    mats, mine = arbitrary256[:2]
    pmats, pyr, _ = pyramid256
    hits = {"arbitrary": 0, "pyramid": 0}
    started = set()
    cases = []
    for o in start_on(mine, 15, 30, 90):
        cases.append(("arbitrary", o, rand_dir(), (0, 0, 0)))
    for o in start_on(mine, 1, 14, 60):
        cases.append(("arbitrary", o, rand_dir(), (0, 0, 0)))
    for o in start_on(pyr, 7, 7, 40) + start_on(pyr, 1, 6, 30):
        cases.append(("pyramid", o, rand_dir(), (0, 0, 0)))
    for name in ("arbitrary", "pyramid"):
        for _ in range(25):                      # from outside the region, towards it
            o = np.array(rng.uniform(-110, 110, size=3))
            a = int(rng.integers(0, 3))
            o[a] = float(rng.choice([-1, 1]) * rng.uniform(129, 200))
            d = np.array(rand_dir(), dtype=np.float64)
            d[a] = -np.sign(o[a]) * abs(d[a])
            cases.append((name, tuple(float(x) for x in o), tuple(d.astype(np.float32)), (0, 0, 0)))
        for lr in ((16, -32, 16), (-48, 0, 112)):    # a scrolled window: positions around lr, the texture wraps
            for _ in range(20):
                o = tuple(float(lr[a] + rng.uniform(-110, 110)) for a in range(3))
                cases.append((name, o, rand_dir(), lr))
    for name, o, d, lr in cases:
        m, f = (mats, mine) if name == "arbitrary" else (pmats, pyr)
        t = tuple(int(np.floor((np.float32(o[a]) + np.float32(128)) % np.float32(256))) for a in range(3))
        started.add((name, int(f[t[2], t[1], t[0]])))
        h = po.trace_ray(m, f, o, d, lr=lr)
        _same_ray(h, st.trace_ray(m, f, o, d, lr=lr), (name, o, d, lr))
        hits[name] += int(not h.air and not h.limit_exit)
    assert {v for n, v in started if n == "arbitrary"} >= set(range(15, 31))
    assert ("pyramid", 7) in started
    assert hits["arbitrary"] > 20 and hits["pyramid"] > 20, hits


@pytest.mark.parametrize("W,H", [(1, 1), (3, 50), (333, 77)])
def test_oracle_post_passes_on_synthetic_planes_against_the_second_restatement(W, H, blue_noise):
    """po.denoise / po.finalize against tests/shader_post.py on planes a rendered frame never holds (tests/synthetic_planes.py),
    with test_post_passes' tolerances: 3 of 65535 per denoised channel, 0.52 of 255 per finalized one."""
    from tests import shader_post as sp
    p = sp_planes.post_planes(W, H, seed=W * 1000 + H)
    for faithful in (True, False):
        got = po.denoise(p["lighting"], p["depth"], p["normal"], faithful).astype(np.int64)
        want = sp.denoise(p["lighting"], p["depth"], p["normal"], faithful).astype(np.int64)
        assert np.abs(got - want).max() <= 3, (faithful, np.abs(got - want).max())
        assert (got[..., 3] == want[..., 3]).all()
        den = got.astype(np.uint16)
        out = po.finalize(p["albedo"], p["emission"], p["fog"], den, p["depth"], blue_noise)
        real = sp.finalize(p["albedo"], p["emission"], p["fog"], den, p["depth"], blue_noise)
        assert np.abs(out[..., [2, 1, 0]].astype(np.float64) - real).max() <= 0.52
        assert (out[..., 3] == 255).all()
    if W * H > 1000:
        assert sp_planes.near_pixels_moved_by_the_pong_passes(po, p) > 10
        assert len(np.unique(p["normal"])) == 256
        assert (p["depth"] >= 32768).any() and (p["depth"] == 0xFFFF).any() and (p["depth"] < 16).any()
