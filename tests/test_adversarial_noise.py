"""The conditions on the inputs of tests/test_gpu_adversarial_noise.py, checked in the oracle on the CPU: the lattice texture makes
a 16 x 16 frame of 256 samples read every (r, g) byte pair exactly once; each cube view shows one face; the degenerate table
entries are what the GPU tests assume (NaN on face 5 with g = 0, z == 0 on face 4 with g = 255, x == +-0 with r = 0) and the
plain cube's face-5 frame takes the NaN branch exactly once per such entry; in the shell world a ray's fate does depend on its
direction; and the oracle's direction and sky formulas agree with the second restatement (tests/shader_formulas.py) over every
entry of the kernels' tables, not a handful."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import adversarial_noise as an
from tests import shader_formulas as sf

W, H, SPP = an.LATTICE_FRAME
SEED0 = an.LATTICE_SEED0


@pytest.fixture(scope="module")
def lattice():
    T = an.lattice_noise()
    T.setflags(write=False)
    return T


def test_lattice_texture_holds_every_pair_once_and_the_frame_reads_each_texel_once(lattice):
    for perm_seed in (0, 1, 7):
        T = lattice if perm_seed == 0 else an.lattice_noise(perm_seed)
        pairs = T[:256, :256, 0].astype(np.int64) | T[:256, :256, 1].astype(np.int64) << 8
        assert len(np.unique(pairs)) == 65536
        reads = an.lattice_reads(W, H, SEED0, SPP, T)
        assert (reads[:256, :256] == 1).all() and reads.sum() == 65536, (perm_seed, reads.sum())
    assert not np.array_equal(an.lattice_noise(1)[:256, :256, :2], lattice[:256, :256, :2])
    assert np.array_equal(an.lattice_reads(W, H, SEED0, SPP), an.lattice_reads(W, H, SEED0, SPP, lattice))
    # the model against the oracle's own lookup, every (sample, pixel)
    seen = np.zeros((512, 512), dtype=np.int64)
    for s in range(SPP):
        for py in range(H):
            for px in range(W):
                _, _, vt, val = po.noise_lookup(lattice, SEED0 + s, px, py)
                seen[vt[1], vt[0]] += 1
                assert val[:2] == tuple(float(np.float32(b) / np.float32(255.0)) for b in lattice[vt[1], vt[0], :2])
    assert np.array_equal(seen, an.lattice_reads(W, H, SEED0, SPP, lattice))
    # a frame that is not the lattice's reads other texels, some of them more than once: the model is not a constant
    other = an.lattice_reads(24, 16, SEED0, SPP, lattice)
    assert other.max() == 2 and other.sum() == 24 * 16 * SPP


@pytest.mark.parametrize("shell", [False, True])
def test_each_view_shows_one_face(shell, lattice):
    mats, mine = an.cube_world(shell)
    for view in an.FACE_VIEWS:
        planes, cn = po.render(mats, mine, lattice, an.view_uniforms(po, view, 0.6), W, H, 1, 0)
        assert (planes["normal_r8"] == view[0]).all(), (view, np.unique(planes["normal_r8"]))
        assert cn.sky_exits == 0 and cn.hits == W * H
    assert sorted(v[0] for v in an.FACE_VIEWS) == [0, 1, 2, 3, 4, 5]
    solid = mine == 0
    assert (mats[solid] != 0).all() and (mats[~solid] == 0).all() and len(np.unique(mats[solid])) > 0.99 * solid.sum()


def test_degenerate_table_entries_are_what_the_gpu_tests_assume():
    for r in range(256):
        assert np.isnan(po.diffuse_direction(5, (r / 255.0, 0.0))).all(), r                 # (0, 0, 1) + (0, 0, -1), normalised
        d = po.diffuse_direction(4, (r / 255.0, 1.0))
        assert d[2] == 0.0 and np.isfinite(d).all() and abs(float(np.hypot(d[0], d[1])) - 1.0) < 1e-6, (r, d)
    with np.errstate(divide="ignore"):
        assert np.isinf(np.float32(1.0) / np.abs(po.diffuse_direction(4, (0.5, 1.0))[2]))   # 1 / |d.z| of trace_ray (:88)
    for face in (2, 3, 4, 5):
        for g in (1, 64, 128, 254):
            assert po.diffuse_direction(face, (0.0, g / 255.0))[0] == 0.0                   # r = 0: x == +-0
    # the NaN entries are exactly face 5 with g = 0: every other entry of every face is finite
    rg = np.stack(np.meshgrid(np.arange(256), np.arange(256)), axis=-1).reshape(-1, 2).astype(np.float32) / np.float32(255.0)
    for face in range(6):
        nan = np.isnan(po.diffuse_direction_n(face, rg)).any(axis=-1)
        assert np.array_equal(nan, (rg[:, 1] == 0) if face == 5 else np.zeros(65536, dtype=bool)), face
    # a NaN direction: one iteration, a border fetch, a non-air hit at a NaN position
    mats, mine = an.cube_world(False)
    h = po.trace_ray(mats, mine, [0.3, 0.2, -64.001], [np.nan] * 3)
    assert h.air == 0 and h.iterations == 1 and h.border_fetches == 1 and np.isnan(h.position[:]).all() and h.packed_material == 0


def test_plain_cube_face5_frame_takes_the_nan_branch_once_per_nan_entry(lattice):
    """Under the cube every diffuse ray leaves the region — except those of the NaN entries (g = 0), which "hit" at a NaN position
    and start a second level there: two more rays, each special as well.  The sun (0.6) stands above, so every shadow ray of level
    1 ends in the cube."""
    mats, mine = an.cube_world(False)
    view = [v for v in an.FACE_VIEWS if v[0] == 5][0]
    reads = an.lattice_reads(W, H, SEED0, SPP, lattice)
    n_nan = int(reads[lattice[..., 1] == 0].sum())           # samples whose noise_value has g == 0
    assert n_nan == 256
    n = W * H * SPP
    _, cn = po.render(mats, mine, lattice, an.view_uniforms(po, view, 0.6), W, H, SPP, 2)
    assert cn.rays_primary == n and cn.rays_shadow == cn.rays_diffuse == n + n_nan
    assert cn.rays == 3 * n + 2 * n_nan
    assert cn.hits == 2 * n + 3 * n_nan                      # primary and shadow of level 1; the NaN diffuse ray and both rays of level 2
    assert cn.sky_exits == n - n_nan and cn.limit_exits == 0
    assert cn.border_fetches == 5 * n_nan                    # the NaN ray's one fetch; level 2's first fetch and the one after its step, twice


def test_shell_world_mixes_sky_exits_and_hits_on_every_face(lattice):
    """Between 10 % and 90 % of the 65 536 diffuse rays of every face leave as sky at depth 1, and so do the 65 536 shadow rays
    under the face's sun of an.FACE_SUN.  A face turned away from the sun has every shadow ray end in the cube at once: its sky
    exits are the diffuse exits alone (the diffuse directions do not depend on the sun)."""
    mats, mine = an.cube_world(True)
    n = W * H * SPP
    measured = {}
    for view in an.FACE_VIEWS:
        face = view[0]
        dark, lit = an.FACE_DARK_SUN[face], an.FACE_SUN[face]
        assert float(np.dot(po.sun(dark)[0], an.FACE_NORMALS[face])) < -0.1 and float(np.dot(po.sun(lit)[0], an.FACE_NORMALS[face])) > 0.1
        _, c_dark = po.render(mats, mine, lattice, an.view_uniforms(po, view, dark), W, H, SPP, 1)
        _, c_lit = po.render(mats, mine, lattice, an.view_uniforms(po, view, lit), W, H, SPP, 1)
        assert c_dark.rays_shadow == c_dark.rays_diffuse == n
        measured[face] = (c_dark.sky_exits / n, (c_lit.sky_exits - c_dark.sky_exits) / n)
    print("face: (diffuse, shadow) sky-exit fractions", {f: (round(a, 3), round(b, 3)) for f, (a, b) in measured.items()})
    for face, (dif, shadow) in measured.items():
        assert 0.1 <= dif <= 0.9 and 0.1 <= shadow <= 0.9, measured
    assert set(an.FACE_SUN.values()) | set(an.FACE_DARK_SUN.values()) <= set(an.SUN_ANGLES)


def test_oracle_agrees_with_the_second_restatement_on_every_table_entry():
    """All 6 x 65 536 (face, r, g) entries, with the tolerances of test_oracle_kat.py::test_k10: diffuse_direction to
    max(2e-6, 6e-7 / |v|) (|v| = the vector's length before its normalisation), sample_sky of that direction to 1e-4, sun vector to
    3e-7; the shadow ray's direction (normalize(sun + (r, g, 0) * 0.05), normalised again by trace_ray) to 2e-6, the diffuse bound at
    |v| ~ 1.  Excluded: the 256 NaN entries by name, entries with |v| < 1e-3, and for the sky the entries within 1e-4 of the sun
    disc's threshold (fp32 and fp64 may fall on either side, as in k10) — at most 1 % in all."""
    bytes_rg = np.stack(np.meshgrid(np.arange(256), np.arange(256)), axis=-1).reshape(-1, 2)      # [g * 256 + r] = (r, g)
    rg32 = bytes_rg.astype(np.float32) / np.float32(255.0)
    rg64 = rg32.astype(np.float64)
    # the vectorised restatements against the scalar ones they repeat
    for face, i in ((0, 0), (5, 513), (4, 65535), (3, 31000), (1, 255 * 256)):
        assert np.allclose(sf.diffuse_direction_n(face, rg64[i:i + 1])[0][0], sf.diffuse_direction(face, rg64[i]), rtol=0, atol=1e-15)
    excluded = 0
    directions = []
    for face in range(6):
        got = po.diffuse_direction_n(face, rg32)
        want, length = sf.diffuse_direction_n(face, rg64)
        named_nan = (bytes_rg[:, 1] == 0) if face == 5 else np.zeros(65536, dtype=bool)
        skip = named_nan | (length < 1e-3)
        assert np.array_equal(np.isnan(got).any(axis=-1), named_nan), face
        excluded += int(skip.sum())
        tol = np.maximum(2e-6, 6e-7 / np.where(skip, 1.0, length))[:, None]
        err = np.abs(got.astype(np.float64) - want)
        bad = ~skip & (err > tol).any(axis=-1)
        assert not bad.any(), (face, bytes_rg[bad][:5], got[bad][:5], want[bad][:5])
        directions.append((got, skip))
    assert excluded <= 0.01 * 6 * 65536, excluded
    for a in an.SUN_ANGLES:
        sky_excluded = 0
        sv, sc = po.sun(a)
        v64 = sf.sun_vector(a)
        c64 = sf.sun_color(v64)
        assert np.allclose(sv, v64, rtol=0, atol=3e-7) and np.allclose(sc, c64, rtol=0, atol=2e-5)
        # shadow directions: the oracle's fp32 operations (trace_sun, then trace_ray's normalize) against fp64 from the fp64 sun vector
        raw = np.stack([sv[0] + rg32[:, 0] * np.float32(0.05), sv[1] + rg32[:, 1] * np.float32(0.05),
                        np.full(65536, sv[2] + np.float32(0.0) * np.float32(0.05), dtype=np.float32)], axis=-1)
        got = po.normalize_n(po.normalize_n(raw))
        want = v64[None, :] + np.concatenate([rg64, np.zeros((65536, 1))], axis=-1) * 0.05
        want /= np.linalg.norm(want, axis=-1)[:, None]
        assert np.abs(got - want).max() <= 2e-6, (a, np.abs(got - want).max())
        for i in (0, 255, 40000, 65535):
            assert np.allclose(want[i], sf.sun_ray_direction(v64, rg64[i]), rtol=0, atol=1e-15)
        for face in range(6):
            d32, skip = directions[face]
            got = po.sample_sky_n(d32, a, True)
            want, sun_amount = sf.sample_sky_n(d32.astype(np.float64), v64, c64, True)
            near_disc = ~skip & (np.abs(sun_amount - 0.98) < 1e-4)
            sky_excluded += int((skip | near_disc).sum())
            use = ~skip & ~near_disc
            worst = float(np.abs(got[use].astype(np.float64) - want[use]).max())
            assert worst < 1e-4, (a, face, worst)
        i = 12345
        assert np.allclose(sf.sample_sky_n(directions[2][0][i:i + 1].astype(np.float64), v64, c64, True)[0][0],
                           sf.sample_sky(directions[2][0][i].astype(np.float64), v64, c64, True), rtol=0, atol=1e-14)
        assert sky_excluded <= 0.01 * 6 * 65536, (a, sky_excluded)
