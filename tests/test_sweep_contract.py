"""The box-sweep rules on their restatement alone (tests/sweep_ref.py; no GPU): closure of chained sweeps, soundness and tightness
against a float64 brute force, the named cases, and the conditions on the input sets the GPU tests use (tests/test_gpu_sweeps.py
imports the samplers from here, so that what is asserted about them here is what runs there).

Coordinates stay below 2^10 in these tests, where an fp32 ulp is at most 6.1e-5: the 1e-3 margins of the brute force are 16 ulps."""
import numpy as np
import pytest

from raytrace_amd import world
from tests import ray_query_ref as rq
from tests import scenes
from tests import sweep_ref as sr

f32 = np.float32
PLAYER = np.float32([0.6, 0.6, 1.8])
EPS = 1e-3


# ---- worlds ---------------------------------------------------------------------------------------------------------------------
def world_order(occ):
    """bool[R, R, R] occupancy indexed [z][y][x] by world voxel minus the window's low corner lr - R/2."""
    solid = occ.minefield == 0
    for axis, a in ((0, 2), (1, 1), (2, 0)):
        solid = np.roll(solid, -occ.lr[a], axis=axis)
    return solid


def surface_heights(occ):
    """int[R, R] indexed [y][x] in world order: world z of the top of the highest occupied voxel of each column (its z + 1); the
    window's bottom where the column is empty."""
    solid = world_order(occ)
    R = occ.R
    top = R - np.argmax(solid[::-1], axis=0)
    top[~solid.any(axis=0)] = 0
    return top + occ.lr[2] - R // 2


@pytest.fixture(scope="module")
def terrain(procedural_region):
    mats, mine = procedural_region
    return sr.Occupancy(mats, mine, (0, 0, 0), 256)


@pytest.fixture(scope="module")
def staircase(native_built):
    return sr.Occupancy(*world.region_from_ids(scenes.staircase_ids()), (0, 0, 0), 256)


@pytest.fixture(scope="module")
def blocks(native_built):
    return sr.Occupancy(*world.region_from_ids(scenes.random_blocks_ids()), (0, 0, 0), 256)


# ---- samplers (shared with the GPU tests) ----------------------------------------------------------------------------------------
def random_motions(rng, n, longest=3.0):
    """float32[n, 3]: random directions, length 0.2 .. `longest`; a fifth with one component zero, a tenth along one axis, a few zero.
    A component that is not zero is at least a twentieth of the length, so that no motion grazes an axis."""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    small = np.abs(d) < 0.05
    d[small] = np.where(d[small] < 0, -0.05, 0.05)
    m = d * rng.uniform(0.2, longest, (n, 1))
    u = rng.random(n)
    one = rng.integers(0, 3, n)
    m[(u < 0.2), one[u < 0.2]] = 0.0                       # one component zero
    along = (u >= 0.2) & (u < 0.3)                         # along one axis
    keep = np.zeros((n, 3), bool)
    keep[np.arange(n), one] = True
    m[along[:, None] & ~keep] = 0.0
    m[(u >= 0.3) & (u < 0.31)] = 0.0                       # no motion at all
    return m.astype(np.float32)


def surface_sweeps(occ, n, seed, heights=None):
    """float32[n, 3, 3] sweeps (lo, hi, motion) that start near the surface of `occ`: mostly player-sized boxes standing on, hovering
    just above or sunk just into the highest voxel of a random column, some with faces on integer planes; one in fifty starts just
    below the window's floor and moves up into it (outside the window is air: the one way to meet a face from below on terrain
    that has no overhang)."""
    rng = np.random.default_rng(seed)
    R, lr = occ.R, np.asarray(occ.lr)
    h = surface_heights(occ) if heights is None else heights
    ix = rng.integers(16, R - 16, n)
    iy = rng.integers(16, R - 16, n)
    base = np.stack([ix + lr[0] - R // 2, iy + lr[1] - R // 2, h[iy, ix]], 1).astype(np.float64)
    u = rng.random(n)
    dz = np.where(u < 0.3, 0.0, np.where(u < 0.65, rng.uniform(0.0, 1.5, n), np.where(u < 0.72, rng.uniform(-1.5, 0.0, n), rng.uniform(0.0, 4.0, n))))
    frac = rng.random((n, 2))
    frac[rng.random(n) < 0.15] = 0.0                       # faces on integer planes in x and y
    size = np.tile(PLAYER.astype(np.float64), (n, 1))
    odd = rng.random(n) < 0.25
    size[odd] = rng.uniform(0.3, 3.0, (int(odd.sum()), 3))
    whole = rng.random(n) < 0.1
    size[whole] = np.round(size[whole]) + 1.0              # integer extents: both faces aligned when the corner is
    lo = base + np.concatenate([frac, dz[:, None]], 1)
    m = random_motions(rng, n).astype(np.float64)
    m[:, 2] -= np.where(rng.random(n) < 0.5, rng.uniform(0.0, 1.0, n), 0.0) * (m[:, 2] != 0)   # gravity on half of them
    below = rng.random(n) < 0.02
    lo[below, 2] = lr[2] - R // 2 - size[below, 2] - rng.uniform(0.0, 0.5, int(below.sum()))
    m[below, 2] = rng.uniform(0.6, 2.0, int(below.sum()))
    out = np.zeros((n, 3, 3), np.float32)
    out[:, 0] = lo
    out[:, 1] = out[:, 0] + size.astype(np.float32)
    out[:, 2] = m
    return out


def scene_sweeps(occ, n, seed, longest=6.0):
    """float32[n, 3, 3] sweeps among the occupied voxels of any world: boxes placed beside random occupied voxels that have an empty
    neighbour (on the torus of texels), moving up to `longest`; some long enough to cross many cells."""
    rng = np.random.default_rng(seed)
    full = occ.minefield == 0
    buried = full.copy()
    for axis in range(3):
        buried &= np.roll(full, 1, axis) & np.roll(full, -1, axis)
    solid = np.argwhere(full & ~buried)
    t = solid[rng.integers(0, len(solid), n)][:, ::-1]
    lr = np.asarray(occ.lr)
    v = lr - occ.R // 2 + (t - lr) % occ.R
    size = np.where(rng.random((n, 1)) < 0.6, PLAYER.astype(np.float64), rng.uniform(0.3, 4.0, (n, 3)))
    off = rng.uniform(-3.0, 3.0, (n, 3))
    aligned = rng.random(n) < 0.2
    off[aligned] = np.round(off[aligned])
    out = np.zeros((n, 3, 3), np.float32)
    out[:, 0] = v + off
    out[:, 1] = out[:, 0] + size.astype(np.float32)
    out[:, 2] = random_motions(rng, n, longest)
    for i in range(n):                                     # most of the boxes that start inside a voxel get other places to try
        for _ in range(6 if i % 8 else 0):
            if sr.sweep(occ, out[i, 0], out[i, 1], (0, 0, 0))["kind"] != sr.EMBEDDED:
                break
            o = rng.uniform(-3.0, 3.0, 3)
            out[i, 0] = v[i] + (np.round(o) if aligned[i] else o)
            out[i, 1] = out[i, 0] + size[i].astype(np.float32)
    return out


TERRAIN_BATCH = dict(n=4096, seed=41)


def has_aligned_face(s):
    return bool(((s[0] == np.floor(s[0])) | (s[1] == np.floor(s[1]))).any())


# ---- float64 brute force -----------------------------------------------------------------------------------------------------------
def _overlaps_any(occ, lo, hi):
    """Does the open float64 box (lo, hi) overlap an occupied voxel?"""
    c = [(int(np.floor(lo[a])), int(np.ceil(hi[a])) - 1) for a in range(3)]
    return occ.first_occupied(c[0], c[1], c[2]) is not None


def assert_sound(occ, s, h):
    """The box at 8 evenly spaced fractions of [0, t], shrunk by 1e-3 per side, overlaps no occupied voxel; nor does the returned box."""
    if h["kind"] not in (sr.FREE, sr.BLOCKED):
        return
    lo, hi, m = (s[k].astype(np.float64) for k in range(3))
    for frac in np.linspace(0.0, float(h["t"]), 8):
        assert not _overlaps_any(occ, lo + m * frac + EPS, hi + m * frac - EPS), (s, h, frac)
    assert not _overlaps_any(occ, np.float64(h["lo"]) + EPS, np.float64(h["hi"]) - EPS), (s, h)


def texel_world(occ, texel):
    lr = np.asarray(occ.lr)
    return lr - occ.R // 2 + (np.asarray(texel) - lr) % occ.R


def assert_tight(occ, s, h):
    """BLOCKED: the box grown by 1e-3 overlaps the reported texel at some time among t + k * delta / 8, k = 1..8, with
    delta = 2e-3 / |motion_axis| (a single probe at t + delta is wrong: the box may leave the cell on another axis within delta)."""
    if h["kind"] != sr.BLOCKED:
        return
    lo, hi, m = (s[k].astype(np.float64) for k in range(3))
    v = texel_world(occ, h["texel"]).astype(np.float64)
    assert occ.occupied(tuple(int(c) for c in v))
    delta = 2e-3 / abs(m[h["axis"]])
    for k in range(1, 9):
        tk = float(h["t"]) + k * delta / 8
        if all(lo[a] + m[a] * tk - EPS < v[a] + 1 and hi[a] + m[a] * tk + EPS > v[a] for a in range(3)):
            return
    raise AssertionError(("not tight", s, h))


def run(occ, sweeps):
    return [sr.sweep(occ, s[0], s[1], s[2]) for s in sweeps]


# ---- (a) closure -------------------------------------------------------------------------------------------------------------------
def _chain(occ, steps, seed, heights):
    rng = np.random.default_rng(seed)
    lr = np.asarray(occ.lr)
    while True:                                            # a start that is not embedded
        ix, iy = rng.integers(40, occ.R - 40, 2)
        lo = np.float32([ix + lr[0] - occ.R // 2 + rng.random(), iy + lr[1] - occ.R // 2 + rng.random(), heights[iy, ix] + rng.uniform(0, 2)])
        hi = lo + PLAYER
        if sr.sweep(occ, lo, hi, (0, 0, 0))["kind"] == sr.FREE:
            break
    motions = random_motions(rng, steps, 2.5)
    kinds = np.zeros(4, int)
    for i in range(steps):
        m = motions[i].copy()
        if m[2] != 0 and i % 3:
            m[2] -= f32(0.8)                               # mostly falling: the walker stays on the ground
        centre = (lo + hi) / 2 - lr
        for a in range(2):                                 # far from the middle of the window: walk back
            if abs(centre[a]) > 90 and m[a] != 0:
                m[a] = -abs(m[a]) * np.sign(centre[a])
        h = sr.sweep(occ, lo, hi, m)
        kinds[h["kind"]] += 1
        assert h["kind"] in (sr.FREE, sr.BLOCKED), (i, lo, hi, m, h)
        lo, hi = np.float32(h["lo"]), np.float32(h["hi"])
    return kinds


def test_chained_sweeps_are_never_embedded(terrain, staircase, blocks):
    """20,000 sweeps in 8 chains, each sweep starting from the box the previous one returned."""
    total = np.zeros(4, int)
    for k, occ in enumerate((terrain, terrain, terrain, terrain, staircase, staircase, blocks, blocks)):
        total += _chain(occ, 2500, 100 + k, surface_heights(occ))
    assert total.sum() == 20000 and total[sr.EMBEDDED] == 0 and total[sr.INVALID] == 0
    assert total[sr.BLOCKED] > 4000 and total[sr.FREE] > 4000


# ---- (b), (c), (e) on the batches the GPU tests run --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def terrain_batch(terrain):
    s = surface_sweeps(terrain, **TERRAIN_BATCH)
    return s, run(terrain, s)


def test_terrain_batch_meets_its_conditions(terrain_batch):
    s, hits = terrain_batch
    n = len(s)
    kinds = np.bincount([h["kind"] for h in hits], minlength=4)
    assert kinds[sr.FREE] >= n // 4 and kinds[sr.BLOCKED] >= n // 4 and kinds[sr.EMBEDDED] >= 50 and kinds[sr.INVALID] == 0
    normals = np.bincount([h["normal"] for h in hits if h["kind"] == sr.BLOCKED], minlength=6)
    assert (normals >= 50).all(), normals
    assert sum(has_aligned_face(x) for x in s) >= n // 10
    assert int((s[:, 2] == 0).any(axis=1).sum()) >= n // 10
    assert np.abs(s).max() <= 1024


def test_terrain_batch_is_sound_and_tight(terrain, terrain_batch):
    s, hits = terrain_batch
    for x, h in zip(s, hits):
        assert_sound(terrain, x, h)
        assert_tight(terrain, x, h)


@pytest.mark.parametrize("name", ["staircase", "blocks"])
def test_scene_batches_are_sound_and_tight(name, staircase, blocks):
    occ = staircase if name == "staircase" else blocks
    s = scene_sweeps(occ, 1024, 7)
    hits = run(occ, s)
    kinds = np.bincount([h["kind"] for h in hits], minlength=4)
    assert kinds[sr.FREE] > 100 and kinds[sr.BLOCKED] > 100 and kinds[sr.EMBEDDED] > 20
    for x, h in zip(s, hits):
        assert_sound(occ, x, h)
        assert_tight(occ, x, h)


# ---- (d) named cases ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def floor(native_built):
    return sr.Occupancy(*world.region_from_ids(scenes.floor_ids(world_z_top=10)), (0, 0, 0), 256)


def _bits(v):
    return np.asarray(v, dtype=np.float32).tobytes()


def test_zero_motion_returns_the_box_bit_for_bit(floor):
    lo, hi = np.float32([3.25, -7.5, 10.0]), np.float32([3.85, -6.9, 11.8])
    h = sr.sweep(floor, lo, hi, (0, 0, 0))
    assert h["kind"] == sr.FREE and h["t"] == 1 and h["axis"] == 3 and h["normal"] == 6 and h["texel"] == (-1, -1, -1) and h["material"] == 0
    assert _bits(h["lo"]) == _bits(lo) and _bits(h["hi"]) == _bits(hi)
    lo[0] = f32(-0.0)                                      # the sign of a zero too
    h = sr.sweep(floor, lo, hi, (0, 0, 0))
    assert _bits(h["lo"]) == _bits(lo)


def test_resting_on_a_floor(floor):
    """A box whose low face lies on the floor's top does not include the cell below: it slides freely, and any motion down is
    blocked at once."""
    lo, hi = np.float32([3.25, -7.5, 10.0]), np.float32([3.85, -6.9, 11.8])
    for m in ((2.5, 0, 0), (-3.0, 1.25, 0), (0, -40.0, 0)):
        h = sr.sweep(floor, lo, hi, m)
        assert h["kind"] == sr.FREE, m
        assert _bits(h["lo"]) == _bits(lo + np.float32(m)) and _bits(h["hi"]) == _bits(hi + np.float32(m))
    for down in (-1e-30, -1e-3, -0.5, -1.0, -64.0):
        for mx in (0.0, 0.75):
            h = sr.sweep(floor, lo, hi, (mx, 0, down))
            assert h["kind"] == sr.BLOCKED and h["t"] == 0 and h["axis"] == 2 and h["normal"] == 4, (down, mx)
            assert h["texel"][2] == 128 + 9 and _bits(h["lo"]) == _bits(lo) and _bits(h["hi"]) == _bits(hi)


def test_motion_that_ends_touching_a_wall_is_free(staircase):
    """The staircase's wall covers world y = 102 .. 111 below z = 72: a box whose high face ends exactly on y = 102 is not blocked; a
    hair further it is, at the wall's face."""
    lo, hi = np.float32([-100.25, 99.0, 40.0]), np.float32([-99.5, 100.5, 41.5])
    assert not staircase.occupied((-100, 101, 40)) and staircase.occupied((-100, 102, 40))
    h = sr.sweep(staircase, lo, hi, (0, 1.5, 0))
    assert h["kind"] == sr.FREE and h["hi"][1] == 102.0
    h = sr.sweep(staircase, lo, hi, (0, 1.75, 0))
    assert h["kind"] == sr.BLOCKED and h["axis"] == 1 and h["normal"] == 3 and h["hi"][1] == 102.0 and h["lo"][1] == 100.5
    assert h["t"] == f32(f32(1.5) / f32(1.75)) and h["texel"] == (27, 230, 168)


def test_the_window_ends_the_world(native_built):
    """A box that leaves the window is free; a wall whose texels the voxels one outside the window wrap onto is air."""
    ids = scenes.empty_ids()
    ids[:, :, 0] = 3                                       # a wall on the window's lowest x: world x = -128 (lr = 0)
    occ = sr.Occupancy(*world.region_from_ids(ids), (0, 0, 0), 256)
    assert occ.occupied((-128, 0, 0)) and not occ.occupied((128, 0, 0)) and not occ.occupied((-129, 0, 0))
    lo, hi = np.float32([126.5, 0.25, 0.25]), np.float32([127.5, 0.75, 1.0])
    h = sr.sweep(occ, lo, hi, (5.0, 0, 0))                 # through x = 128, whose texel column 0 holds the wall
    assert h["kind"] == sr.FREE and h["lo"][0] == 131.5
    h = sr.sweep(occ, np.float32([-126.5, 0.25, 0.25]), np.float32([-125.5, 0.75, 1.0]), (-5.0, 0, 0))
    assert h["kind"] == sr.BLOCKED and h["normal"] == 0 and h["texel"][0] == 0 and h["lo"][0] == -127.0
    occ2 = sr.Occupancy(occ.materials, occ.minefield, (16, 0, 0), 256)      # the same bytes under a scrolled window: the wall is x = 128
    assert occ2.occupied((128, 0, 0)) and not occ2.occupied((-128, 0, 0))
    h = sr.sweep(occ2, lo, hi, (5.0, 0, 0))
    assert h["kind"] == sr.BLOCKED and h["normal"] == 1 and h["hi"][0] == 128.0


def test_six_directions_give_the_ray_query_normals(native_built):
    """A box moved against each face of one voxel reports the normal code a ray travelling the same way reports (the ray-query
    restatement's trace_ray)."""
    mats, mine = world.region_from_ids(scenes.single_voxel_ids((128, 128, 128)))
    occ = sr.Occupancy(mats, mine, (0, 0, 0), 256)
    seen = []
    for a in range(3):
        for sign in (1.0, -1.0):
            centre = np.float32([0.5, 0.5, 0.5])
            centre[a] -= f32(sign * 3.0)
            m = np.zeros(3, np.float32)
            m[a] = sign * 4.0
            h = sr.sweep(occ, centre - f32(0.25), centre + f32(0.25), m)
            ray = rq.trace_ray(mats, mine, centre, m)
            assert ray["kind"] == rq.HIT_SOLID and ray["texel"] == (128, 128, 128)
            assert h["kind"] == sr.BLOCKED and h["axis"] == a and h["texel"] == (128, 128, 128) and h["normal"] == ray["normal"]
            assert h["material"] == ray["material"] and h["t"] == f32(f32(2.25) / f32(4.0))
            seen.append(h["normal"])
    assert sorted(seen) == [0, 1, 2, 3, 4, 5]


def test_out_of_domain_records_are_invalid(floor):
    ok = np.float32([[0, 0, 20], [1, 1, 21], [1, 0, 0]])
    assert sr.sweep(floor, *ok)["kind"] == sr.FREE
    for k, (i, j, v) in enumerate(((0, 0, np.nan), (2, 1, np.inf), (1, 2, 20.0), (1, 0, 9.0), (2, 2, -65.0), (0, 1, 2.0 ** 23))):
        bad = ok.copy()
        bad[i, j] = v
        if k == 5:
            bad[1, j] = f32(v + 1)
        h = sr.sweep(floor, *bad)
        assert h["kind"] == sr.INVALID and h["t"] == 0 and h["texel"] == (-1, -1, -1), k
        assert _bits(h["lo"]) == _bits(bad[0]) and _bits(h["hi"]) == _bits(bad[1])


def test_move_and_slide_walks_down_the_staircase(staircase):
    """The character-controller loop: a walker pushed along -x with gravity lands on each step in turn and never sinks into one."""
    lo = np.float32([-3.7, 10.2, 0.0])
    lo[2] = surface_heights(staircase)[138, 124] + 0.5
    hi = lo + PLAYER
    floors = set()
    for _ in range(40):
        lo, hi, hits = sr.move_and_slide(staircase, lo, hi, (-0.9, 0.1, -1.3))
        assert 1 <= len(hits) <= 3 and all(h["kind"] in (sr.FREE, sr.BLOCKED) for h in hits)
        assert sr.sweep(staircase, lo, hi, (0, 0, 0))["kind"] == sr.FREE
        if hits[0]["kind"] == sr.BLOCKED and hits[0]["axis"] == 2:
            floors.add(float(lo[2]))
    assert len(floors) >= 4
