"""RT_FLAG_REPROJECT, the part that needs no GPU: the contract (tests/temporal_ref.py) applied to the oracle's one-sample frames.
What it shows: a still camera folds to the oracle's multi-sample frame; on one plane only pixels that leave the frame lose their
history; an occluder's disocclusions restart and nothing is ever taken across two faces; the 0.25 plane tolerance separates two
populations that are orders of magnitude apart; the path the GPU tests walk exercises both branches; and the feature helps."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import scenes
from tests import temporal_ref as tr

W, H, DEPTH = 104, 56, 2
SUN = 0.3


@pytest.fixture(scope="module")
def terrain(native_built):
    from raytrace_amd import world
    return world.generate_region(world.DEFAULT_SEED)


def _floor_region(wall):
    from raytrace_amd import world
    ids = scenes.floor_ids()
    if wall:
        ids[128:168, 150:153, 100:140] = 3
    return world.region_from_ids(ids)


def _floor_uniforms(k):
    return po.camera_uniforms((-20.0 + 0.5 * k, -60.0, 20.0), np.pi / 2, -0.3, SUN, (tr.SEED0 + k) % (512 * 512 * 4))


def _walk(region, noise, uniforms, cap=tr.DEFAULT_CAP):
    """Yields (k, u, planes, lighting_f32, counts, accepted, history) along a list of uniforms."""
    mats, mine = region
    h = tr.History(W, H, cap)
    for k, u in enumerate(uniforms):
        planes = po.render(mats, mine, noise, u, W, H, 1, DEPTH)[0]
        light, _, counts, acc = h.step(planes, u)
        yield k, u, planes, light, counts, acc, h


def test_a_still_camera_folds_to_the_frame_of_five_samples(terrain, blue_noise):
    us = [tr.path_uniforms(k, step=0) for k in range(5)]
    mats, mine = terrain
    h = tr.History(W, H)
    for u in us:
        light, rgba16, counts, acc = h.step(po.render(mats, mine, blue_noise, u, W, H, 1, DEPTH)[0], u)
    want = po.render(mats, mine, blue_noise, us[0], W, H, 5, DEPTH)[0]
    assert np.array_equal(light, want["lighting_f32"], equal_nan=True)
    assert np.array_equal(rgba16, want["lighting_rgba16"])
    assert (counts == 5).all() and acc.all() and (h.frames, h.samples) == (5, 5)


def test_on_one_plane_only_pixels_that_leave_the_frame_lose_their_history(blue_noise, native_built):
    chain = None
    for k, u, planes, light, counts, acc, h in _walk(_floor_region(False), blue_noise, [_floor_uniforms(k) for k in range(8)]):
        floor = planes["normal_r8"] < 6
        assert floor.sum() > 2000
        if k == 0:
            chain = floor.copy()
            continue
        d = h.diag
        outside = floor & ~(d["in_front"] & d["in_frame"])
        rejected = floor & ~acc
        print("frame %d: floor %d rejected %d outside %d, columns %s" % (k, floor.sum(), rejected.sum(), outside.sum(),
                                                                          sorted(set(np.nonzero(rejected)[1]))))
        assert np.array_equal(rejected, outside)
        assert 0 < rejected.sum() < 0.05 * floor.sum()
        # a pixel whose whole chain of history pixels stayed in view has one sample per frame
        chain = acc & chain[d["qy"], d["qx"]]
        assert chain.sum() > 0.5 * floor.sum()
        assert (counts[chain] == k + 1).all()
        assert (counts[floor & ~chain] <= k).all()


def _hit_coordinate(u, planes, xs, ys, axis):
    """World coordinate along `axis` of the primary hit of pixels (xs, ys), in float64 from the frame's own planes."""
    o, f, r, up = (np.array(v[:], dtype=np.float64) for v in (u.origin, u.forward, u.right, u.up))
    sx, sy = xs / W * 2.0 - 1.0, ys / H * 2.0 - 1.0
    d = f + r * sx[..., None] + up * sy[..., None]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    P = o + d * (planes["depth_f32"][ys, xs].astype(np.float64) / 32.0)[..., None]
    return np.take_along_axis(P, axis[..., None], -1)[..., 0]


def test_an_occluder_restarts_what_it_uncovers_and_nothing_crosses_faces(blue_noise, native_built):
    prev = None
    uncovered_total = wall_total = wall_accepted = 0
    for k, u, planes, light, counts, acc, h in _walk(_floor_region(True), blue_noise, [_floor_uniforms(k) for k in range(8)]):
        nrm = planes["normal_r8"].astype(np.int64)
        if prev is not None:
            pu, pplanes = prev
            d = h.diag
            qx, qy = d["qx"], d["qy"]
            pn = pplanes["normal_r8"].astype(np.int64)[qy, qx]
            on_screen = d["hit"] & d["in_front"] & d["in_frame"]
            # floor the wall covered in the previous frame: restarted
            uncovered = on_screen & (nrm == 4) & (pn != 4)
            uncovered_total += int(uncovered.sum())
            assert (counts[uncovered] == 1).all() and not acc[uncovered].any()
            # accepted pixels, from the two frames' planes alone: same normal, same integer plane along the normal's axis
            ys, xs = np.nonzero(acc)
            axis = nrm[ys, xs] >> 1
            assert (pn[ys, xs] == nrm[ys, xs]).all()
            here = _hit_coordinate(u, planes, xs, ys, axis)
            there = _hit_coordinate(pu, pplanes, qx[ys, xs], qy[ys, xs], axis)
            assert (np.round(here) == np.round(there)).all()
            assert np.abs(here - np.round(here)).max() < 0.01 and np.abs(there - np.round(there)).max() < 0.01
            wall = nrm < 4
            wall_total += int(wall.sum())
            wall_accepted += int(acc[wall].sum())
        prev = (u, planes)
    print("uncovered floor pixels %d, wall pixels accepted %d of %d" % (uncovered_total, wall_accepted, wall_total))
    assert uncovered_total > 0 and wall_total > 1000
    # the wall's faces are planes too: only the one-pixel rim of its silhouette and what enters the frame can lose its history
    assert wall_accepted >= 0.9 * wall_total


def test_the_plane_tolerance_is_not_doing_any_tuning(terrain, blue_noise):
    accepted_max, rejected_min, moved = 0.0, np.inf, 0
    for k, u, planes, light, counts, acc, h in _walk(terrain, blue_noise, [tr.path_uniforms(k, step=s) for k, s in enumerate(tr.GPU_PATH_STEPS)]):
        if h.mode != "moved":
            continue
        moved += 1
        d = h.diag
        diff = d["plane_diff"]
        accepted_max = max(accepted_max, float(diff[acc].max()))
        by_distance = d["same_face"] & ~acc
        if by_distance.any():
            rejected_min = min(rejected_min, float(diff[by_distance].min()))
    print("largest accepted plane difference %.3g, smallest rejected %.3g" % (accepted_max, rejected_min))
    assert moved == 9
    assert accepted_max < 0.01
    assert rejected_min > 0.9


@pytest.mark.parametrize("variant", ["region 256", "region 512 with lr", "below the region"])
def test_the_gpu_path_exercises_both_branches(terrain, blue_noise, variant):
    """A condition on the inputs of tests/test_gpu_reprojection.py, not a measurement: in every moved frame of its paths the
    restatement accepts at least half and rejects at least 5 % of the non-sky pixels, wherever the camera itself moved."""
    from raytrace_amd import world
    region, r, kw = terrain, 256, {}
    if variant == "region 512 with lr":
        region, r = world.generate_region(world.DEFAULT_SEED, region=512), 512
    elif variant == "below the region":
        kw = dict(base=(-30.0, -200.0, 100.0))
    mats, mine = region
    h = tr.History(W, H)
    modes = []
    for k, s in enumerate(tr.GPU_PATH_STEPS):
        lr = (k // 2, -(k // 3), 0) if r == 512 else (0, 0, 0)
        u = tr.path_uniforms(k, step=s, lr=lr, **kw)
        planes = po.render(mats, mine, blue_noise, u, W, H, 1, DEPTH, region=r)[0]
        _, _, counts, acc = h.step(planes, u)
        modes.append(h.mode)
        nonsky = planes["normal_r8"] < 6
        if h.mode == "moved":
            share = acc[nonsky].mean()
            print("%s frame %d: accepted %.3f of %d" % (variant, k, share, nonsky.sum()))
            assert share >= 0.5
            # (a frame of the scrolled region whose pose stands still differs in lr alone: moved, and nothing to reject)
            assert share <= 0.95 or s == tr.GPU_PATH_STEPS[k - 1]
    assert modes.count("still") >= (2 if r == 256 else 0) and modes.count("moved") >= 9 and modes[0] == "restart"


def test_the_feature_helps(terrain, blue_noise):
    """Mean absolute error of the reprojected lighting against the 256-sample frame at the last pose of a 16-frame path (0.05
    voxel and 0.0005 rad per frame), over the error of the last one-sample frame alone: measured 0.52.  Far from 1 / sqrt(count):
    a workgroup's pixels share one noise texel and the nearest-pixel tap carries a half-pixel bias."""
    mats, mine = terrain
    us = [tr.path_uniforms(k, dx=0.05, dh=0.0005) for k in range(16)]
    for k, u, planes, light, counts, acc, h in _walk(terrain, blue_noise, us):
        pass
    ref = po.render(mats, mine, blue_noise, us[-1], W, H, 256, DEPTH)[0]["lighting_f32"][..., :3]
    nonsky = planes["normal_r8"] < 6
    err_reprojected = np.abs(light[..., :3] - ref)[nonsky].mean()
    err_single = np.abs(planes["lighting_f32"][..., :3] - ref)[nonsky].mean()
    print("error reprojected %.5f, single frame %.5f, ratio %.3f, mean count %.2f" % (err_reprojected, err_single,
                                                                                       err_reprojected / err_single, counts[nonsky].mean()))
    assert err_reprojected / err_single <= 0.75
