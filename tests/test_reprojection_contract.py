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


# ---- the sequences of tests/temporal_ref.py: conditions on the inputs of tests/test_gpu_reprojection_edges.py ---------------------
def _moved_frames(name, noise):
    """[(frame number, expected frame, counts among the pixels with a hit)] of a sequence's moved frames.  The classes partition
    the hit pixels: behind the previous camera; in front but off its screen (NaN coordinates count here); on screen on another face;
    the same face further than the plane tolerance; accepted.  `scaled`: accepted from a count above the cap."""
    out = []
    for k, e in enumerate(tr.sequence_expected(name, noise)):
        if e["mode"] != "moved":
            continue
        d = e["diag"]
        hit, front, frame, face, acc = d["hit"], d["in_front"], d["in_frame"], d["same_face"], d["accepted"]
        n = dict(hit=hit.sum(), behind=(hit & ~front).sum(), outside=(hit & front & ~frame).sum(),
                 other_face=(hit & front & frame & ~face).sum(), plane=(face & ~acc).sum(), accepted=acc.sum(),
                 scaled=(acc & (d["prev_count"] > tr.sequences()[name].cap)).sum())
        n = {key: int(v) for key, v in n.items()}
        assert n["behind"] + n["outside"] + n["other_face"] + n["plane"] + n["accepted"] == n["hit"]
        assert np.array_equal(acc, e["accepted"]) and not acc[~hit].any()
        print("%s frame %d: %s" % (name, k, n))
        out.append((k, e, n))
    return out


def _modes(name, noise):
    return [e["mode"] for e in tr.sequence_expected(name, noise)]


def test_the_sequences_are_what_their_table_says(blue_noise, native_built):
    seqs = tr.sequences()
    assert tuple(seqs) == tr.SEQUENCE_NAMES
    for name, q in seqs.items():
        assert [u.seed for u in q.uniforms] == [(tr.SEED0 + k) % tr.NOISE_BYTES for k in range(len(q.uniforms))], name
        assert len(q.uniforms) <= 12
        assert (q.width, q.height) == ((72, 44) if not name.startswith("shape") else tuple(int(v) for v in name[6:].split("x")))
    # the lens cameras leave the shape every other test has: |forward| = 1, |right| = |up| = 0.4, at right angles
    g = lambda v: np.array(v[:], dtype=np.float64)
    plain, rolled, last = (seqs["lens"].uniforms[k] for k in (0, 1, 4))
    assert abs(np.linalg.norm(g(plain.forward)) - 1) < 1e-6 and abs(np.linalg.norm(g(plain.right)) - 0.4) < 1e-6
    assert abs(g(rolled.right) @ g(plain.up)) > 0.04 and abs(g(rolled.right) @ g(rolled.up)) < 1e-6
    assert abs(np.linalg.norm(g(last.forward)) - 0.5) < 1e-6 and abs(np.linalg.norm(g(last.up)) - 0.68) < 1e-6
    assert abs(np.linalg.norm(g(seqs["lens"].uniforms[3].forward)) - 2.0) < 1e-6
    assert not any(seqs["degenerate"].uniforms[1].right[:]) and any(seqs["degenerate"].uniforms[1].up[:])


def test_turn_puts_hits_behind_and_beside_the_previous_camera(blue_noise, native_built):
    frames = _moved_frames("turn", blue_noise)
    assert [k for k, _, _ in frames] == [1, 2, 3, 4, 5, 6]
    assert all(n["accepted"] == 0 for k, _, n in frames if k <= 5)
    assert sum(n["behind"] >= 500 for k, _, n in frames if k <= 5) >= 4
    assert sum(n["outside"] >= 400 for k, _, n in frames if k <= 5) >= 4
    # (every hit behind the previous camera here lands, mirrored, on another face or off the screen: `mirror` is the sequence in
    # which the test of step 3 alone decides)
    assert frames[-1][2]["accepted"] >= 0.7 * frames[-1][2]["hit"]
    assert not any(e["diag"]["mirror_match"].any() for _, e, _ in frames)


def test_mirror_has_hits_that_only_the_in_front_test_rejects(blue_noise, native_built):
    """Hits behind the previous camera whose mirrored projection lies on the screen, on the same face plane, with the same normal:
    without `a > 0` they would be accepted (seen: 2088 of the 2232 hits of frame 1; the threshold is half of that)."""
    frames = _moved_frames("mirror", blue_noise)
    k, e, n = frames[0]
    d = e["diag"]
    assert k == 1 and n["behind"] == n["hit"] > 2000 and n["accepted"] == 0 and (e["counts"] == 1).all()
    assert int(d["mirror_match"].sum()) >= 1000
    assert not (d["mirror_match"] & d["in_front"]).any()
    assert frames[1][2]["accepted"] >= 0.9 * frames[1][2]["hit"]


def test_lens_changes_every_length_and_angle_of_the_basis(blue_noise, native_built):
    frames = _moved_frames("lens", blue_noise)
    assert [k for k, _, _ in frames] == [1, 2, 3, 4, 5]
    for k, _, n in frames:
        if k == 4:
            assert n["outside"] >= 0.9 * n["hit"]
        else:
            assert 0.4 * n["hit"] <= n["accepted"] <= 0.9 * n["hit"]
            assert n["plane"] >= 50


def test_dolly_crosses_faces_one_voxel_apart(blue_noise, native_built):
    frames = _moved_frames("dolly", blue_noise)
    assert _modes("dolly", blue_noise).count("still") == 1 and len(frames) == 5
    for k, _, n in frames:
        assert n["accepted"] >= 0.7 * n["hit"] and n["other_face"] >= 100


def test_cap1_scales_nearly_every_history_it_takes(blue_noise, native_built):
    frames = _moved_frames("cap1", blue_noise)
    assert _modes("cap1", blue_noise) == ["restart"] + ["still"] * 4 + ["moved"] * 2 + ["still", "moved"]
    for k, e, n in frames:
        assert n["accepted"] > 1000 and (e["counts"][e["accepted"]] == 2).all()
        assert n["scaled"] >= 0.8 * n["accepted"]


def test_cap3_scales_from_six_and_stays_at_four(blue_noise, native_built):
    frames = _moved_frames("cap3", blue_noise)
    assert _modes("cap3", blue_noise) == ["restart"] + ["still"] * 5 + ["moved"] * 3
    k, e, n = frames[0]
    assert n["accepted"] >= 500 and n["scaled"] == n["accepted"] and (e["prev_counts"] == 6).all()
    assert (e["counts"][e["accepted"]] == 4).all()
    for k, e, n in frames:
        assert e["counts"].max() == 4 and e["accumulation"] == (k + 1, 4)
    # later frames read counts above the cap (4) beside counts below it (1, 2), never the cap itself: that is cap3_edge
    assert any(0 < n["scaled"] < n["accepted"] for _, _, n in frames[1:])
    assert not any((e["diag"]["prev_count"][e["accepted"]] == 3).any() for _, e, _ in frames)


def test_cap3_edge_reads_counts_equal_to_the_cap(blue_noise, native_built):
    """c == cap is taken unscaled.  Scaling it instead, (p / 3) * 3, is not the identity in fp32: the first moved frame reads c == 3
    at every accepted pixel (seen: 1150, for 317 of which some channel of (p / 3) * 3 differs from p), a later one reads 3 beside
    4, 2 and 1 (seen: 107, 26 inexact).  Thresholds are half of what was seen, in the direction of the check."""
    frames = _moved_frames("cap3_edge", blue_noise)
    assert _modes("cap3_edge", blue_noise) == ["restart", "still", "still"] + ["moved"] * 4
    at_cap, inexact, read = [], [], []
    for k, e, n in frames:
        d = e["diag"]
        c, p = d["prev_count"], d["prev_sum"]
        at = e["accepted"] & (c == 3)
        with np.errstate(all="ignore"):
            differs = ((p / np.float32(3)) * np.float32(3) != p).any(axis=-1)
        at_cap.append(int(at.sum()))
        inexact.append(int((at & differs).sum()))
        read.append(set(np.unique(c[e["accepted"]]).tolist()))
        assert n["scaled"] == int((e["accepted"] & (c == 4)).sum())
        assert (e["counts"][at] == 4).all() and e["counts"].max() == 4
    print("cap3_edge: accepted at the cap %s, of which inexact when scaled %s, counts read %s" % (at_cap, inexact, read))
    assert at_cap[0] == frames[0][2]["accepted"] >= 500 and inexact[0] >= 150
    assert read[-1] == {1, 2, 3, 4} and at_cap[-1] >= 50 and inexact[-1] >= 13


def test_cap_max_never_scales(blue_noise, native_built):
    frames = _moved_frames("cap_max", blue_noise)
    assert len(frames) == 3
    for k, e, n in frames:
        assert n["scaled"] == 0 and n["accepted"] > 1000
    for k, e in enumerate(tr.sequence_expected("cap_max", blue_noise)):
        assert e["counts"].max() == k + 1 and e["accumulation"] == (k + 1, k + 1)


def test_degenerate_divides_zero_by_zero(blue_noise, native_built):
    frames = _moved_frames("degenerate", blue_noise)
    (k1, e1, n1), (k2, e2, n2), (k3, e3, n3) = frames
    assert (k1, k2, k3) == (1, 2, 3)
    assert n1["accepted"] == n1["hit"] > 2000                    # the same origin and the previous camera is a plain one
    assert n2["accepted"] == 0 and n2["outside"] == n2["hit"] > 2000 and (e2["counts"] == 1).all()
    assert n3["accepted"] >= 0.5 * n3["hit"]


@pytest.mark.parametrize("name", ["arbitrary", "pyramid"])
def test_the_other_worlds_take_both_branches_and_scale(blue_noise, native_built, name):
    frames = _moved_frames(name, blue_noise)
    modes = _modes(name, blue_noise)
    per_pose = ["restart", "moved", "moved", "still", "moved", "moved"]
    assert modes == per_pose * (len(modes) // 6) and len(frames) == 4 * (len(modes) // 6)
    for k, _, n in frames:
        assert 0.5 * n["hit"] <= n["accepted"] <= 0.92 * n["hit"]
        if k % 6 >= 4:
            assert n["scaled"] >= 0.5 * n["accepted"]


def test_the_small_shapes_take_both_outcomes(blue_noise, native_built):
    one = tr.sequence_expected("shape 1x1", blue_noise)
    assert [e["mode"] for e in one] == ["restart", "moved", "still", "moved", "moved"]
    assert all(e["planes"]["normal_r8"][0, 0] < 6 for e in one)
    outcomes = [bool(e["accepted"][0, 0]) for e in one if e["mode"] == "moved"]
    assert True in outcomes and False in outcomes
    for name in ("shape 7x3", "shape 9x17", "shape 333x77"):
        for k, _, n in _moved_frames(name, blue_noise):
            assert 0.5 * n["hit"] <= n["accepted"] < n["hit"]
