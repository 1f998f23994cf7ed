"""The rules of rt_add_lights_occluded on the CPU: tests/light_shadow_ref.py (the restatement the GPU tests compare with bit for bit)
held against hand answers on hand-made planes over a tiny hand-made world — the floor, the camera and the light of
test_point_light_contract.py, with boxes and small models between, beyond and around the light."""
import numpy as np

from raytrace_amd import render
from tests import draw_stamps_ref as stamps_ref
from tests import light_shadow_ref as ref
from tests import point_light_ref
from tests import stamp_edits as se
from tests.test_point_light_contract import CAM_Z, H, W, _segment_meets_box, down_camera, floor_planes, floor_world, light, points, same

f32 = np.float32
POS = np.array([0.5, 0.5, 4.0])


def box(lo, hi):
    b = np.zeros(1, dtype=render.DRAW_BOX_DTYPE)
    b["lo"], b["hi"] = np.asarray(lo, dtype=f32), np.asarray(hi, dtype=f32)
    b["material"], b["emission"] = 0x1FFFFF, 0xFF000000
    return b


def seen_with(planes, u, L, boxes=None, models=None, stamps=None, mine=None):
    return ref.weights(planes, u, L, boxes, models, stamps, floor_world() if mine is None else mine, W, H)[1][0]


def stamp(state):
    """(materials, state) of a stamp from its state[ez, ey, ex]."""
    state = np.asarray(state, dtype=np.uint8)
    return np.where(state == se.SOLID, 7, 0).astype(np.uint32), state


def test_zero_occluders_is_add_lights_byte_for_byte():
    u = down_camera()
    planes, mine = floor_planes(u), floor_world([(2, 0, 1), (0, 0, 5)])
    L = np.concatenate([light(POS, radius=12.0), light((-2.5, 1.5, 2.0), radius=5.0, color=(0.3, 7.0, 11.0))])
    want = point_light_ref.add_lights(planes, u, L, mine, W, H)
    assert not same(want, planes)
    for boxes, models in ((None, None), (np.zeros(0, dtype=render.DRAW_BOX_DTYPE), np.zeros(0, dtype=stamps_ref.MODEL_DTYPE))):
        assert same(ref.add_lights_occluded(planes, u, L, boxes, models, {}, mine, W, H), want)
    assert same(ref.add_lights_occluded(planes, u, L[:0], box((2, 0, 1), (3, 1, 2)), None, {}, mine, W, H), planes)


def test_a_box_between_light_and_floor_darkens_exactly_the_pixels_whose_segment_crosses_it():
    u = down_camera()
    planes = floor_planes(u)
    L = light(POS, radius=12.0)
    lo, hi = (2, 0, 1), (3, 1, 2)
    open_seen = seen_with(planes, u, L)
    seen = seen_with(planes, u, L, box(lo, hi))
    P = points(planes, u).reshape(-1, 3)
    surely = _segment_meets_box(P, POS, lo, hi, -1e-3).reshape(H, W)
    maybe = _segment_meets_box(P, POS, lo, hi, 1e-3).reshape(H, W)
    assert open_seen.all() and 5 < surely.sum() < W * H // 4
    assert not seen[surely].any() and seen[~maybe].all()
    assert (maybe & ~surely).sum() <= 4                              # the undecided rim is a handful of pixels
    # ... which is what the world's own voxel there does to rt_add_lights
    assert np.array_equal(seen, point_light_ref.weights(planes, u, L, floor_world([lo]), W, H)[1][0])
    # only the darkened pixels differ from the unoccluded call, and they keep every bit of the input
    a = point_light_ref.add_lights(planes, u, L, floor_world(), W, H)
    b = ref.add_lights_occluded(planes, u, L, box(lo, hi), None, {}, floor_world(), W, H)
    for name in a:
        assert np.array_equal(b[name][seen], a[name][seen]) and np.array_equal(b[name][~seen], planes[name][~seen]), name


def test_the_same_box_beyond_the_light_changes_nothing():
    u = down_camera()
    planes, mine = floor_planes(u), floor_world()
    L = light(POS, radius=12.0)
    want = point_light_ref.add_lights(planes, u, L, mine, W, H)
    for lo, hi in (((-1, -1, 4.5), (2, 2, 6)), ((0, 0, 4.001), (1, 1, 5)), ((-30, -30, 4.25), (30, 30, 4.5))):
        assert same(ref.add_lights_occluded(planes, u, L, box(lo, hi), None, {}, mine, W, H), want), (lo, hi)
    # the last one, lowered to just under the light, darkens everything
    assert same(ref.add_lights_occluded(planes, u, L, box((-30, -30, 3.5), (30, 30, 3.75)), None, {}, mine, W, H), planes)


def test_a_light_inside_a_box_lights_nothing_outside():
    u = down_camera()
    planes, mine = floor_planes(u), floor_world()
    L = light(POS, radius=12.0)
    assert same(ref.add_lights_occluded(planes, u, L, box((0, 0, 3.5), (1, 1, 4.5)), None, {}, mine, W, H), planes)
    assert same(ref.add_lights_occluded(planes, u, L, box((-40, -40, 0.5), (40, 40, 30)), None, {}, mine, W, H), planes)
    # ... but a box that holds the light AND the surface points blocks them too: every point lies inside it (t_in < 0 < t_out)
    assert same(ref.add_lights_occluded(planes, u, L, box((-40, -40, -1), (40, 40, 30)), None, {}, mine, W, H), planes)


def test_a_surface_point_inside_a_box_is_shaded_by_it():
    u = down_camera()
    planes = floor_planes(u)
    L = light(POS, radius=12.0)
    lo, hi = (-1, -1, -0.5), (1, 1, 0.5)
    seen = seen_with(planes, u, L, box(lo, hi))
    P = points(planes, u)
    inside = (np.abs(P[..., 0]) < 0.999) & (np.abs(P[..., 1]) < 0.999)
    assert 4 <= inside.sum() < 60 and not seen[inside].any()
    surely = _segment_meets_box(P.reshape(-1, 3), POS, lo, hi, -1e-3).reshape(H, W)
    maybe = _segment_meets_box(P.reshape(-1, 3), POS, lo, hi, 1e-3).reshape(H, W)
    assert not seen[surely].any() and seen[~maybe].all() and (inside & ~maybe).sum() == 0


def test_a_segment_with_zero_direction_components():
    u = down_camera()
    planes = floor_planes(u)
    _, P, _, _ = point_light_ref.surface_points(planes, u, W, H)
    y, x = H // 2 + 3, W // 2 + 5
    p = P[y, x]
    L = light((p[0], p[1], 3.0), radius=12.0)                        # straight above the pixel: d = (0, 0, 1)
    v = (L["position"][0].astype(f32) - p).astype(f32)
    assert v[0] == 0 and v[1] == 0 and v[2] > 0
    cases = ((box((p[0] - 0.5, p[1] - 0.5, 1), (p[0] + 0.5, p[1] + 0.5, 2)), False, "over the pixel"),
             (box((p[0], p[1] - 0.5, 1), (p[0] + 0.5, p[1] + 0.5, 2)), True, "lo_x == o_x: the zero axis fails lo < o"),
             (box((p[0] - 0.5, p[1] - 0.5, 1), (p[0] + 0.5, p[1], 2)), True, "hi_y == o_y: the zero axis fails o < hi"),
             (box((p[0] - 0.5, p[1] - 0.5, 3.0), (p[0] + 0.5, p[1] + 0.5, 3.5)), True, "t_in == len is not before the light"),
             (box((p[0] - 0.5, p[1] - 0.5, 2.9), (p[0] + 0.5, p[1] + 0.5, 3.5)), False, "the light sits inside the box"))
    for b, visible, what in cases:
        assert seen_with(planes, u, L, b)[y, x] == visible, what
    # the zero axes are exact: the pixels next to it have d_x != 0 and take the ordinary way to the same verdict
    assert not seen_with(planes, u, L, cases[0][0])[y, x + 1]


def test_a_model_with_a_hole_lets_light_through_the_hole():
    u = down_camera()
    planes = floor_planes(u)
    L = light(POS, radius=12.0)
    state = np.full((1, 3, 3), se.SOLID, dtype=np.uint8)
    state[0, 1, 1] = se.AIR
    stamps = {5: stamp(state)}
    models = stamps_ref.batch([stamps_ref.model(5, (-1.0, -1.0, 1.0), 1.0, 0)])
    seen = seen_with(planes, u, L, None, models, stamps)
    P = points(planes, u).reshape(-1, 3)
    cells = [((i - 1, j - 1, 1), (i, j, 2)) for j in range(3) for i in range(3) if (i, j) != (1, 1)]
    surely = np.zeros(H * W, dtype=bool)
    maybe = np.zeros(H * W, dtype=bool)
    for lo, hi in cells:
        surely |= _segment_meets_box(P, POS, lo, hi, -1e-3)
        maybe |= _segment_meets_box(P, POS, lo, hi, 1e-3)
    surely, maybe = surely.reshape(H, W), maybe.reshape(H, W)
    through = _segment_meets_box(P, POS, (0, 0, 1), (1, 1, 2), -1e-3).reshape(H, W) & ~maybe
    assert through.sum() >= 4 and seen[through].all()                # light through the hole
    assert surely.sum() > 50 and not seen[surely].any() and seen[~maybe].all()
    # the eight solid cells as boxes give the same verdict at every pixel (their planes are the model's, exactly, at scale 1)
    eight = np.concatenate([box(lo, hi) for lo, hi in cells])
    assert np.array_equal(seen, seen_with(planes, u, L, eight))
    # an ABSENT hole is as see-through as an AIR one
    state[0, 1, 1] = se.ABSENT
    assert np.array_equal(seen, seen_with(planes, u, L, None, models, {5: stamp(state)}))


def test_a_solid_cell_behind_the_light_in_the_same_model_does_not_block():
    u = down_camera()
    planes, mine = floor_planes(u), floor_world()
    L = light(POS, radius=12.0)
    column = np.full((3, 1, 1), se.AIR, dtype=np.uint8)
    column[2, 0, 0] = se.SOLID                                       # cells z 2.5..3.5, 3.5..4.5 (the light's), 4.5..5.5 (solid)
    stamps = {9: stamp(column)}
    models = stamps_ref.batch([stamps_ref.model(9, (0.0, 0.0, 2.5), 1.0, 0)])
    want = point_light_ref.add_lights(planes, u, L, mine, W, H)
    assert same(ref.add_lights_occluded(planes, u, L, None, models, stamps, mine, W, H), want)
    # the bounding box is entered all the same (as a box it would block), and the column turned over blocks
    b = box((0, 0, 2.5), (1, 1, 5.5))
    assert not seen_with(planes, u, L, b).all()
    stamps[9] = stamp(column[::-1])
    assert not seen_with(planes, u, L, None, models, stamps).all()


def test_a_one_voxel_model_and_the_equal_box_give_the_same_verdict():
    u = down_camera()
    planes = floor_planes(u)
    L = light(POS, radius=12.0)
    stamps = {3: stamp(np.full((1, 1, 1), se.SOLID, dtype=np.uint8))}
    for origin, scale in (((2.0, 0.0, 1.0), 1.0), ((-1.75, 0.5, 0.25), 0.5), ((0.25, 0.25, -0.125), 0.25)):
        models = stamps_ref.batch([stamps_ref.model(3, origin, scale, 0)])
        hi = tuple(o + scale for o in origin)
        a, b = seen_with(planes, u, L, None, models, stamps), seen_with(planes, u, L, box(origin, hi))
        assert np.array_equal(a, b) and not a.all() and a.any(), (origin, scale)


def test_a_boxs_own_lit_face_is_not_self_shadowed():
    u = down_camera()
    planes = floor_planes(u)
    lo, hi = (-1.0, -1.0, 0.0), (1.0, 1.0, 2.0)
    d = point_light_ref.directions(u, W, H)
    t_top = (f32(CAM_Z - 2.0) / -d[..., 2]).astype(f32)
    at = d * t_top[..., None]
    top = (np.abs(at[..., 0] + 0.25) < 0.999) & (np.abs(at[..., 1] + 0.25) < 0.999)     # the pixels that show the box's +z face
    planes["depth_f32"][top] = (t_top * f32(32.0)).astype(f32)[top]
    L = light((0.5, 0.5, 5.0), radius=14.0)
    seen = seen_with(planes, u, L, box(lo, hi))
    P = points(planes, u)
    assert top.sum() >= 9 and np.abs(P[top][:, 2] - 2.03125).max() < 1e-4
    assert seen[top].all()                                           # the segment leaves the box: t_out <= 0 on the face's axis
    assert not seen[~top].all() and seen[~top].any()                 # ... while the floor round the box lies in its shadow
