"""The entity queries' rules without a GPU: tests/entity_query_ref.py — the restatement the GPU tests compare the device with — on
answers worked out by hand, and against the two drawing references (tests/draw_boxes_ref.py, tests/draw_stamps_ref.py), which restate
the same slab test and walk independently for the pixels of a frame."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import draw_boxes_ref as boxes_ref
from tests import draw_stamps_ref as stamps_ref
from tests import entity_query_ref as ref
from tests import entity_query_sets as sets
from tests import stamp_edits as se

f32 = np.float32
NONE_RECORD = dict(kind=ref.NONE, index=0xFFFFFFFF, normal=6, material=0, t=0.0, position=(0, 0, 0), cell=(-1, -1, -1), voxel=0xFFFFFFFF)


def box(lo, hi, material=0x1234):
    b = np.zeros(1, dtype=sets.BOX_DTYPE)
    b["lo"], b["hi"], b["material"], b["emission"] = lo, hi, material, 0xFF000000
    return b


def model(stamp, origin, scale=1.0, orient=0):
    m = np.zeros(1, dtype=sets.MODEL_DTYPE)
    m["stamp"], m["origin"], m["scale"], m["orient"], m["emission"] = stamp, origin, scale, orient, 0xFF000000
    return m


def wall(position):
    """The world hit of one ray that met a solid texel at `position`."""
    w = sets.sky(1)
    w["kind"], w["position"] = 1, position
    return w


def ask(o, d, boxes=None, models=None, stamps=None, world=None):
    out = ref.trace([o], [d], sets.sky(1) if world is None else world, boxes, models, stamps)
    assert out.shape == (1,) and out.dtype.itemsize == 48
    return out[0]


def is_none(h):
    return all(np.array_equal(np.asarray(h[k]), np.asarray(v, dtype=h[k].dtype)) for k, v in NONE_RECORD.items())


BOX = box((3, -1, -1), (5, 1, 1))


def test_an_axis_parallel_ray_enters_a_box_where_the_hand_says():
    h = ask((0, 0, 0), (2, 0, 0), BOX)                       # the direction is normalised: t counts world units
    assert (h["kind"], h["index"], h["normal"], h["material"]) == (ref.BOX, 0, 1, 0x1234)
    assert h["t"] == f32(3.0) and h["position"].tolist() == [3.0, 0.0, 0.0]
    assert h["cell"].tolist() == [-1, -1, -1] and h["voxel"] == 0xFFFFFFFF
    h = ask((10, 0.5, 0), (-1, 0, 0), BOX)                   # from the other side: the high face, code 2 * 0
    assert (h["kind"], h["normal"], h["t"]) == (ref.BOX, 0, f32(5.0)) and h["position"].tolist() == [5.0, 0.5, 0.0]
    h = ask((4, 0, 9), (0, 0, -3), BOX)
    assert (h["kind"], h["normal"], h["t"]) == (ref.BOX, 4, f32(8.0))


def test_an_origin_inside_a_box_does_not_hit_it():
    assert is_none(ask((4, 0, 0), (1, 0, 0), BOX))
    assert is_none(ask((4, 0.5, -0.5), (0.3, -0.2, 0.9), BOX))
    assert is_none(ask((6, 0, 0), (1, 0, 0), BOX))           # and a box behind the ray neither


def test_a_grazing_ray_misses():
    # t_in == t_out: the ray meets the box in the edge x = 2 .. 3, y = 0 only
    assert is_none(ask((0, 0, 0), (1, 1, 0), box((2, 0, -1), (3, 2, 1))))
    assert is_none(ask((0, 0, 0), (1, 1, 0), box((2, -5, -1), (3, 2, 1))))                  # (still t_in = t_out = 2 / d_x)
    assert ask((0, 0, 0), (1, 1, 0), box((2, 1, -1), (3, 3, 1)))["kind"] == ref.BOX


@pytest.mark.parametrize("o, d, hits", [
    ((0, 0.5, 0.5), (1, 0, 0), True),        # two zero components, both inside their slabs
    ((0, 1.0, 0.5), (1, 0, 0), False),       # o_y on the slab's face: lo < o < hi is strict
    ((0, 0.5, -1.0), (1, 0, 0), False),
    ((0, 2.0, 0.0), (1, 0, 0), False),
    ((0, -3.0, 0.5), (1, 1, 0), True),       # one zero component, inside
    ((0, -3.0, 1.0), (1, 1, 0), False),      # ... on the face
    ((0, -3.0, 1.5), (1, 1, -0.0), False),   # a negative zero is a zero
    ((4, 0, 0.5), (0, 0, 0), False),         # no axis bounds the ray (0 / 0: d is NaN)
])
def test_zero_direction_components(o, d, hits):
    h = ask(o, d, BOX)
    assert (h["kind"] == ref.BOX) == hits and (hits or is_none(h))


def test_of_two_identical_boxes_the_lower_index_wins():
    two = np.concatenate([BOX, BOX])
    two["material"] = (7, 8)
    h = ask((0, 0, 0), (1, 0, 0), two)
    assert (h["kind"], h["index"], h["material"]) == (ref.BOX, 0, 7)
    far_first = np.concatenate([box((6, -1, -1), (7, 1, 1)), BOX])
    assert ask((0, 0, 0), (1, 0, 0), far_first)["index"] == 1            # the smaller t wins whatever the order


def test_a_box_wins_against_a_solid_voxel_with_its_bounds():
    stamps = {9: (np.full((1, 1, 1), 0x777, dtype=np.uint32), np.full((1, 1, 1), se.SOLID, dtype=np.uint8))}
    m = model(9, (3, -1, -1), 2.0)
    both = ask((0, 0, 0), (1, 0, 0), BOX, m, stamps)
    alone = ask((0, 0, 0), (1, 0, 0), None, m, stamps)
    assert (both["kind"], both["index"], both["material"]) == (ref.BOX, 0, 0x1234)
    assert (alone["kind"], alone["index"], alone["material"], alone["normal"]) == (ref.MODEL, 0, 0x777, 1)
    assert alone["t"] == both["t"] == f32(3.0) and alone["cell"].tolist() == [0, 0, 0] and alone["voxel"] == 0


def test_absent_and_air_cells_are_see_through():
    state = np.array([[[se.ABSENT, se.AIR, se.SOLID]]], dtype=np.uint8)
    mats = np.array([[[0, 5, 6]]], dtype=np.uint32)
    h = ask((0, 0, 0), (1, 0, 0), None, model(3, (3, -0.5, -0.5)), {3: (mats, state)})
    assert (h["kind"], h["material"], h["normal"], h["voxel"]) == (ref.MODEL, 6, 1, 2)
    assert h["t"] == f32(5.0) and h["cell"].tolist() == [2, 0, 0] and h["position"].tolist() == [5.0, 0.0, 0.0]
    h = ask((10, 0, 0), (-1, 0, 0), None, model(3, (3, -0.5, -0.5)), {3: (mats, state)})       # from the solid end: the bounding box's face
    assert (h["kind"], h["t"], h["normal"], h["cell"].tolist()) == (ref.MODEL, f32(4.0), 0, [2, 0, 0])
    empty = np.array([[[se.ABSENT, se.AIR, se.AIR]]], dtype=np.uint8)
    assert is_none(ask((0, 0, 0), (1, 0, 0), None, model(3, (3, -0.5, -0.5)), {3: (mats, empty)}))


@pytest.mark.parametrize("orient", range(48))
def test_every_orientation_names_the_voxel_and_the_cell(orient):
    ex, ey, ez = 3, 4, 5
    state = np.full((ez, ey, ex), se.AIR, dtype=np.uint8)
    state[3, 2, 1] = se.SOLID
    mats = np.arange(ex * ey * ez, dtype=np.uint32).reshape(ez, ey, ex) + 1000
    voxel = 1 + ex * (2 + ey * 3)
    (cz, cy, cx), = np.argwhere(se.oriented(state, orient) == se.SOLID)
    origin, scale = np.array([7.0, -2.0, 1.0]), 0.5
    centre = origin + (np.array([cx, cy, cz]) + 0.5) * scale
    for axis in range(3):                                   # along every axis, towards the cell from outside the bounding box
        o, d = centre.copy(), np.zeros(3)
        o[axis], d[axis] = origin[axis] - 3.0, 1.0
        h = ask(o, d, None, model(4, origin, scale, orient), {4: (mats, state)})
        assert h["kind"] == ref.MODEL and h["voxel"] == voxel and h["material"] == 1000 + voxel
        assert h["cell"].tolist() == [cx, cy, cz] and h["normal"] == 2 * axis + 1
        assert h["t"] == f32(3.0 + [cx, cy, cz][axis] * scale)


def test_the_depth_test_against_the_world():
    o, d = (0, 0, 0), (1, 0, 0)                             # the box is entered at t = 3: depth_f = 96
    assert is_none(ask(o, d, BOX, world=wall((2, 0, 0))))                                        # a nearer world hit hides it
    assert ask(o, d, BOX, world=wall((3.5, 0, 0)))["kind"] == ref.BOX
    assert is_none(ask(o, d, BOX, world=wall((3, 0, 0))))                                        # D == depth_f: the world wins ties
    above = wall((np.nextafter(f32(3.0), f32(4.0)), 0, 0))
    out, info = ref.trace([o], [d], above, BOX, details=True)
    assert out[0]["kind"] == ref.BOX and info["depth_f"][0] == f32(96.0) and f32(96.0) < info["D"][0] < f32(96.001)
    assert is_none(ask(o, d, BOX, world=wall((np.nan, 0, 0))))                                   # a NaN D reports none
    limit = wall((100, 0, 0))
    limit["kind"] = 2
    assert ask(o, d, BOX, world=limit)["kind"] == ref.BOX and is_none(ask(o, d, BOX, world=wall((1, 0, 0))))
    far = box((2048, -1, -1), (2050, 1, 1))
    near = box((2047.5, -1, -1), (2050, 1, 1))
    assert is_none(ask(o, d, far)) and ask(o, d, near)["kind"] == ref.BOX                         # 2048 units away under the sky: 65535 is not < 65535


@pytest.mark.parametrize("o, d", [((np.nan, 0, 0), (1, 0, 0)), ((0, np.nan, 0), (1, 0, 0)), ((0, 0, 0), (np.nan, 0, 0)), ((0, 0, 0), (1, np.nan, 0)),
                                  ((np.inf, 0, 0), (-1, 0, 0)), ((0, 0, 0), (np.inf, 0, 0)), ((0, 0, 0), (1, -np.inf, 0)), ((-np.inf, 0, 0), (1, 0, 0)),
                                  ((0, 0, 0), (1e30, 0, 0)), ((0, 0, 0), (1e-30, 0, 0))])
def test_nan_and_infinite_rays_hit_no_entity(o, d):
    stamps = {9: (np.full((2, 2, 2), 0x777, dtype=np.uint32), np.full((2, 2, 2), se.SOLID, dtype=np.uint8))}
    both = np.concatenate([BOX, box((-9, -9, -9), (9, 9, 9))])
    assert is_none(ask(o, d, both, model(9, (3, -1, -1), 1.0), stamps))


def test_no_entities_and_no_rays():
    assert is_none(ask((0, 0, 0), (1, 0, 0)))
    assert ref.trace(np.zeros((0, 3)), np.zeros((0, 3)), sets.sky(0), BOX).shape == (0,)


# ---- the two independent restatements agree on a frame's pixel rays ---------------------------------------------------------------------
W, H = 40, 24


def frame_rays():
    u = po.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 5)
    d = boxes_ref.directions(u, W, H)
    o = np.repeat(np.array([[u.origin[0], u.origin[1], u.origin[2]]], dtype=f32), W * H, axis=0)
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2)
    return u, o, d.reshape(-1, 3), xy


def test_boxes_agree_with_the_drawing_reference():
    u, o, d, xy = frame_rays()
    boxes = sets.boxes_along(o, d, 70, seed=11, near=10.0, far=200.0)
    t, idx, axis, _ = boxes_ref.winners(u, boxes, W, H)
    share = np.count_nonzero(idx >= 0) / idx.size
    assert 0.05 <= share < 1.0                               # (of the existing reference alone)
    won = ref.winners(o, d, boxes, None, {})
    assert np.array_equal(won["index"].reshape(H, W), idx)
    has = idx >= 0
    assert won["t"].reshape(H, W)[has].tobytes() == t[has].tobytes() and np.array_equal(won["axis"].reshape(H, W)[has], axis[has])
    assert (won["kind"].reshape(H, W)[has] == ref.BOX).all()
    # ... and through the pixel call's door, under the sky: every winner nearer than 2048 is reported
    out = ref.pick(u, xy, W, H, sets.sky(W * H), boxes)
    assert np.array_equal(out["kind"].reshape(H, W) == ref.BOX, has) and np.array_equal(out["index"].reshape(H, W)[has], idx[has])


def test_models_agree_with_the_drawing_reference():
    u, o, d, xy = frame_rays()
    stamps = sets.stamps_by_id()
    models = sets.models_along(o, d, 20, seed=4, stamps=stamps, near=10.0, far=120.0, scales=[0.37, 1.0, 2.5])
    t, idx, axis, material, _ = stamps_ref.winners(u, models, stamps, W, H)
    share = np.count_nonzero(idx >= 0) / idx.size
    assert 0.05 <= share < 1.0
    won = ref.winners(o, d, None, models, stamps)
    assert np.array_equal(won["index"].reshape(H, W), idx)
    has = idx >= 0
    assert won["t"].reshape(H, W)[has].tobytes() == t[has].tobytes() and np.array_equal(won["axis"].reshape(H, W)[has], axis[has])
    assert np.array_equal(won["material"].reshape(H, W)[has], material[has])
    # the voxel and the cell name the same stamp voxel
    flat = won["index"] >= 0
    for i in np.nonzero(flat)[0][::7]:
        m = models[won["index"][i]]
        mats, state = stamps[int(m["stamp"])]
        assert mats.reshape(-1)[won["voxel"][i]] == won["material"][i] and state.reshape(-1)[won["voxel"][i]] == se.SOLID
        cx, cy, cz = won["cell"][i]
        assert se.oriented(mats, int(m["orient"]))[cz, cy, cx] == won["material"][i]
