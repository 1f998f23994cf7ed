"""The contract of rt_shadow_entities on the CPU: tests/entity_shadow_ref.py (the numpy restatement the GPU tests compare with, bit
for bit) held against things it was not written from — a fully solid model against its bounding box as an RtDrawBox, a sparse model
against one box per solid voxel placed between the model's own planes, the world's ray against the CPU oracle's trace_ray — and the
write rule: the strength, the clamp at 0, the night.  The frame is the CPU oracle's."""
import numpy as np
import pytest

from oracle import pyoracle as po
from raytrace_amd import render
from tests import entity_shadow_ref as ref
from tests import stamp_edits as se
from tests.denoise_history_ref import fma

f32 = np.float32
W, H = 64, 40
POSE = dict(origin=(-30.0, -128.0, 100.0), heading=np.pi / 2, pitch=-0.2, sun=0.3)


@pytest.fixture(scope="module")
def frame(procedural_region, blue_noise):
    u = po.camera_uniforms(POSE["origin"], POSE["heading"], POSE["pitch"], POSE["sun"], 5, (0, 0, 0))
    planes, _ = po.render(procedural_region[0], procedural_region[1], blue_noise, u, W, H, 1, 2)
    return u, planes


@pytest.fixture(scope="module")
def points(frame):
    u, planes = frame
    surface, P, _, _ = ref.surface_points(planes, u, W, H)
    return P[surface].astype(f32), ref.sun_of(u)[0]


def _voxel_boxes(m, state):
    """One RtDrawBox per SOLID cell of the placed model, between the model's own planes: [fma(c, scale, origin), fma(c + 1, scale, origin)]."""
    placed = se.oriented(state, int(m["orient"]))
    cz, cy, cx = np.nonzero(placed == se.SOLID)
    c = np.stack([cx, cy, cz], axis=-1).astype(f32)
    b = np.zeros(len(c), dtype=render.DRAW_BOX_DTYPE)
    scale = np.full(c.shape, m["scale"], dtype=f32)
    origin = np.broadcast_to(m["origin"].astype(f32), c.shape)
    b["lo"], b["hi"] = fma(c, scale, origin), fma((c + f32(1.0)).astype(f32), scale, origin)
    return b


@pytest.mark.parametrize("scale", [0.125, 1.0, 3.0])
def test_a_fully_solid_model_shades_what_its_bounding_box_shades(scale, frame, points):
    u, planes = frame
    o, s = points
    solid = (np.ones((5, 4, 3), dtype=np.uint32), np.full((5, 4, 3), se.SOLID, dtype=np.uint8))
    stamps = {7: solid}
    models = ref.scatter_models(planes, u, W, H, 24 if scale >= 1 else 240, 11, 7, (3, 4, 5), scales=(scale,), lift=(-1.0, 4.0))   # small models shade few pixels
    boxes = ref.stamps_ref.bounding_boxes(models, stamps)
    total = 0
    for i in range(len(models)):
        by_model, by_box = ref.models_shade(models[i:i + 1], stamps, o, s), ref.boxes_shade(boxes[i:i + 1], o, s)
        assert np.array_equal(by_model, by_box), "model %d" % i
        total += int(by_box.sum())
    assert total > 20


@pytest.mark.parametrize("scale", [0.125, 1.0, 2.5])
def test_a_sparse_model_is_the_or_of_its_solid_voxels_boxes(scale, frame, points):
    u, planes = frame
    o, s = points
    stamp = ref.small_stamp(seed=3)
    stamps = {9: stamp}
    models = ref.scatter_models(planes, u, W, H, 30 if scale >= 1 else 300, 23, 9, (3, 4, 5), scales=(scale,), lift=(-1.0, 4.0))
    total = inside = 0
    for i in range(len(models)):
        vox = _voxel_boxes(models[i], stamp[1])
        assert len(vox) == int((stamp[1] == se.SOLID).sum())
        by_model, by_boxes = ref.models_shade(models[i:i + 1], stamps, o, s), ref.boxes_shade(vox, o, s)
        assert np.array_equal(by_model, by_boxes), "model %d: %d pixels differ" % (i, int((by_model != by_boxes).sum()))
        total += int(by_model.sum())
        bb = ref.stamps_ref.bounding_boxes(models[i:i + 1], stamps)
        inside += int(((o > bb["lo"][0]) & (o < bb["hi"][0])).all(axis=1).sum())
        assert by_model.sum() <= ref.boxes_shade(bb, o, s).sum()
    assert total > 20
    assert scale < 1.0 or inside > 0                      # some points start inside a bounding box: the other first-cell rule ran


def test_an_all_air_model_shades_nothing(frame, points):
    u, planes = frame
    o, s = points
    stamps = {2: (np.zeros((5, 4, 3), dtype=np.uint32), np.full((5, 4, 3), se.AIR, dtype=np.uint8))}
    models = ref.scatter_models(planes, u, W, H, 16, 5, 2, (3, 4, 5), scales=(2.0,), lift=(-1.0, 3.0))
    assert not ref.models_shade(models, stamps, o, s).any()
    assert ref.boxes_shade(ref.stamps_ref.bounding_boxes(models, stamps), o, s).any()


def test_a_point_inside_a_box_is_shaded_and_a_box_behind_it_is_not(points):
    o, s = points
    p = o[len(o) // 2].astype(np.float64)
    b = np.zeros(3, dtype=render.DRAW_BOX_DTYPE)
    b["lo"][0], b["hi"][0] = p - 0.5, p + 0.5                                    # contains the point
    b["lo"][1], b["hi"][1] = p - 3.0 * s - 0.4, p - 3.0 * s + 0.4                # down the sun's line, behind the point: t_out < 0
    b["lo"][2], b["hi"][2] = p + 3.0 * s - 0.4, p + 3.0 * s + 0.4                # towards the sun
    one = o[len(o) // 2][None]
    assert [bool(ref.boxes_shade(b[i:i + 1], one, s)[0]) for i in range(3)] == [True, False, True]


def test_the_worlds_ray_is_the_oracles_trace_ray(frame, points, procedural_region):
    o, s = points
    kind = ref.trace_kind(procedural_region[1], 256, (0, 0, 0), o, s)
    assert (kind == ref.AIR).sum() > 100 and (kind == ref.SOLID).sum() > 100
    for i in range(0, len(o), 2):
        h = po.trace_ray(procedural_region[0], procedural_region[1], o[i], s)
        want = ref.AIR if h.air else (ref.LIMIT if h.limit_exit else ref.SOLID)
        assert kind[i] == want, "origin %s" % (o[i],)
    # a start inside an occupied texel, and a scrolled window
    inside = o - f32(0.5) * np.array([0, 0, 1], dtype=f32)
    kind_in = ref.trace_kind(procedural_region[1], 256, (16, 0, 0), inside, s)
    for i in range(0, len(o), 7):
        h = po.trace_ray(procedural_region[0], procedural_region[1], inside[i], s, (16, 0, 0))
        assert kind_in[i] == (ref.AIR if h.air else (ref.LIMIT if h.limit_exit else ref.SOLID))


def test_strength_the_clamp_and_the_night(frame, procedural_region):
    u, planes = frame
    mine = procedural_region[1]
    boxes = ref.scatter_boxes(planes, u, W, H, 130, 430)
    classes = ref.masks(planes, u, boxes, None, {}, mine, W, H)
    changed = classes["changed"]
    assert changed.sum() > 10 and classes["world"].sum() > 10 and classes["open"].sum() > 10 and classes["sky"].sum() > 10
    sunlight = ref.sun_of(u)[1]
    for strength in (1.0, 0.5, 0.125):
        got = ref.shadow_entities(planes, u, boxes, None, {}, mine, W, H, strength=strength, classes=classes)
        sub = ((sunlight * f32(strength)).astype(f32) / f32(16.0)).astype(f32)
        L = planes["lighting_f32"][..., :3]
        want = np.maximum((L - sub).astype(f32), f32(0.0))
        assert np.array_equal(got["lighting_f32"][..., :3][changed], want[changed])
        for name in planes:                                                        # every other pixel and plane keeps its bits
            assert got[name][~changed].tobytes() == planes[name][~changed].tobytes(), name
            if name not in ref.WRITTEN:
                assert got[name].tobytes() == planes[name].tobytes(), name
        assert got["lighting_f32"][..., 3].tobytes() == planes["lighting_f32"][..., 3].tobytes()
        assert got["lighting_rgba16"][..., 3].tobytes() == planes["lighting_rgba16"][..., 3].tobytes()
        q, q0 = got["lighting_rgba16"][..., :3][changed], planes["lighting_rgba16"][..., :3][changed]
        assert (got["lighting_f32"][..., :3][changed] <= L[changed]).all() and (q <= q0).all() and (q < q0).sum() > q.size // 2
    # the clamp: lighting below the sun term goes to exactly 0 in both planes
    dim = {k: v.copy() for k, v in planes.items()}
    dim["lighting_f32"][..., :3] = (sunlight / f32(64.0)).astype(f32)
    dim["lighting_rgba16"][..., :3] = 1000
    got = ref.shadow_entities(dim, u, boxes, None, {}, mine, W, H, classes=classes)
    assert (got["lighting_f32"][..., :3][changed] == 0).all() and (got["lighting_rgba16"][..., :3][changed] == 0).all()
    assert got["lighting_f32"][~changed].tobytes() == dim["lighting_f32"][~changed].tobytes()
    # the night: a sun colour of (0, 0, 0) is the identity; so is a call without occluders
    night = ref.shadow_entities(planes, u, boxes, None, {}, mine, W, H, sunlight=(0.0, 0.0, 0.0))
    none = ref.shadow_entities(planes, u, boxes[:0], None, {}, mine, W, H)
    for name in planes:
        assert night[name].tobytes() == planes[name].tobytes() and none[name].tobytes() == planes[name].tobytes()


def test_a_sun_angle_of_zero_gives_a_direction_with_a_zero_component(points):
    """s_y == 0 is representable (sun_angle = 0: sin 0 = 0): the slab test's zero-direction rule is reachable through the ABI."""
    s, color = po.sun(0.0)
    assert s[1] == 0.0 and s[0] != 0.0 and s[2] != 0.0 and (color > 0).all()
    o, _ = points
    p = o[10].astype(np.float64)
    b = np.zeros(2, dtype=render.DRAW_BOX_DTYPE)
    b["lo"][0], b["hi"][0] = p + 2.0 * s - 0.5, p + 2.0 * s + 0.5                # on the sun's line: lo_y < o_y < hi_y
    b["lo"][1], b["hi"][1] = b["lo"][0], b["hi"][0]
    b["lo"][1][1], b["hi"][1][1] = o[10][1], o[10][1] + f32(1.0)                 # its y slab starts AT o_y: lo_y < o_y fails
    one = o[10][None]
    assert [bool(ref.boxes_shade(b[i:i + 1], one, s)[0]) for i in range(2)] == [True, False]
