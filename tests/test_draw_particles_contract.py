"""The restatement of rt_draw_particles (tests/draw_particles_ref.py) without a GPU: its validity rule over the shared record table,
its expansion to rt_draw_boxes' records, and that drawing through it is drawing the derived boxes — on synthetic planes, with the
properties the GPU test's inputs must have."""
import numpy as np

from oracle import pyoracle as po
from raytrace_amd import abi, render
from tests import draw_boxes_ref
from tests import draw_particles_ref as ref
from tests import draw_particles_sets as sets

f32 = np.float32
TWO22 = f32(4194304.0)


def _u():
    u = po.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, -0.2, 0.3, 5, (0, 0, 0))
    for k in range(3):
        u.forward[k], u.right[k], u.up[k] = (0.0, 1.0, 0.0)[k], (0.4, 0.0, 0.0)[k], (0.0, 0.0, 0.4)[k]
    return u


def _sky(width, height, depth=65535.0):
    return {"depth_f32": np.full((height, width), depth, dtype=f32), "depth_r16": np.full((height, width), 65535, dtype=np.uint16),
            "normal_r8": np.zeros((height, width), dtype=np.uint8), "albedo_rgba8": np.zeros((height, width, 4), dtype=np.uint8),
            "emission_rgba8": np.zeros((height, width, 4), dtype=np.uint8), "lighting_f32": np.zeros((height, width, 4), dtype=f32),
            "lighting_rgba16": np.zeros((height, width, 4), dtype=np.uint16)}


def test_the_validity_rule_over_the_record_table():
    table, expected, names = sets.record_table()
    got = ref.valid(table, sets.TABLE_LIGHTS)
    assert got.tolist() == expected.tolist(), [n for n, g, w in zip(names, got, expected) if g != w]
    by_name = dict(zip(names, got))
    assert not by_name["half 0.1 vanishes at 2^22"] and not by_name["light == nlights"] and not by_name["NaN centre x"]
    assert not by_name["reserved != 0"] and by_name["last light"]
    # one more light, and the record that named it becomes valid; none at all, and no record is
    assert ref.valid(table, sets.TABLE_LIGHTS + 1)[names.index("light == nlights")]
    assert not ref.valid(table, 0).any()


def test_the_derived_box_is_one_rounding_per_corner():
    p = render.make_particles([(TWO22, 1.0e6, 0.1), (3.0e6, 0.0, -TWO22)], [0.25, 0.0625], 0)
    lo, hi = ref.derived(p)
    assert lo.dtype == f32 and hi.dtype == f32
    assert lo[0].tolist() == [float(TWO22) - 0.25, 1.0e6 - 0.25, float(f32(0.1) - f32(0.25))]
    assert hi[0].tolist() == [float(TWO22), 1.0e6 + 0.25, float(f32(0.1) + f32(0.25))]     # 2^22 + 1/4 rounds to even
    assert lo[1][0] == hi[1][0] == f32(3.0e6)                                               # the half vanished
    assert ref.valid(p, 1).tolist() == [True, False]


def test_expansion_gives_each_box_its_particles_light_on_six_faces_and_blanks_invalid_records():
    table, expected, _ = sets.record_table()
    lights = sets.some_lights(sets.TABLE_LIGHTS)
    boxes, face = ref.expand(table, lights)
    assert boxes.dtype == render.DRAW_BOX_DTYPE and face.dtype == render.PROBE_LIGHT_DTYPE
    assert boxes.size == table.size and face.size == 6 * table.size
    assert draw_boxes_ref.valid(boxes).tolist() == expected.tolist()
    lo, hi = ref.derived(table)
    for i in np.flatnonzero(expected):
        assert boxes["lo"][i].tolist() == lo[i].tolist() and boxes["hi"][i].tolist() == hi[i].tolist()
        assert (boxes["material"][i], boxes["emission"][i]) == (table["material"][i], table["emission"][i])
        assert all(face[6 * i + n] == lights[table["light"][i]] for n in range(6))
    empty_boxes, empty_face = ref.expand(table[:0], lights)
    assert empty_boxes.size == 0 and empty_face.size == 0


def test_drawing_is_drawing_the_derived_boxes_and_the_lowest_index_wins_a_tie():
    W, H = 72, 40
    u = _u()
    o = np.array(u.origin[:])
    p = render.make_particles([o + (0, 30, 0), o + (0, 30, 0), o + (4, 50, 2), (np.nan, 0, 0), o + (0, -30, 0)], [1.0, 1.0, 0.5, 1.0, 1.0],
                              [0x1FFFFF, 0x00007F, 0x003F80, 1, 2], [0, 1, 2, 0, 0])
    lights = sets.some_lights(3)
    before = _sky(W, H)
    got = ref.draw_particles(before, u, p, lights, W, H)
    boxes, face = ref.expand(p, lights)
    want = draw_boxes_ref.draw_boxes(before, u, boxes, face, W, H)
    for name in want:
        assert got[name].tobytes() == want[name].tobytes(), name
    _, idx, _, _ = draw_boxes_ref.winners(u, boxes, W, H)
    assert set(np.unique(idx).tolist()) == {-1, 0, 2}                       # the duplicate, the NaN and the cube behind never win
    centre = got["albedo_rgba8"][H // 2, W // 2]
    assert centre.tolist() == [255, 255, 255, 255]                          # particle 0's material, not particle 1's
    drawn = got["depth_f32"] != before["depth_f32"]
    assert drawn[idx == 0].all() and got["lighting_f32"][H // 2, W // 2, :3].tolist() == (lights["light"][0] / f32(16.0)).tolist()
    # behind a wall nothing is drawn
    wall = _sky(W, H, depth=32.0 * 10.0)
    behind = ref.draw_particles(wall, u, p, lights, W, H)
    assert all(behind[name].tobytes() == wall[name].tobytes() for name in wall)


def test_the_adversarial_set_has_the_properties_the_gpu_test_relies_on():
    W, H = 72, 40
    u = _u()
    p, nlights, notes = sets.adversarial(u, W, H)
    ok = ref.valid(p, nlights)
    assert not ok[notes["invalid"]].any() and np.count_nonzero(~ok) == len(notes["invalid"])
    gaps = np.diff(sorted(notes["invalid"]))
    assert (gaps > 1).all()                                                # valid records between the invalid ones
    boxes, _ = ref.expand(p, sets.some_lights(nlights))
    t_in, idx, _, _ = draw_boxes_ref.winners(u, boxes, W, H)
    won = set(np.unique(idx[idx >= 0]).tolist())
    assert {notes["behind"], notes["inside"], notes["on_face"], notes["at_2^22"][2]}.isdisjoint(won)
    assert notes["duplicates"][0] in won and notes["duplicates"][1] not in won and notes["duplicates"][2] not in won
    # the sweep runs from cubes under a pixel to one that covers the frame
    covered = [np.count_nonzero(draw_boxes_ref.winners(u, boxes[i:i + 1], W, H)[1] >= 0) for i in notes["sweep"]]
    assert min(covered) <= 1 and max(covered) == W * H and len({c for c in covered}) >= 8
    tiles = [len({(y // 8, x // 8) for y, x in np.argwhere(draw_boxes_ref.winners(u, boxes[i:i + 1], W, H)[1] >= 0)}) for i in notes["sweep"]]
    assert any(1 < t <= 16 for t in tiles) and any(16 < t < 45 for t in tiles) and 45 in tiles      # both sides of the wide threshold
    # the boundary cubes start exactly at a tile's first column and row or end just before it
    for i in notes["boundary"]:
        ys, xs = np.nonzero(draw_boxes_ref.winners(u, boxes[i:i + 1], W, H)[1] >= 0)
        assert xs.size and (xs.min() % 8 in (0, 1) or xs.max() % 8 in (7, 0))
