"""The binding's numpy record layouts and its pure size check, without a GPU.

Every *_DTYPE of raytrace_amd.render is np.dtype(<the ctypes struct of abi.py>).  The literals below are the field lists the binding
spelled by hand before that; they stay here as the pinned expectation: names, offsets, formats, sub-array shapes and item size."""
import numpy as np
import pytest

from raytrace_amd import render

LAYOUTS = {
    "HIT_DTYPE": (48, [("position", "<f4", 3), ("distance", "<f4"), ("texel", "<i4", 3), ("material", "<u4"), ("normal", "<u4"),
                       ("kind", "<u4"), ("iterations", "<u4"), ("border_fetches", "<u4")]),
    "PROBE_DTYPE": (32, [("position", "<f4", 3), ("normal", "<u4"), ("cell", "<u2", 2), ("reserved", "<u4", 3)]),
    "PROBE_LIGHT_DTYPE": (16, [("light", "<f4", 3), ("sun_samples", "<u4")]),
    "SWEEP_DTYPE": (48, [("lo", "<f4", 3), ("reserved0", "<u4"), ("hi", "<f4", 3), ("reserved1", "<u4"), ("motion", "<f4", 3),
                         ("reserved2", "<u4")]),
    "SWEEP_HIT_DTYPE": (64, [("t", "<f4"), ("kind", "<u4"), ("normal", "<u4"), ("material", "<u4"), ("texel", "<i4", 3), ("axis", "<u4"),
                             ("lo", "<f4", 3), ("reserved0", "<u4"), ("hi", "<f4", 3), ("reserved1", "<u4")]),
    "DRAW_BOX_DTYPE": (32, [("lo", "<f4", 3), ("material", "<u4"), ("hi", "<f4", 3), ("emission", "<u4")]),
    "DRAW_STAMP_DTYPE": (32, [("origin", "<f4", 3), ("scale", "<f4"), ("stamp", "<u4"), ("orient", "u1"), ("reserved0", "u1", 3),
                              ("emission", "<u4"), ("reserved", "<u4")]),
    "ENTITY_HIT_DTYPE": (48, [("position", "<f4", 3), ("t", "<f4"), ("kind", "<u4"), ("index", "<u4"), ("normal", "<u4"),
                              ("material", "<u4"), ("cell", "<i4", 3), ("voxel", "<u4")]),
    "POINT_LIGHT_DTYPE": (32, [("position", "<f4", 3), ("radius", "<f4"), ("color", "<f4", 3), ("reserved", "<u4")]),
    "SHAPE_DTYPE": (32, [("a", "<i4", 3), ("material", "<u4"), ("b", "<i4", 3), ("kind", "u1"), ("where", "u1"), ("solid", "u1"),
                         ("reserved", "u1")]),
    "STAMP_PLACE_DTYPE": (32, [("at", "<i4", 3), ("stamp", "<u4"), ("orient", "u1"), ("where", "u1"), ("reserved0", "u1", 2),
                               ("reserved", "<u4", 3)]),
    # the record Context.edit_voxels spelled inline
    "VOXEL_EDIT_DTYPE": (16, [("x", "<u2"), ("y", "<u2"), ("z", "<u2"), ("solid", "<u2"), ("material", "<u4"), ("reserved", "<u4")]),
}


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_record_layout_is_the_hand_written_one(name):
    itemsize, fields = LAYOUTS[name]
    want, got = np.dtype(fields), getattr(render, name)
    assert got.names == want.names == tuple(f[0] for f in fields)
    assert got.itemsize == want.itemsize == itemsize
    for field in want.names:
        (wt, wo), (gt, go) = want.fields[field][:2], got.fields[field][:2]
        assert go == wo, field
        assert gt.base.str == wt.base.str and gt.shape == wt.shape and gt.itemsize == wt.itemsize, field
    assert got == want
    a = np.arange(3 * itemsize, dtype=np.uint8)
    for field in want.names:                                               # the same bytes read as the same values
        assert np.array_equal(a.view(got)[field], a.view(want)[field]), field


def test_every_record_dtype_of_the_binding_is_pinned():
    assert sorted(n for n in dir(render) if n.endswith("_DTYPE")) == sorted(LAYOUTS)


@pytest.mark.parametrize("itemsize", [16, 32, 48, 64])
def test_record_count(itemsize):
    count = render.record_count
    assert count("boxes", 0, itemsize) == 0 and count("boxes", 0, itemsize, 0) == 0
    assert count("boxes", 5 * itemsize, itemsize) == 5
    for nbytes in (5 * itemsize - 1, 5 * itemsize + 1, 1):
        with pytest.raises(ValueError, match="boxes must hold whole %d-byte records" % itemsize):
            count("boxes", nbytes, itemsize)
    with pytest.raises(ValueError, match="boxes must hold whole %d-byte RtDrawBox records" % itemsize):
        count("boxes", itemsize + 1, itemsize, None, "RtDrawBox")
    assert count("boxes", 7 * itemsize, itemsize, 7) == 7                    # the cap itself is inside
    with pytest.raises(ValueError, match="at most 7 boxes per call"):
        count("boxes", 8 * itemsize, itemsize, 7)
    with pytest.raises(ValueError, match="whole"):                           # a partial record is refused before the cap is asked
        count("boxes", 8 * itemsize + 1, itemsize, 7)
    assert count("rays", (1 << 31) * itemsize, itemsize) == 1 << 31          # plain integers: no 32-bit wrap
