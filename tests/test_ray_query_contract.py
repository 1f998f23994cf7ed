"""Ray queries (rt_trace_rays, rt_pick_pixels), CPU side: the RtRay / RtRayHit layout of include/rt_abi.h against the ctypes and
numpy mirrors, the restatement of tests/ray_query_ref.py against the oracle's trace_ray, and the pure pick helpers of
raytrace_amd/render.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from raytrace_amd import abi, world
from tests import ray_query_ref as rq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
CTYPES = {"float": 4, "uint32_t": 4, "int32_t": 4}


def _header_struct(name):
    """[(field, byte offset, bytes)] of a typedef struct of the header (scalar and fixed-array members)."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, off = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(\w+)\s+(\w+)(?:\[(\d+)\])?$", decl)
        assert m, decl
        size = CTYPES[m.group(1)] * int(m.group(3) or 1)
        fields.append((m.group(2), off, size))
        off += size
    return fields


@pytest.mark.parametrize("name,size", [("RtRay", 32), ("RtRayHit", 48)])
def test_ray_structs_match_the_header(name, size):
    hdr = _header_struct(name)
    assert hdr[-1][1] + hdr[-1][2] == size
    ct = getattr(abi, name)
    assert C.sizeof(ct) == size
    assert [(n, getattr(ct, n).offset, getattr(ct, n).size) for n, _ in ct._fields_] == hdr
    if name == "RtRayHit":
        from raytrace_amd.render import HIT_DTYPE
        assert HIT_DTYPE.itemsize == size
        assert [(n, HIT_DTYPE.fields[n][1]) for n in HIT_DTYPE.names] == [(n, o) for n, o, _ in hdr]


def test_hit_kinds_match_the_header():
    for n in ("RT_HIT_AIR", "RT_HIT_SOLID", "RT_HIT_LIMIT"):
        assert int(re.search(r"#define %s\s+(\d+)" % n, HEADER).group(1)) == getattr(abi, n)
    assert (rq.HIT_AIR, rq.HIT_SOLID, rq.HIT_LIMIT) == (abi.RT_HIT_AIR, abi.RT_HIT_SOLID, abi.RT_HIT_LIMIT)


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def assert_float_bits(a, b):
    """Bit-equal float32 values; NaNs must coincide (their payload is not part of the contract)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    assert np.array_equal(_bits(a)[~nan], _bits(b)[~nan])


def oracle_kind(h):
    return abi.RT_HIT_LIMIT if h.limit_exit else (abi.RT_HIT_AIR if h.air else abi.RT_HIT_SOLID)


def seeded_rays(rng, n, R=256):
    """Origins in and around the region (some below it, some outside), directions random with axis-aligned, zero-component,
    zero and NaN ones mixed in."""
    h = R / 2
    o = rng.uniform(-h, h, (n, 3)).astype(np.float32)
    o[: n // 8] *= np.float32(1.6)                                     # some outside the region
    o[n // 8: n // 6, 1] = np.float32(-1.3 * R)                        # some below it
    d = rng.normal(size=(n, 3)).astype(np.float32)
    k = n // 10
    d[:k] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, k)] * rng.choice(np.float32([-1, 1]), (k, 1))
    d[k: 2 * k, rng.integers(0, 3)] = 0.0
    if n > 20:
        d[2 * k] = 0.0
        d[2 * k + 1] = np.nan
        o[2 * k + 2: 2 * k + 6] = np.round(o[2 * k + 2: 2 * k + 6]) + np.float32(0.5)
    return o, d


def test_restatement_agrees_with_the_oracle(procedural_region):
    """tests/ray_query_ref.py against pyoracle.trace_ray, every field the oracle reports, on seeded rays; on solid hits the texel it
    reports holds the material word and a minefield 0."""
    mats, mine = procedural_region
    m3, f3 = mats.reshape(256, 256, 256), mine.reshape(256, 256, 256)
    rng = np.random.default_rng(11)
    o, d = seeded_rays(rng, 160)
    solid = 0
    for i in range(len(o)):
        r = rq.trace_ray(m3, f3, o[i], d[i])
        h = po.trace_ray(mats, mine, o[i], d[i])
        assert_float_bits(r["position"], h.position[:])
        assert_float_bits(r["distance"], h.distance)
        assert (r["normal"], r["kind"], r["material"], r["iterations"], r["border_fetches"]) == (
            h.normal, oracle_kind(h), h.packed_material, h.iterations, h.border_fetches), i
        if r["kind"] == abi.RT_HIT_SOLID and min(r["texel"]) >= 0:
            x, y, z = r["texel"]
            assert m3[z, y, x] == r["material"] and f3[z, y, x] == 0
            solid += 1
        else:
            assert r["texel"] == (-1, -1, -1) or r["kind"] == abi.RT_HIT_SOLID
    assert solid > 10


def test_restatement_on_a_scrolled_window():
    lr = (48, 0, 32)
    mats, mine = world.toroidal_region(lr)
    m3, f3 = mats.reshape(256, 256, 256), mine.reshape(256, 256, 256)
    rng = np.random.default_rng(5)
    o, d = seeded_rays(rng, 60)
    o += np.float32(lr)
    for i in range(len(o)):
        r = rq.trace_ray(m3, f3, o[i], d[i], lr)
        h = po.trace_ray(mats, mine, o[i], d[i], lr)
        assert_float_bits(r["position"], h.position[:])
        assert (r["normal"], r["kind"], r["material"], r["iterations"], r["border_fetches"]) == (
            h.normal, oracle_kind(h), h.packed_material, h.iterations, h.border_fetches), i


def test_pick_helpers():
    from raytrace_amd.render import adjacent_texel, row_from_bottom, texel_to_world
    assert tuple(adjacent_texel((10, 20, 30), 0)) == (11, 20, 30)
    assert tuple(adjacent_texel((10, 20, 30), 1)) == (9, 20, 30)
    assert tuple(adjacent_texel((10, 20, 30), 2)) == (10, 21, 30)
    assert tuple(adjacent_texel((10, 20, 30), 3)) == (10, 19, 30)
    assert tuple(adjacent_texel((10, 20, 30), 4)) == (10, 20, 31)
    assert tuple(adjacent_texel((10, 20, 30), 5)) == (10, 20, 29)
    assert tuple(adjacent_texel((255, 0, 0), 0)) == (0, 0, 0)
    assert tuple(adjacent_texel((0, 0, 511), 5, 512)) == (0, 0, 510)
    assert tuple(adjacent_texel((0, 0, 0), 1, 512)) == (511, 0, 0)
    # texel = world + R/2 (mod R), world inside [lr - R/2, lr + R/2)
    rng = np.random.default_rng(3)
    for R in (256, 512, 1024):
        lr = rng.integers(-4096, 4096, (200, 3))
        w = lr - R // 2 + rng.integers(0, R, (200, 3))
        t = (w + R // 2) % R
        assert np.array_equal(texel_to_world(t, lr, R), w)
    assert tuple(texel_to_world((0, 128, 255), (0, 0, 0))) == (-128, 0, 127)
    assert row_from_bottom(0, 40) == 39 and row_from_bottom(39, 40) == 0
    # the face a ray crosses and the neighbour it came from: a ray along +x (normal 1) enters texel t from t - 1
    mats = np.zeros((256, 256, 256), np.uint32)
    mine = np.ones((256, 256, 256), np.uint8)
    mine[128, 128, 140] = 0
    r = rq.trace_ray(mats, mine, (0.5, 0.5, 0.5), (1.0, 0.0, 0.0))
    assert r["kind"] == abi.RT_HIT_SOLID and r["texel"] == (140, 128, 128) and r["normal"] == 1
    assert tuple(adjacent_texel(r["texel"], r["normal"])) == (139, 128, 128)
    assert tuple(texel_to_world(r["texel"])) == (12, 0, 0)
