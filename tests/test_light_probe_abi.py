"""The light-probe part of the C ABI (include/rt_abi.h): record layouts, the exported symbols, the version history, and the
rejections that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytrace_amd import _lib, abi, render
from tests.conftest import ROOT

pytestmark = pytest.mark.usefixtures("native_built")


def test_record_layouts():
    assert C.sizeof(abi.RtLightProbe) == 32 and C.sizeof(abi.RtProbeLight) == 16
    assert {n: getattr(abi.RtLightProbe, n).offset for n, _ in abi.RtLightProbe._fields_} == {
        "position": 0, "normal": 12, "cell": 16, "reserved": 20}
    assert {n: getattr(abi.RtProbeLight, n).offset for n, _ in abi.RtProbeLight._fields_} == {"light": 0, "sun_samples": 12}
    assert render.PROBE_DTYPE.itemsize == 32 and render.PROBE_LIGHT_DTYPE.itemsize == 16
    assert {n: render.PROBE_DTYPE.fields[n][1] for n in render.PROBE_DTYPE.names} == {
        "position": 0, "normal": 12, "cell": 16, "reserved": 20}
    assert {n: render.PROBE_LIGHT_DTYPE.fields[n][1] for n in render.PROBE_LIGHT_DTYPE.names} == {"light": 0, "sun_samples": 12}
    assert abi.RT_PROBE_SPHERE == 6


def test_header_declares_the_records_as_the_bindings_have_them():
    text = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    assert int(re.search(r"#define RT_PROBE_SPHERE (\d+)", text).group(1)) == abi.RT_PROBE_SPHERE
    probe = text.split("typedef struct RtLightProbe {")[1].split("} RtLightProbe;")[0]
    assert re.findall(r"^\s*(\w+)\s+(\w+)(?:\[(\d)\])?;", probe, flags=re.M) == [
        ("float", "position", "3"), ("uint32_t", "normal", ""), ("uint16_t", "cell", "2"), ("uint32_t", "reserved", "3")]
    light = text.split("typedef struct RtProbeLight {")[1].split("} RtProbeLight;")[0]
    assert re.findall(r"^\s*(\w+)\s+(\w+)(?:\[(\d)\])?;", light, flags=re.M) == [("float", "light", "3"), ("uint32_t", "sun_samples", "")]


def test_symbols_are_exported_and_named_in_the_history():
    lib = _lib.amd()
    for name in ("rt_probe_light", "rt_probe_light_async"):
        assert hasattr(lib, name), name
        assert name in _lib.ABI_SYMBOLS
    text = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    history = text.split("1.3  round 4:")[1].split("#define RT_ABI_VERSION_MAJOR")[0]
    for needle in ("RtLightProbe", "RtProbeLight", "RT_PROBE_SPHERE", "rt_probe_light", "rt_probe_light_async"):
        assert needle in history, needle
    assert lib.rt_abi_version() == (1 << 16) | 3


def test_null_context_is_rejected():
    lib = _lib.amd()
    u = abi.RtUniforms()
    probes = np.zeros(1, render.PROBE_DTYPE)
    out = np.zeros(1, render.PROBE_LIGHT_DTYPE)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.rt_probe_light(None, C.byref(u), P(probes), 1, 1, 2, P(out)) == abi.RT_ERR_INVALID_ARG
    assert lib.rt_probe_light_async(None, C.byref(u), P(probes), 1, 1, 2, P(out)) == abi.RT_ERR_INVALID_ARG


def test_make_probes_and_workgroup_of():
    p = render.make_probes([(1.0, 2.0, 3.0), (4.0, 5.0, 6.0)], [3, abi.RT_PROBE_SPHERE], [(7, 65535), (0, 1)])
    assert p.dtype == render.PROBE_DTYPE and p.tobytes()[:32] == np.array(
        [1.0, 2.0, 3.0], "<f4").tobytes() + np.array([3], "<u4").tobytes() + np.array([7, 65535], "<u2").tobytes() + bytes(12)
    with pytest.raises(ValueError):
        render.make_probes([(0, 0, 0)], [0], [(65536, 0)])
    with pytest.raises(ValueError):
        render.make_probes([(0, 0, 0)], [0, 1], [(0, 0)])
    from oracle import pyoracle as po
    for v in (0, 1, 15, 16, 127, 128, 129, 1000, 4095):
        assert int(render.workgroup_of(v)) == po.lib().rt_oracle_workgroup_of(v)
