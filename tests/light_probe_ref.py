"""Reference for one light probe (rt_probe_light, include/rt_abi.h), composed from what the CPU oracle exports: trace_ray, sun,
sample_sky, diffuse_direction, noise_lookup and the arithmetic contract's mod, plus the albedo decode of raytrace.comp:156-158.  The
loop and the unwind order are those of the oracle's level_light (raytrace.comp:324-349 generalised to `depth` levels), in numpy
float32.  pyoracle.trace_ray is region 256 only; for another region pass `trace`, e.g. restated_trace(), which goes through
tests/ray_query_ref.py (Python loops: a few dozen probes).  tests/test_light_probe_contract.py pins it to the oracle's renderer."""
import types

import numpy as np

from oracle import pyoracle as po

f32 = np.float32
NOISE_SIZE = 512
NOISE_BYTES = 512 * 512 * 4
PROBE_SPHERE = 6


def workgroup_of(p):
    """The noise cell of a frame's pixel coordinate (raytrace.comp:291-294, inverted): the oracle's own owning_workgroup."""
    return int(po.lib().rt_oracle_workgroup_of(int(p)))


def albedo_of(packed):
    """raytrace.comp:156-158."""
    packed = int(packed)
    return [f32(f32(packed >> 14 & 0x7F) / f32(127.0)), f32(f32(packed >> 7 & 0x7F) / f32(127.0)), f32(f32(packed & 0x7F) / f32(127.0))]


def _texel(noise, cx, cy):
    """texture(blue_noise, coord): NEAREST, CLAMP_TO_EDGE; (r, g) as UNORM8 floats."""
    ix = int(min(max(np.floor(cx), 0), NOISE_SIZE - 1))
    iy = int(min(max(np.floor(cy), 0), NOISE_SIZE - 1))
    t = noise[(iy * NOISE_SIZE + ix) * 4: (iy * NOISE_SIZE + ix) * 4 + 2]
    return f32(f32(t[0]) / f32(255.0)), f32(f32(t[1]) / f32(255.0))


def noise_offset(noise, seed, cell):
    """noise_offset of raytrace.comp:298-304 with `cell` in place of gl_WorkGroupID.xy."""
    (bx, by), _, _, _ = po.noise_lookup(noise, seed, 0, 0)      # the base texel of the seed (with the sampler's clamp)
    r, g = _texel(noise, bx, by)
    return (f32(f32(r * f32(255.0)) + f32(int(cell[0]) * 8)), f32(f32(g * f32(255.0)) + f32(int(cell[1]) * 8)))


def noise_value(noise, off, level):
    """raytrace.comp:324 (level 1) and :336 (level 2: + 2 / 512); level j adds (j - 1) * 2 / 512."""
    add = f32(f32(level - 1) * f32(f32(2.0) / f32(NOISE_SIZE)))
    m = po.math("mod", np.array([f32(off[0] + add), f32(off[1] + add)], f32), np.array([NOISE_SIZE, NOISE_SIZE], f32))
    return _texel(noise, m[0], m[1])


def restated_trace(mats, mine, lr, R):
    """trace(pos, direction) for probe_sample / probe_light on a region of edge R: tests/ray_query_ref.trace_ray's answer with the
    fields of the oracle's hit that the probe reads."""
    from tests import ray_query_ref as rq

    def trace(pos, direction):
        h = rq.trace_ray(mats, mine, pos, direction, lr, R)
        return types.SimpleNamespace(air=h["kind"] == rq.HIT_AIR, position=h["position"], normal=h["normal"], packed_material=h["material"])
    return trace


def probe_sample(mats, mine, noise, sun_angle, seed, lr, position, normal, cell, depth, stats=None, trace=None):
    """One sample: (light float32[3], sun1.air).  stats (a dict) receives 'levels', the deepest level the path reached; `trace`
    replaces the oracle's trace_ray (region 256) as trace(pos, direction)."""
    if trace is None:
        trace = lambda pos, direction: po.trace_ray(mats, mine, pos, direction, lr)   # noqa: E731
    sunangle, sunlight = po.sun(sun_angle)
    off = noise_offset(noise, seed % NOISE_BYTES, cell)
    first = [False]
    reached = [0]

    def level_light(pos, nrm, level):
        reached[0] = max(reached[0], level)
        nr, ng = noise_value(noise, off, level)
        light = [f32(0.0), f32(0.0), f32(0.0)]
        d = [f32(sunangle[0] + f32(nr * f32(0.05))), f32(sunangle[1] + f32(ng * f32(0.05))), f32(sunangle[2] + f32(f32(0.0) * f32(0.05)))]
        sun = trace(pos, po.normalize(d))                                                       # trace_sun, :185-187
        if sun.air:
            light = [f32(light[k] + sunlight[k]) for k in range(3)]
            if level == 1:
                first[0] = True
        ddir = po.diffuse_direction(nrm, (nr, ng))
        dif = trace(pos, ddir)
        if dif.air:
            sky = po.sample_sky(ddir, sun_angle, True)
            light = [f32(light[k] + sky[k]) for k in range(3)]
        elif level < depth:
            light2 = level_light([f32(v) for v in dif.position[:]], int(dif.normal), level + 1)
            alb = albedo_of(dif.packed_material)
            light2 = [f32(light2[k] * alb[k]) for k in range(3)]
            light2 = [f32(light2[k] + f32(0.0)) for k in range(3)]                              # + emission, always vec3(0) (:155)
            light = [f32(light[k] + light2[k]) for k in range(3)]
        return light

    l1 = level_light([f32(v) for v in position], int(normal), 1)
    if stats is not None:
        stats["levels"] = reached[0]
    return np.array([f32(f32(0.0) + l1[k]) for k in range(3)], f32), first[0]


def probe_light(mats, mine, noise, sun_angle, seed, lr, position, normal, cell, samples, depth, trace=None):
    """The RtProbeLight of one probe: (light float32[3] = the ordered fp32 sum of the samples / samples, sun_samples)."""
    total = np.zeros(3, f32)
    sun_samples = 0
    with np.errstate(all="ignore"):
        for s in range(samples):
            light, sun = probe_sample(mats, mine, noise, sun_angle, (int(seed) + s) % NOISE_BYTES, lr, position, normal, cell, depth, trace=trace)
            total = (total + light).astype(f32)
            sun_samples += bool(sun)
        return (total / f32(samples)).astype(f32), sun_samples
