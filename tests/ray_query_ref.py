"""Restatement of trace_ray (shaders/glsl/raytrace.comp:82-183) for the ray-query tests, generalised in the region edge R and
returning what RtRayHit holds beyond the shader's HitResult: the texel whose material word was fetched, the kind of exit and the
border fetches.  Scalar numpy float32 with the exact helpers of tests/shader_trace.py (fused multiply-add, mod, length, normalize
as include/rt_math.h pins them).  Test infrastructure; Python loops, meant for a few hundred rays."""
import numpy as np

from tests.shader_trace import fma32, length3, mod32, normalize3

f32 = np.float32
LIMIT = 2048
HIT_AIR, HIT_SOLID, HIT_LIMIT = 0, 1, 2


def _texel(c, R):
    """Unnormalised NEAREST lookup on one axis: the texel, or -1 outside [0, R) or NaN (CLAMP_TO_BORDER)."""
    return int(c) if (c >= 0 and c < R) else -1


def trace_ray(materials, minefield, origin, direction, lr=(0, 0, 0), R=256):
    """materials, minefield: [R, R, R] arrays indexed [z][y][x].  Returns a dict with the fields of RtRayHit."""
    with np.errstate(all="ignore"):
        materials = np.asarray(materials).reshape(R, R, R)
        minefield = np.asarray(minefield).reshape(R, R, R)
        origin = [f32(x) for x in origin]
        d = normalize3([f32(x) for x in direction])                                              # :83
        pos = list(origin)
        lpa = [f32(f32(1.0) / np.abs(x)) for x in d]                                             # :88
        normals = [1 if d[0] > 0 else 0, 3 if d[1] > 0 else 2, 5 if d[2] > 0 else 4]             # :89-93
        muls = [f32(-1.0) if x > 0 else f32(1.0) for x in d]                                     # :94-98
        rot = [f32(x) for x in lr]                                                               # :104
        off = f32(R // 2)                                                                        # :105
        W = f32(R)
        border = 0

        def get_step(p):                                                                         # :78-80
            nonlocal border
            t = [_texel(mod32(f32(c + off), W), R) for c in p]
            if min(t) < 0:
                border += 1
                return 0
            return int(minefield[t[2], t[1], t[0]])

        step = get_step(pos)                                                                     # :106
        step_size = (1 << (step & 31)) // 2                                                      # :107
        normal, kind, texel, material, iterations = 0, None, (-1, -1, -1), 0, 0
        for _ in range(LIMIT):                                                                   # :109-113
            iterations += 1
            ss = f32(step_size)
            lt = [f32(f32(f32(0.0001) + mod32(f32(f32(pos[a] + off) * muls[a]), ss)) * lpa[a]) for a in range(3)]   # :119
            if lt[0] < lt[1]:                                                                    # :120-136
                axis = 0 if lt[0] < lt[2] else 2
            else:
                axis = 1 if lt[1] < lt[2] else 2
            pos = [fma32(d[a], lt[axis], pos[a]) for a in range(3)]
            normal = normals[axis]
            step = get_step(pos)                                                                 # :137
            if any(np.abs(f32(pos[a] - rot[a])) >= R // 2 for a in range(3)):                   # :138-145
                kind = HIT_AIR
                break
            if step <= 0:                                                                        # :146-160
                kind = HIT_SOLID
                uvw = [f32(mod32(f32(f32(c + off) / W), f32(1.0)) * W) for c in pos]
                t3 = tuple(_texel(u, R) for u in uvw)
                if min(t3) >= 0:
                    texel, material = t3, int(materials[t3[2], t3[1], t3[0]])
                break
            step_size = (1 << (step & 31)) // 2                                                  # :161
        if kind is None:
            kind = HIT_LIMIT                                                                     # Q8
        distance = length3([f32(origin[a] - pos[a]) for a in range(3)])                          # :164
        a = normal // 2                                                                          # :166-180
        pos[a] = f32(pos[a] + f32(0.001)) if normal % 2 == 0 else f32(pos[a] - f32(0.001))
        return {"position": pos, "distance": distance, "texel": texel, "material": material, "normal": normal, "kind": kind,
                "iterations": iterations, "border_fetches": border}
