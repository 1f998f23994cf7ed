"""Build driver: compiles the gfx950 library and the C++ host mirror in-tree.

    python -m raytrace_amd.build            # build what is stale
    python -m raytrace_amd.build --force

Artifacts (git-ignored, shipped to the GPU box by gpurun):
    raytrace_amd/librt_amd.so    HIP kernels + the C ABI of include/rt_abi.h   (hipcc --offload-arch=gfx950)
    raytrace_amd/librt_host.so   C++ host mirror of the reference's render/world/game API (g++)
    raytrace_amd/rt_bench        headless counterpart of src/bin/main.rs
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
API = os.path.join(CSRC, "api")   # the host layer of the C ABI: no device code (bench.py's kernel hash does not cover it)
HOST = os.path.join(HERE, "host")
INC = os.path.join(ROOT, "include")

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXX = os.environ.get("CXX", "g++")

# -ffp-contract=off is part of the arithmetic contract (include/rt_math.h).
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
             "-Wall", "-Wno-unused-function"]
CXX_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra"]

AMD_SRCS = [os.path.join(CSRC, "rt_kernels.hip"), os.path.join(CSRC, "rt_world.hip"), os.path.join(CSRC, "rt_persist.hip"), os.path.join(CSRC, "rt_paths.hip"), os.path.join(CSRC, "rt_frame.hip"), os.path.join(CSRC, "rt_post.hip"),
            os.path.join(CSRC, "rt_edit.hip"), os.path.join(CSRC, "rt_query.hip"), os.path.join(CSRC, "rt_probe.hip"), os.path.join(CSRC, "rt_terrain.hip"),
            os.path.join(CSRC, "rt_temporal.hip"), os.path.join(CSRC, "rt_slab.hip"), os.path.join(CSRC, "rt_sweep.hip"),
            os.path.join(CSRC, "rt_boxes.hip"), os.path.join(CSRC, "rt_lights.hip"), os.path.join(CSRC, "rt_draw_stamps.hip"),
            os.path.join(CSRC, "rt_shadows.hip"), os.path.join(CSRC, "rt_entity_query.hip"), os.path.join(CSRC, "rt_particles.hip"),
            os.path.join(CSRC, "rt_step_particles.hip"), os.path.join(CSRC, "rt_sweep_entities.hip"), os.path.join(CSRC, "rt_emit.hip"),
            os.path.join(CSRC, "rt_deposit.hip"), os.path.join(CSRC, "rt_settle.hip"), os.path.join(CSRC, "rt_detach.hip"),
            os.path.join(CSRC, "rt_nav.hip"), os.path.join(CSRC, "rt_flow.hip"),
            ] + [os.path.join(API, f) for f in ("api_context.hip", "api_frame.hip", "api_world.hip", "api_query.hip", "api_post.hip",
                                                 "api_gather.hip", "api_passes.hip", "api_nav.hip")]
AMD_DEPS = AMD_SRCS + sorted(os.path.join(d, f) for d in (CSRC, API) for f in os.listdir(d) if f.endswith(".hpp")) + [
    os.path.join(INC, "rt_abi.h"), os.path.join(INC, "rt_math.h")]
HOST_SRCS = [os.path.join(HOST, f) for f in ("world.cpp", "chunk_storage.cpp", "terrain_upload.cpp", "render.cpp", "host_capi.cpp")]
HOST_DEPS = HOST_SRCS + [os.path.join(HOST, f) for f in ("world.hpp", "render.hpp", "chunk_storage.hpp", "terrain_upload.hpp")] + [os.path.join(INC, "rt_abi.h")]
BENCH_SRCS = [os.path.join(HOST, f) for f in ("rt_bench.cpp", "bench_modes.cpp")]
BENCH_DEPS = BENCH_SRCS + [os.path.join(HOST, f) for f in ("bench_run.hpp", "bench_scene.hpp", "render.hpp")] + [os.path.join(INC, "rt_abi.h")]

LIB_AMD = os.path.join(HERE, "librt_amd.so")
LIB_HOST = os.path.join(HERE, "librt_host.so")
BENCH = os.path.join(HERE, "rt_bench")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def _run(cmd):
    print("+", " ".join(cmd), file=sys.stderr, flush=True)   # stderr: bench.py's stdout carries one JSON line only
    subprocess.check_call(cmd)


def build(force=False, verbose=True):
    built = []
    if force or _stale(LIB_AMD, AMD_DEPS):
        objs = []
        for src in AMD_SRCS:
            obj = src + ".o"
            _run([HIPCC] + HIP_FLAGS + ["-I", INC, "-c", src, "-o", obj])
            objs.append(obj)
        _run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_AMD] + objs)
        built.append(LIB_AMD)
    if force or _stale(LIB_HOST, HOST_DEPS + [LIB_AMD]):
        _run([CXX] + CXX_FLAGS + ["-shared", "-o", LIB_HOST] + HOST_SRCS +
             ["-L", HERE, "-lrt_amd", "-ldl", "-Wl,-rpath,$ORIGIN"])
        built.append(LIB_HOST)
    if all(os.path.exists(s) for s in BENCH_SRCS) and (force or _stale(BENCH, BENCH_DEPS + [LIB_HOST, LIB_AMD])):
        _run([CXX] + CXX_FLAGS + ["-o", BENCH] + BENCH_SRCS + ["-L", HERE, "-lrt_host", "-lrt_amd", "-lpthread", "-ldl", "-Wl,-rpath,$ORIGIN"])
        built.append(BENCH)
    return built


if __name__ == "__main__":
    build(force="--force" in sys.argv)
