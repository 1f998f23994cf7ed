"""Drives every call that changes the resident world, at R = 256, 512 and 1024, so that one rocprofv3 --kernel-trace run shows every
world-changing kernel at every size: rt_upload_world (k_flatten_voxels + k_build_maps; R <= 512 only — the 1024 region is filled on
the device, 5 GiB of host arrays are not worth one row), rt_generate_world (k_terrain_heights, k_terrain_fill, k_build_maps), 36
rt_upload_slice calls (k_flatten_slab + k_build_maps), axis by axis, with slabs read back from the region itself, 50 one-voxel
rt_edit_voxels calls (k_rebuild_chunks + k_rebuild_chunk_maps) and one rt_selftest(RT_SELFTEST_SCENE_MAPS) (k_check_maps).
tools/world_rows.py turns the run's kernel trace into one row per (call, R, axis); it relies on the order of the calls here."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytrace_amd import abi, render, world

noise = np.fromfile(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "blue_noise_512.rgba"), dtype=np.uint8)
for region in (256, 512, 1024):
    cfg = render.make_config(64, 64, spp=1, depth=2, region=region, flags=abi.RT_FLAG_TRUSTED_WORLD | abi.RT_FLAG_TIMING_ALL)
    with render.Context(cfg) as ctx:
        if region <= 512:
            mats, mine = world.generate_region(world.DEFAULT_SEED, region=region)
            for rep in range(3):
                ctx.upload_world(mats, mine)
            del mats, mine
        for rep in range(3):
            ctx.generate_world(world.DEFAULT_SEED)
        ctx.upload_noise(noise)
        n = 0
        for axis in range(3):
            slabs = []
            for off in (0, 64, region - 16):
                origin, extent = [0, 0, 0], [region] * 3
                origin[axis], extent[axis] = off, 16
                slabs.append((off,) + ctx.read_box(origin, extent))
            for rep in range(4):
                for off, m, f in slabs:
                    ctx.upload_slice(axis, off, m, f)
                    n += 1
            del slabs
        rng = np.random.default_rng(region)
        for i in range(50):
            ctx.edit_voxels(rng.integers(0, region, size=(1, 3)), [0x1234 | 1 << 15], [i & 1])
        print("region %d: selftest(maps) = %d" % (region, ctx.selftest(2)))
        ctx.draw_frame(render.camera_uniforms((-30.0, -128.0, 100.0), np.pi / 2, 0.0, 0.0, seed=1))
        ctx.sync()
        tm = ctx.timing()
        print("region %d: %d slabs, 50 edits, %d launches, %.3f ms of kernels in total" % (region, n, tm.other_launches, tm.shade_ms))
