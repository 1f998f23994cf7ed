"""Frames of an RT_FLAG_REPROJECT context, each followed by one denoise; meant to run under `rocprofv3 --kernel-trace --stats`
so that the seven launches of the denoise get per-launch durations (profiles/history_denoise_*, DESIGN.md "History-aware denoise").

    python tools/history_denoise_profile.py WIDTH HEIGHT MODE [FRAMES]

MODE  plain    rt_denoise                                      (camera moves every frame)
      neutral  rt_denoise_history, settle all 0, no weighting  (camera moves: the same arithmetic on the counted kernels)
      preset   rt_denoise_history, HISTORY_DENOISE_PRESET      (camera moves)
      weight   rt_denoise_history, the preset's settle with weight_by_count (camera moves)
      held     rt_denoise_history, HISTORY_DENOISE_PRESET      (camera holds still: after 16 frames every surface pixel is settled
                                                                in the five wide dispatches)
Prints the share of surface pixels with 8 samples or more in the last frame."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from raytrace_amd import abi, render, world

W, H, MODE = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
N = int(sys.argv[4]) if len(sys.argv) > 4 else 40
noise = np.fromfile(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "blue_noise_512.rgba"), dtype=np.uint8)
mats, mine = world.generate_region()
preset = render.HISTORY_DENOISE_PRESET
params = {"neutral": render.denoise_params(True), "preset": render.denoise_params(True, **preset),
          "weight": render.denoise_params(True, True, preset["settle"]), "held": render.denoise_params(True, **preset)}.get(MODE)
cfg = render.make_config(W, H, spp=1, depth=2, flags=abi.RT_FLAG_CACHE_PRIMARY | abi.RT_FLAG_ACCUMULATE | abi.RT_FLAG_REPROJECT)
with render.Context(cfg) as ctx:
    ctx.upload_world(mats, mine)
    ctx.upload_noise(noise)
    for k in range(N):
        step = 0 if MODE == "held" else k
        ctx.draw_frame(render.camera_uniforms((-30.0 + 0.25 * step, -128.0, 100.0), np.pi / 2 + 0.0025 * step, -0.1, 0.3, 5 + k))
        if MODE == "plain":
            ctx.denoise(True)
        else:
            ctx.denoise_history(params)
        ctx.finalize()
    ctx.sync()
    counts, normal = ctx.read_history(), ctx.readback(abi.RT_BUF_NORMAL_R8UI)
surface = normal < 16
print("done", W, H, MODE, N, "surface pixels with >= 8 samples: %.3f" % float((counts[surface] >= 8).mean()))
