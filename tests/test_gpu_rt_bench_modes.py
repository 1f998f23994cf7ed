"""rt_bench's modes that had no test of their own: --rays, --entity-rays, --boxes, --particles, --particles --simulate and --models.
Each runs the built binary once on a 128x96 frame and reads its JSON line (--lights, --shadows, --light-shadows, --edit-shape,
--edit-stamp and the frame loop are tested beside the calls they time)."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "raytrace_amd", "rt_bench")
FRAME = ["--width", "128", "--height", "96"]


def _bench(*args):
    r = subprocess.run([EXE] + FRAME + list(args), cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def _bad(flag, *args):
    r = subprocess.run([EXE] + list(args), cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and flag in r.stderr, (r.returncode, r.stderr[-2000:])


@pytest.mark.parametrize("coherent", [False, True])
def test_rt_bench_rays_runs_and_reports(native_built, coherent):
    j = _bench("--rays", "4096", *(["--rays-coherent"] if coherent else []))
    assert j["rays"] == 4096 and j["coherent"] is coherent
    assert 0 < j["solid_hits"] <= 4096
    assert j["trace_rays_ms"] > 0 and j["pick_ms_idle_median"] > 0 and j["pick_ms_in_flight_median"] > 0 and j["pick_ms_in_flight_max"] > 0


def test_rt_bench_entity_rays_runs_and_reports(native_built):
    # (exit 0 also says that the world hits of rt_trace_entities equal rt_trace_rays': the program compares them itself)
    j = _bench("--entity-rays", "4096", "--coherent", "--boxes", "16", "--models", "16", "--model-scale", "1")
    assert j["entity_rays"] == 4096 and j["coherent"] is True and j["boxes"] == 16 and j["models"] == 16 and j["model_scale"] == 1
    assert j["entities_reported"] <= 4096 and j["reported_under_sky"] <= j["entities_reported"]


def test_rt_bench_boxes_runs_and_reports(native_built):
    j = _bench("--boxes", "64")
    assert j["boxes"] == 64 and j["pixels_drawn"] > 0
    assert j["draw_boxes_device_ms"] > 0 and j["draw_boxes_call_ms"] > 0 and j["probe_light_call_ms"] > 0
    _bad("--boxes", "--boxes", "4097")


def test_rt_bench_particles_draw_what_their_boxes_draw(native_built):
    j = _bench("--particles", "256")
    assert j["particles"] == 256
    assert j["pixels_drawn"] == j["boxes_pixels_drawn"] > 0     # rt_draw_particles' contract: the planes rt_draw_boxes leaves


def test_rt_bench_particles_past_the_boxes_limit_have_no_yardstick(native_built):
    j = _bench("--particles", "5000")
    assert j["particles"] == 5000 and "boxes_pixels_drawn" not in j


def test_rt_bench_simulate_runs_and_reports(native_built):
    j = _bench("--particles", "256", "--simulate", "4")
    assert j["particles"] == 256 and j["simulate"] == 4 and j["sweeps"] == 3
    assert j["alive"] <= 256 and j["first_tick_blocked"] <= 256
    assert j["step_device_ms"] > 0 and j["sweep_boxes_device_ms"] > 0
    _bad("--simulate", "--simulate", "3")


def test_rt_bench_models_draw_inside_their_bounding_boxes(native_built):
    j = _bench("--models", "32", "--model-scale", "1")
    assert j["models"] == 32 and 0 < j["pixels_drawn"] <= j["bounding_box_pixels"]
