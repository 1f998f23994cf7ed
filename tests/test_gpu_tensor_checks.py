"""The eight device-argument checks of the binding (raytrace_amd.render.check_*) on real device tensors: N = 4 records on cuda:0, no
library call.  For every function and every tensor it takes, a misaligned view, a strided view, a host copy and a numpy array are
refused with a ValueError that names the argument; so are a size that is not whole records, a second tensor one byte short or over,
and one record more than the call's limit.  The well-formed arguments give N.

A uint8 view is misaligned by one byte; `rays`, which the queries take as float32[N, 8] only, by one float."""
import pytest
import torch

from raytrace_amd import abi, render

pytestmark = pytest.mark.gpu

N = 4


def _bytes(n):
    return torch.zeros(n, dtype=torch.uint8, device="cuda:0")


def _rays(n=N):
    return torch.empty((n, 8), dtype=torch.float32, device="cuda:0")


# per function: how it is called with a dict of its arguments; `records`: the tensors whose size gives a count, {name: record bytes};
# `per_n`: the tensors that must hold exactly so many bytes per N; `caps`: {what the message counts: (argument, limit)}; the result.
CASES = {
    "check_query_tensors": dict(
        call=lambda t: render.check_query_tensors(t["rays"], t["hits"], 0),
        rays=True, records={}, per_n={"hits": 48}, caps={}, want=N),
    "check_entity_query_tensors": dict(
        call=lambda t: render.check_entity_query_tensors(t["rays"], t["boxes"], t["world_hits"], t["entity_hits"], 0),
        rays=True, records={"boxes": 32}, per_n={"world_hits": 48, "entity_hits": 48},
        caps={"rays": ("rays", abi.MAX_ENTITY_RAYS), "boxes": ("boxes", abi.MAX_DRAW_BOXES)}, want=(N, N)),
    "check_sweep_tensors": dict(
        call=lambda t: render.check_sweep_tensors(t["sweeps"], t["hits"], 0),
        rays=False, records={"sweeps": 48}, per_n={"hits": 64}, caps={}, want=N),
    "check_draw_box_tensors": dict(
        call=lambda t: render.check_draw_box_tensors(t["boxes"], t["face_lights"], 0),
        rays=False, records={"boxes": 32}, per_n={"face_lights": 6 * 16}, caps={"boxes": ("boxes", abi.MAX_DRAW_BOXES)}, want=N),
    "check_shadow_box_tensor": dict(
        call=lambda t: render.check_shadow_box_tensor(t["boxes"], 0),
        rays=False, records={"boxes": 32}, per_n={}, caps={"boxes": ("boxes", abi.MAX_DRAW_BOXES)}, want=N),
    "check_draw_stamp_lights": dict(       # the models are host records: their count is an argument, and nothing is returned
        call=lambda t: render.check_draw_stamp_lights(t["n"], t["face_lights"], 0),
        rays=False, records={}, per_n={"face_lights": 6 * 16}, caps={"models": ("n", abi.MAX_DRAW_STAMPS)}, want=None),
    "check_point_light_tensors": dict(
        call=lambda t: render.check_point_light_tensors(t["lights"], 0),
        rays=False, records={"lights": 32}, per_n={}, caps={"lights": ("lights", abi.MAX_POINT_LIGHTS)}, want=N),
    "check_probe_tensors": dict(
        call=lambda t: render.check_probe_tensors(t["probes"], t["out"], 0),
        rays=False, records={"probes": 32}, per_n={"out": 16}, caps={}, want=N),
}


def _sizes(case):
    return {k: N * v for k, v in list(case["records"].items()) + list(case["per_n"].items())}


def _good(case):
    t = {name: _bytes(nbytes) for name, nbytes in _sizes(case).items()}
    t["n"] = N
    if case["rays"]:
        t["rays"] = _rays()
    return t


def _refused(case, message, **changed):
    with pytest.raises(ValueError, match=message):
        case["call"](dict(_good(case), **changed))


@pytest.mark.parametrize("name", sorted(CASES))
def test_well_formed_arguments_give_the_count(name):
    case = CASES[name]
    assert case["call"](_good(case)) == case["want"]


def test_every_check_of_the_binding_is_covered():
    assert sorted(n for n in dir(render) if n.startswith("check_")) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_what_a_kernel_could_not_read_is_refused_by_argument(name):
    case = CASES[name]
    for arg, nbytes in _sizes(case).items():
        _refused(case, arg + " must be 16-byte aligned", **{arg: _bytes(nbytes + 16)[1:1 + nbytes]})
        _refused(case, arg + " must be contiguous", **{arg: torch.zeros((nbytes, 2), dtype=torch.uint8, device="cuda:0")[:, 0]})
        _refused(case, arg + " must be a tensor on cuda:0", **{arg: torch.zeros(nbytes, dtype=torch.uint8)})
        _refused(case, arg + " must be a torch tensor", **{arg: torch.zeros(nbytes, dtype=torch.uint8).numpy()})
    if case["rays"]:
        _refused(case, "rays must be 16-byte aligned", rays=torch.zeros(N * 8 + 1, dtype=torch.float32, device="cuda:0")[1:].view(N, 8))
        _refused(case, "rays must be contiguous", rays=torch.zeros((N, 16), dtype=torch.float32, device="cuda:0")[:, :8])
        _refused(case, "rays must be a tensor on cuda:0", rays=torch.zeros((N, 8), dtype=torch.float32))
        _refused(case, "rays must be a torch tensor", rays=torch.zeros((N, 8), dtype=torch.float32).numpy())


@pytest.mark.parametrize("name", sorted(CASES))
def test_sizes_and_counts_are_refused_by_argument(name):
    case = CASES[name]
    for arg, itemsize in case["records"].items():
        for nbytes in (N * itemsize - 1, N * itemsize + 1):
            _refused(case, "%s must hold whole %d-byte" % (arg, itemsize), **{arg: _bytes(nbytes)})
    if case["rays"]:
        for bad in (torch.zeros((N, 7), dtype=torch.float32, device="cuda:0"), torch.zeros(N * 8, dtype=torch.float32, device="cuda:0"),
                    torch.zeros((N, 8), dtype=torch.float64, device="cuda:0")):
            _refused(case, "rays must be a contiguous float32 tensor of shape \\[N, 8\\]", rays=bad)
    for arg, per_n in case["per_n"].items():
        for nbytes in (N * per_n - 1, N * per_n + 1):
            _refused(case, arg + " must be a contiguous tensor of", **{arg: _bytes(nbytes)})
    for counted, (arg, cap) in case["caps"].items():
        over = cap + 1 if arg == "n" else _rays(cap + 1) if arg == "rays" else _bytes((cap + 1) * case["records"][arg])
        _refused(case, "at most %d %s per call" % (cap, counted), **{arg: over})
