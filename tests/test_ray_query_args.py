"""Context.trace_rays_async's argument checks (raytrace_amd.render.check_query_tensors), CPU side: a host tensor, or a tensor of
the wrong shape, type or size, is refused before its address can reach the kernel."""
import pytest
import torch

from raytrace_amd.render import check_query_tensors


@pytest.mark.parametrize("what", ["host rays", "host hits", "host both", "not tensors"])
def test_host_tensors_are_refused(what):
    rays = torch.zeros((4, 8), dtype=torch.float32)
    hits = torch.zeros((4, 48), dtype=torch.uint8)
    if what == "not tensors":
        rays, hits = rays.numpy(), hits.numpy()
    with pytest.raises(ValueError):
        check_query_tensors(rays, hits, 0)


def test_device_mismatch_shape_and_size_are_refused_without_a_device():
    # every tensor here lives on the host: the device check refuses them first, whatever else is wrong with them
    for rays, hits in ((torch.zeros((4, 7)), torch.zeros((4, 48), dtype=torch.uint8)),
                       (torch.zeros((4, 8), dtype=torch.float64), torch.zeros((4, 48), dtype=torch.uint8)),
                       (torch.zeros((4, 8)), torch.zeros((4, 47), dtype=torch.uint8))):
        with pytest.raises(ValueError, match="cuda:1"):
            check_query_tensors(rays, hits, 1)
