"""The kernels of the hash-grid radiance cache: register, scratch and LDS budget, read from the code-object metadata
of the built objects -- tests/kernel_metadata.py reads it, no GPU needed. pt_rcache.hip.o holds these nine kernels and no other. All are
held to no scratch, no LDS (the resolve keeps its bucket in the registers of half a wave and compacts by ballot, so it stages nothing) and
at most 64 VGPRs: the table kernels hide the latency of dependent atomics and gathers with resident waves, and 64 VGPRs is the full eight
waves per SIMD they were designed for. The surface query sits next to pt_trace_rays_kernel in pt_megakernel.hip.o and shares its budget:
the private traversal stack is its only scratch, and it stays within 128 VGPRs (four waves per SIMD)."""
import pytest

from kernel_metadata import kernels as _kernels

KERNELS = ["rcache_insert<true>", "rcache_insert<false>", "rcache_resolve", "rcache_query", "rcache_clear", "rcache_update_rays", "rcache_gather_samples",
           "rcache_serve", "rcache_apply"]


@pytest.fixture(scope="module")
def rcache():
    return _kernels("pt_rcache.hip.o")


def test_the_object_holds_these_kernels_only(rcache):
    assert sorted(rcache) == sorted(KERNELS)


@pytest.mark.parametrize("name", KERNELS)
def test_no_scratch_no_lds_at_eight_waves(rcache, name):
    assert name in rcache, sorted(rcache)
    k = rcache[name]
    print(name, k)
    assert k["scratch"] == 0 and k["lds"] == 0 and k["vgpr"] <= 64, k


@pytest.mark.parametrize("tl", ["true", "false"])
def test_the_surface_query_keeps_the_budget_of_the_ray_query(tl):
    mega = _kernels("pt_megakernel.hip.o")
    k, ray = mega[f"pt_surface_rays_kernel<{tl}>"], mega[f"pt_trace_rays_kernel<false, {tl}>"]
    print(k, ray)
    assert k["lds"] == 0 and k["vgpr"] <= 128 and k["scratch"] == ray["scratch"], (k, ray)
