"""The kernels of hrpt_trace_radiance: register, scratch and LDS budget, read from the code-object metadata of the
built objects -- tests/kernel_metadata.py reads it, no GPU needed.

The two streaming kernels around the pipeline use no scratch, no LDS and at most 128 VGPRs (the project's standing bar); pt_radiance_kernel,
the one-thread-per-ray path, runs pt_megakernel's bounce loop and may take no more registers or scratch than that kernel in the same object."""
import pytest

from kernel_metadata import kernels as _kernels


@pytest.fixture(scope="module")
def wavefront():
    return _kernels("pt_wavefront.hip.o")


@pytest.fixture(scope="module")
def megakernel():
    return _kernels("pt_megakernel.hip.o")


@pytest.mark.parametrize("name", ["wf_raygen_rays", "wf_store_radiance"])
def test_streaming_kernels_without_scratch_or_lds(wavefront, name):
    assert name in wavefront, sorted(wavefront)[:8]
    k = wavefront[name]
    print(name, k)
    assert k["scratch"] == 0 and k["lds"] == 0 and k["vgpr"] <= 128, (name, k)


@pytest.mark.parametrize("tl", ["true", "false"])
def test_pt_radiance_kernel_within_the_megakernel(megakernel, tl):
    r, m = megakernel[f"pt_radiance_kernel<{tl}>"], megakernel[f"pt_megakernel<{tl}>"]
    print(tl, r, m)
    assert r["vgpr"] <= m["vgpr"] and r["scratch"] <= m["scratch"] and r["lds"] == 0, (tl, r, m)
