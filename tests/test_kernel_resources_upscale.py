"""The kernels of hrpt_upscale: register, scratch and LDS budget, read from the code-object metadata of the built
object -- tests/kernel_metadata.py reads it, no GPU needed. upscale_resolve (the default: global gathers) and
upscale_resolve_staged (HRPT_UPSCALE_STAGED=1) are held to the project's standing bar: no scratch and at most 128 VGPRs (four waves per
SIMD); the staged window of render texels is static LDS of at most 16 KiB."""
import pytest

from kernel_metadata import kernels as _kernels


@pytest.fixture(scope="module")
def upscale():
    return _kernels("pt_upscale.hip.o")


def test_upscale_resolve_exists_without_scratch_at_four_waves(upscale):
    assert "upscale_resolve" in upscale, sorted(upscale)
    k = upscale["upscale_resolve"]
    print("upscale_resolve", k)
    assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] == 0, k


def test_upscale_resolve_staged_keeps_its_window_in_static_lds(upscale):
    assert "upscale_resolve_staged" in upscale, sorted(upscale)
    k = upscale["upscale_resolve_staged"]
    print("upscale_resolve_staged", k)
    assert k["scratch"] == 0 and k["vgpr"] <= 128, k
    assert 0 < k["lds"] <= 16 * 1024, k
