"""The kernel of hrpt_denoise: register and scratch budget, read from the code-object metadata of the built object --
tests/kernel_metadata.py reads it, no GPU needed. denoise_poisson is held to the project's standing bar: no scratch and at
most 128 VGPRs (four waves per SIMD); it uses no LDS."""
import pytest

from kernel_metadata import kernels as _kernels


@pytest.fixture(scope="module")
def denoise():
    return _kernels("pt_denoise.hip.o")


def test_denoise_poisson_exists_without_scratch_at_four_waves(denoise):
    assert "denoise_poisson" in denoise, sorted(denoise)
    k = denoise["denoise_poisson"]
    print("denoise_poisson", k)
    assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] == 0, k
