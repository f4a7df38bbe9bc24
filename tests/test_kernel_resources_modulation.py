"""The kernels of hrpt_demodulate / hrpt_compose: register and scratch budget, read from the code-object metadata of
the built object -- tests/kernel_metadata.py reads it, no GPU needed. Both are held to the project's standing bar: no
scratch and at most 128 VGPRs (four waves per SIMD); neither uses LDS."""
import pytest

from kernel_metadata import kernels as _kernels


@pytest.fixture(scope="module")
def modulation():
    return _kernels("pt_modulation.hip.o")


@pytest.mark.parametrize("name", ["modulation_demodulate", "modulation_compose"])
def test_kernel_exists_without_scratch_or_lds_at_four_waves(modulation, name):
    assert name in modulation, sorted(modulation)
    k = modulation[name]
    print(name, k)
    assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] == 0, k
