"""The kernels of deferred lighting: register, scratch and LDS budget, read from the code-object metadata of the built
object -- tests/kernel_metadata.py reads it, no GPU needed. Both are held to the project's standing bar: no scratch and at
most 128 VGPRs (four waves per SIMD); neither uses LDS."""
import pytest

from kernel_metadata import kernels as _kernels


@pytest.fixture(scope="module")
def deferred():
    return _kernels("pt_deferred.hip.o")


@pytest.mark.parametrize("name", ["deferred_rays", "deferred_shade"])
def test_no_scratch_no_lds_at_four_waves(deferred, name):
    assert name in deferred, sorted(deferred)
    k = deferred[name]
    print(name, k)
    assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] == 0, k
