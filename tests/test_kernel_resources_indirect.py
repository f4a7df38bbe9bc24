"""The kernels of traced indirect lighting: register, scratch and LDS budget, read from the code-object metadata of the
built object -- tests/kernel_metadata.py reads it, no GPU needed. All three are held to the project's standing bar: no scratch and at most
128 VGPRs (four waves per SIMD); none uses LDS."""
import pytest

from kernel_metadata import kernels as _kernels


@pytest.fixture(scope="module")
def indirect():
    return _kernels("pt_indirect.hip.o")


@pytest.mark.parametrize("name", ["indirect_rays", "indirect_resolve", "indirect_compose"])
def test_no_scratch_no_lds_at_four_waves(indirect, name):
    assert name in indirect, sorted(indirect)
    k = indirect[name]
    print(name, k)
    assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] == 0, k


def test_the_object_holds_these_three_kernels_only(indirect):
    assert sorted(indirect) == ["indirect_compose", "indirect_rays", "indirect_resolve"]
