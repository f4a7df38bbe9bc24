"""The kernels of resampled direct lighting: register, scratch and LDS budget, read from the code-object metadata of
the built object -- tests/kernel_metadata.py reads it, no GPU needed. The object holds these five kernels and no other; all are held to the
project's standing bar, no scratch and at most 128 VGPRs (four waves per SIMD); only restir_initial<true> uses LDS, and what it uses is the
staged light list, 64 bytes for each of HRPT_RESTIR_LDS_MAX_LIGHTS lights."""
import pytest

from hobbyrenderer_amd import structs as S
from kernel_metadata import kernels as _kernels

KERNELS = ["restir_initial<true>", "restir_initial<false>", "restir_temporal", "restir_spatial", "restir_shade"]


@pytest.fixture(scope="module")
def restir():
    return _kernels("pt_restir.hip.o")


def test_the_object_holds_these_kernels_only(restir):
    assert sorted(restir) == sorted(KERNELS)


@pytest.mark.parametrize("name", KERNELS)
def test_no_scratch_at_four_waves_and_lds_only_for_the_staged_lights(restir, name):
    assert name in restir, sorted(restir)
    k = restir[name]
    print(name, k)
    assert k["scratch"] == 0 and k["vgpr"] <= 128, k
    assert k["lds"] == (64 * S.RESTIR_LDS_MAX_LIGHTS if name == "restir_initial<true>" else 0), k
