"""The kernels of the irradiance probe volume: register, scratch and LDS budget, read from the code-object metadata of
the built object -- tests/kernel_metadata.py reads it, no GPU needed. All four are held to the project's standing bar: no
scratch and at most 128 VGPRs (four waves per SIMD). probes_blend stages its rays and passes its tiles through static LDS of at most 34 KiB;
the other three use none."""
import pytest

from kernel_metadata import kernels as _kernels


@pytest.fixture(scope="module")
def probes():
    return _kernels("pt_probes.hip.o")


@pytest.mark.parametrize("name", ["probes_raygen", "probes_blend", "probes_query", "probes_shade_gbuffer"])
def test_no_scratch_at_four_waves(probes, name):
    assert name in probes, sorted(probes)
    k = probes[name]
    print(name, k)
    assert k["scratch"] == 0 and k["vgpr"] <= 128, k


def test_only_the_blend_uses_lds(probes):
    assert 0 < probes["probes_blend"]["lds"] <= 34 * 1024, probes["probes_blend"]
    for name in ("probes_raygen", "probes_query", "probes_shade_gbuffer"):
        assert probes[name]["lds"] == 0, (name, probes[name])
