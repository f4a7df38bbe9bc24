"""The kernel of hrpt_temporal_accumulate: register and scratch budget, read from the code-object metadata of the
built object -- tests/kernel_metadata.py reads it, no GPU needed. temporal_accumulate is held to the project's standing
bar: no scratch and at most 128 VGPRs (four waves per SIMD); it uses no LDS."""
import pytest

from kernel_metadata import kernels as _kernels


@pytest.fixture(scope="module")
def temporal():
    return _kernels("pt_temporal.hip.o")


def test_temporal_accumulate_exists_without_scratch_at_four_waves(temporal):
    assert "temporal_accumulate" in temporal, sorted(temporal)
    k = temporal["temporal_accumulate"]
    print("temporal_accumulate", k)
    assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] == 0, k
