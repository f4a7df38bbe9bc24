"""The kernel of the vertex quantiser (hrpt_quantize_vertices_device / hrpt_update_vertices_device): register and
scratch budget, read from the code-object metadata of the built object -- tests/kernel_metadata.py reads it, no GPU
needed. Held to the project's standing bar: no scratch, no LDS and at most 128 VGPRs."""
import pytest

from kernel_metadata import kernels as _kernels


@pytest.fixture(scope="module")
def deform():
    return _kernels("pt_deform.hip.o")


def test_kernel_exists_without_scratch_or_lds_at_four_waves(deform):
    assert "quantise_vertices" in deform, sorted(deform)
    k = deform["quantise_vertices"]
    print("quantise_vertices", k)
    assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] == 0, k
