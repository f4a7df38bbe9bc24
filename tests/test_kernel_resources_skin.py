"""The kernel of the vertex producer (hrpt_skin_vertices_device / hrpt_update_vertices_skinned): register, scratch
and LDS budget, read from the code-object metadata of the built object -- tests/kernel_metadata.py reads it, no GPU
needed. Both instantiations are held to the project's standing bar, no scratch and at most 128 VGPRs; the one that gathers its palette
from global memory has no LDS, the staged one has the palette stage (48 bytes x HRPT_SKIN_LDS_MAX_JOINTS) and nothing more. (The kernel
that also quantised was measured no faster than this one followed by the quantiser and is not built: section 22.)"""
import pytest

from hobbyrenderer_amd import structs as S
from kernel_metadata import kernels as _kernels


@pytest.fixture(scope="module")
def skin():
    return _kernels("pt_skin.hip.o")


def test_skin_kernels_exist_without_scratch_at_four_waves(skin):
    names = {f"skin_vertices<{lds}>" for lds in ("true", "false")}
    assert names == set(skin), sorted(skin)
    for n, k in sorted(skin.items()):
        print(n, k)
        assert k["scratch"] == 0 and k["vgpr"] <= 128, (n, k)
        assert k["lds"] == (48 * S.SKIN_LDS_MAX_JOINTS if n.endswith("<true>") else 0), (n, k)
