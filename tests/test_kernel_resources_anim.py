"""The kernels of the animation stage (hrpt_animate): register, scratch and LDS budget, read from the code-object
metadata of the built object -- tests/kernel_metadata.py reads it, no GPU needed. All four are held to the project's
standing bar, no scratch and at most 128 VGPRs; the sampling kernel's LDS is the staged animation times (4 bytes x
HRPT_ANIM_LDS_MAX_ANIMATIONS) and nothing more, the others have none."""
import pytest

from hobbyrenderer_amd import structs as S
from kernel_metadata import kernels as _kernels


@pytest.fixture(scope="module")
def anim():
    return _kernels("pt_anim.hip.o")


def test_anim_kernels_exist_without_scratch_at_four_waves(anim):
    assert {"anim_sample", "anim_compose", "anim_compose_groups", "anim_emit"} == set(anim), sorted(anim)
    for n, k in sorted(anim.items()):
        print(n, k)
        assert k["scratch"] == 0 and k["vgpr"] <= 128, (n, k)
        assert k["lds"] == (4 * S.ANIM_LDS_MAX_ANIMATIONS if n == "anim_sample" else 0), (n, k)
