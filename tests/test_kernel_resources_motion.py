"""The kernels of hrpt_render_motion_vectors: register and scratch budget, read from the code-object metadata of the
built objects -- tests/kernel_metadata.py reads it, no GPU needed.

wf_gbuffer_motion is held to what the shade kernels are held to: no scratch and at most 128 VGPRs (four waves per SIMD). pt_motion_kernel,
the validation path, may use no scratch beyond the private traversal stack pt_gbuffer_kernel has."""
import pytest

from kernel_metadata import kernels as _kernels


@pytest.fixture(scope="module")
def wavefront():
    return _kernels("pt_wavefront.hip.o")


@pytest.fixture(scope="module")
def megakernel():
    return _kernels("pt_megakernel.hip.o")


def test_wf_gbuffer_motion_exists_without_scratch_at_four_waves(wavefront):
    motion = {n: k for n, k in wavefront.items() if n.startswith("wf_gbuffer_motion")}
    assert {"wf_gbuffer_motion<true>", "wf_gbuffer_motion<false>"} <= set(motion), sorted(wavefront)[:8]
    for n, k in motion.items():
        print(n, k)
        assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] == 0, (n, k)
    assert motion["wf_gbuffer_motion<false>"]["vgpr"] < motion["wf_gbuffer_motion<true>"]["vgpr"]      # motion only: none of gbuffer_texels' registers
    assert wavefront["wf_gbuffer"]["scratch"] == 0                                                         # the G-buffer call's own kernel is still there


def test_pt_motion_kernel_has_only_the_traversal_stack(megakernel):
    for tl in ("true", "false"):
        m, g = megakernel[f"pt_motion_kernel<{tl}>"], megakernel[f"pt_gbuffer_kernel<{tl}>"]
        print(tl, m, g)
        assert g["scratch"] > 0 and m["scratch"] <= g["scratch"], (tl, m, g)
