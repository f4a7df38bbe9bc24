"""wf_bounce0 (bounce 0 traced and shaded in one kernel, pt_wf_shade.h): register, scratch and LDS budget of every instantiation, read from
the code-object metadata of the built library -- tests/kernel_metadata.py reads it, no GPU needed.

The kernel is compiled for a forced four waves per SIMD like wf_shade, whose history of miscompiles under register pressure is told in
tests/test_kernel_resources.py: no scratch and at most 128 VGPRs. Four waves per SIMD are four 256-thread blocks per CU, so the static LDS
plus the dynamic LDS of the plan (at most kShadeLdsPerBlock: above it the plan keeps the two-kernel pair) must fit a quarter of the CU's 160 KiB."""
import json
import subprocess

import pytest

import kernel_metadata
from kernel_metadata import CSRC
from test_kernel_resources_shade_lt import BLOCKS_PER_CU, CU_LDS
from test_wavefront_plan import CORNELL

PLAN = r"""
#include <stdio.h>
#include "pt_wavefront_plan.h"
using namespace hrt;
int main()
{
    SceneTraits t; TreeCounts c; WavefrontKnobs k;
    t.bvhMaxDepth = @bvhMaxDepth@; t.bvh4MaxDepth = @bvh4MaxDepth@; c.nodeCount = @nodeCount@; c.node4Count = @node4Count@; c.triCount = @triCount@;
    c.instanceCount = 8; c.materialCount = 4;
    const RenderPlan p = plan_render(t, c, 1, 256, k);
    printf("{\"fusedBounce0\": %d, \"bounce0LdsBytes\": %zu, \"perBlock\": %zu, \"margin\": %zu}\n", p.fusedBounce0, p.bounce0LdsBytes, kShadeLdsPerBlock, kShadeLdsMargin);
    return 0;
}
"""


@pytest.fixture(scope="module")
def kernels():
    return {n: k for n, k in kernel_metadata.kernels("pt_wavefront.hip.o").items() if "wf_bounce0" in n}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("bounce0_limits")
    src = PLAN
    for k, v in CORNELL.items():
        src = src.replace(f"@{k}@", str(v))
    (d / "plan.cpp").write_text(src)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(d / "plan"), str(d / "plan.cpp")])
    return json.loads(subprocess.check_output([str(d / "plan")]).decode())


def test_instantiations_exist(kernels):
    assert set(kernels) == {"wf_bounce0<16>", "wf_bounce0<32>", "wf_bounce0<64>"}        # one per stack class of the closest-hit variant


def test_no_scratch_and_four_waves(kernels):
    for n, k in kernels.items():
        assert k["scratch"] == 0 and k["vgpr"] <= 128, (n, k)


def test_four_blocks_per_cu_fit_lds(kernels, plan):
    assert plan["fusedBounce0"] == 1 and 0 < plan["bounce0LdsBytes"] <= plan["perBlock"]
    for n, k in kernels.items():
        assert k["lds"] <= plan["margin"], (n, k)              # static LDS stays inside the margin the plan keeps back
        assert BLOCKS_PER_CU * (k["lds"] + plan["bounce0LdsBytes"]) <= CU_LDS, (n, k)
        assert BLOCKS_PER_CU * (k["lds"] + plan["perBlock"]) <= CU_LDS, (n, k)       # ... at the largest size the plan lets through, too
