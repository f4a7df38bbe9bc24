"""RenderPlan::fusedBounce0 / bounce0LdsBytes (hobbyrenderer_amd/csrc/pt_wavefront_plan.h): when bounce 0 runs wf_bounce0 instead of the
wf_extend<PRIMARY> + wf_shade_lt<PRIMARY> pair, and with how much LDS. No GPU: a driver compiled with plain g++ against the header, the method of
tests/test_wavefront_plan.py (whose inputs and Cornell-class numbers are used here)."""
import json
import subprocess

import pytest

from test_wavefront_plan import CORNELL, CORNELL_TREE4, CSRC, KIB

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include "pt_wavefront_plan.h"
using namespace hrt;
int main(int argc, char** argv)
{
    SceneTraits t; TreeCounts c; WavefrontKnobs k;
    unsigned long long lights = 1;
    for (int i = 1; i < argc; ++i) {
        const std::string s = argv[i], name = s.substr(0, s.find('='));
        const long long v = atoll(s.c_str() + s.find('=') + 1);
        if (name == "lights") lights = v;
#define FIELD(obj, f) else if (name == #f) obj.f = (decltype(obj.f))v;
        FIELD(t, hasNonOpaque) FIELD(t, hasTextures) FIELD(t, bvhMaxDepth) FIELD(t, bvh4MaxDepth)
        FIELD(c, nodeCount) FIELD(c, node4Count) FIELD(c, triCount) FIELD(c, instanceCount) FIELD(c, materialCount)
        FIELD(k, noFusedPrimary) FIELD(k, noFusedBounce0) FIELD(k, noShadeLdsTables) FIELD(k, bvhWidth)
        else { fprintf(stderr, "unknown input %s\n", name.c_str()); return 2; }
    }
    const RenderPlan p = plan_render(t, c, (uint32_t)lights, 256, k);
    printf("{\"fusedBounce0\": %d, \"bounce0LdsBytes\": %zu, \"fusedPrimary\": %d, \"shadeLdsTables\": %d, \"shadeTableBytes\": %zu, \"shadeLdsBytes\": %zu, "
           "\"vElds\": %d, \"vEldsBytes\": %zu, \"perBlock\": %zu, \"ringBytes\": %zu}\n",
           p.fusedBounce0, p.bounce0LdsBytes, p.fusedPrimary, p.shadeLdsTables, p.shadeTableBytes, p.shadeLdsBytes, p.vE.lds, p.vE.ldsBytes,
           kShadeLdsPerBlock, kBounce0RingBytes);
    return 0;
}
"""

# the Cornell box of config 2: 36 triangles of 8 instances over 4 materials (the counts only size the tables)
TABLES = dict(instanceCount=8, materialCount=4)
TABLE_BYTES = (36 * 80 + 8 * 48 + 4 * 180 + 15) // 16 * 16


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("bounce0_plan")
    (d / "driver.cpp").write_text(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(d / "driver"), str(d / "driver.cpp")])

    def run(**inputs):
        return json.loads(subprocess.check_output([str(d / "driver")] + [f"{k}={int(v)}" for k, v in inputs.items()]).decode())
    return run


def test_on_for_the_cornell_class(plan):
    p = plan(**CORNELL, **TABLES)
    assert (p["fusedBounce0"], p["fusedPrimary"], p["shadeLdsTables"], p["vElds"]) == (1, 1, 1, 1)
    # stack columns + tree (the closest-hit variant's bytes) + four 32-entry rings of 23 floats + the tables padded to 128 bytes
    assert p["ringBytes"] == 4 * 32 * 23 * 4 and p["shadeTableBytes"] == TABLE_BYTES
    assert p["bounce0LdsBytes"] == 16 * KIB + CORNELL_TREE4 + p["ringBytes"] + (TABLE_BYTES + 127) // 128 * 128
    assert p["bounce0LdsBytes"] <= p["perBlock"] == 39 * KIB
    # the pair's own numbers are what they were
    assert p["vEldsBytes"] == 16 * KIB + CORNELL_TREE4 and p["shadeLdsBytes"] == 4 * 64 * 23 * 4 + TABLE_BYTES


def test_knob_keeps_the_pair(plan):
    p = plan(**CORNELL, **TABLES, noFusedBounce0=1)
    assert (p["fusedBounce0"], p["bounce0LdsBytes"], p["fusedPrimary"], p["shadeLdsTables"]) == (0, 0, 1, 1)


@pytest.mark.parametrize("off", [dict(noFusedPrimary=1), dict(hasNonOpaque=1), dict(lights=3), dict(instanceCount=0, materialCount=0),
                                 dict(noShadeLdsTables=1), dict(bvhWidth=2), dict(hasTextures=1)],
                         ids=["raygen-pass", "non-opaque-geometry", "several-lights", "table-counts-unknown", "global-tables", "two-wide-tree", "textures"])
def test_off_outside_the_class(plan, off):
    p = plan(**dict(dict(CORNELL, **TABLES), **off))
    assert (p["fusedBounce0"], p["bounce0LdsBytes"]) == (0, 0), p


def test_off_when_the_tree_does_not_fit(plan):
    # a tree that fits the closest-hit kernel's 64 KiB (so vE.lds stays on) but not a quarter of the CU next to ring and tables
    big = dict(CORNELL, node4Count=64, nodeCount=200, triCount=100, **TABLES)          # 8 192 + 4 800 B of tree, 9 104 B of tables
    p = plan(**big)
    assert (p["vElds"], p["shadeLdsTables"], p["fusedPrimary"], p["fusedBounce0"]) == (1, 1, 1, 0)
    # ... and one that does not fit LDS at all: no LDS variant, so no fused kernel either
    p = plan(**dict(CORNELL, node4Count=400, nodeCount=1200, triCount=600, **TABLES))
    assert (p["vElds"], p["fusedBounce0"]) == (0, 0)
    # the boundary: the largest triangle count at which the block still fits
    fits = [n for n in range(36, 100) if plan(**dict(CORNELL, triCount=n, **TABLES))["fusedBounce0"]]
    n = max(fits)
    assert fits == list(range(36, n + 1))
    assert plan(**dict(CORNELL, triCount=n, **TABLES))["bounce0LdsBytes"] <= 39 * KIB < \
        16 * KIB + 12 * 128 + (n + 1) * 48 + 4 * 32 * 23 * 4 + (((n + 1) * 80 + 8 * 48 + 4 * 180 + 15) // 16 * 16 + 127) // 128 * 128
