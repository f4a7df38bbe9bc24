"""Where wf_shade reads its triangle, instance and material records from (hobbyrenderer_amd/csrc/pt_wavefront_plan.h, RenderPlan::shadeLdsTables):
a per-block LDS copy when the three tables fit next to the specular-lobe ring and a CU still holds the four blocks the kernel is compiled for,
global memory otherwise. No GPU: a g++ driver over the header, as tests/test_wavefront_plan.py."""
import json
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hobbyrenderer_amd", "csrc")

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include "pt_wavefront_plan.h"
using namespace hrt;
int main(int argc, char** argv)
{
    SceneTraits t; TreeCounts c; WavefrontKnobs k; unsigned long long lights = 1;
    for (int i = 1; i < argc; ++i) {
        const std::string s = argv[i], name = s.substr(0, s.find('='));
        const long long v = atoll(s.c_str() + s.find('=') + 1);
        if (name == "lights") lights = v;
#define FIELD(obj, f) else if (name == #f) obj.f = (decltype(obj.f))v;
        FIELD(t, hasTextures) FIELD(t, hasTransmissiveOrBlend) FIELD(t, directionalLightsOnly) FIELD(t, twoLevelStackNeed) FIELD(t, bvhMaxDepth) FIELD(t, bvh4MaxDepth)
        FIELD(c, nodeCount) FIELD(c, node4Count) FIELD(c, triCount) FIELD(c, hasInstances) FIELD(c, instanceCount) FIELD(c, materialCount)
        FIELD(k, noShadeLdsTables)
        else { fprintf(stderr, "unknown input %s\n", name.c_str()); return 2; }
    }
    const RenderPlan p = plan_render(t, c, (uint32_t)lights, 256, k);
    printf("{\"shadeLdsTables\": %d, \"shadeTableBytes\": %zu, \"shadeLdsBytes\": %zu, \"simpleScene\": %d, \"ringBytes\": %zu, \"perBlock\": %zu, \"cuLds\": %zu, "
           "\"blocksPerCu\": %u, \"margin\": %zu, \"tri\": %zu, \"inst\": %zu, \"mat\": %zu}\n",
           p.shadeLdsTables, p.shadeTableBytes, p.shadeLdsBytes, p.simpleScene, kShadeRingBytes, kShadeLdsPerBlock, kCuLdsBytes, kShadeBlocksPerCu, kShadeLdsMargin,
           kTriAttrBytes, kInstShadeBytes, kMaterialBytes);
    return 0;
}
"""

# config 2 (scenes.config_cornell): 38 triangles in 9 instances, 4 materials
CONFIG2 = dict(nodeCount=37, node4Count=13, triCount=38, bvhMaxDepth=6, bvh4MaxDepth=3, instanceCount=9, materialCount=4)
RING = 4 * 64 * 23 * 4          # four waves x 64 parked paths x 23 floats


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("shade_tables_plan")
    (d / "driver.cpp").write_text(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(d / "driver"), str(d / "driver.cpp")])

    def run(**inputs):
        return json.loads(subprocess.check_output([str(d / "driver")] + [f"{k}={int(v)}" for k, v in inputs.items()]).decode())
    return run


def align16(n):
    return (n + 15) // 16 * 16


def test_config2_tables_go_to_lds(plan):
    p = plan(**CONFIG2)
    assert (p["tri"], p["inst"], p["mat"], p["ringBytes"]) == (80, 48, 180, RING)
    tables = align16(38 * 80 + 9 * 48 + 4 * 180)
    assert (p["simpleScene"], p["shadeLdsTables"], p["shadeTableBytes"], p["shadeLdsBytes"]) == (1, 1, tables, RING + tables)
    # four blocks per CU still fit: 160 KiB per CU, and the block keeps a margin for its static LDS and the allocation granularity
    assert (p["cuLds"], p["blocksPerCu"]) == (160 * 1024, 4) and p["margin"] >= 1024
    assert p["perBlock"] == p["cuLds"] // 4 - p["margin"]
    assert 4 * (p["shadeLdsBytes"] + p["margin"]) <= p["cuLds"]


def test_budget_boundary(plan):
    per_block = plan(**CONFIG2)["perBlock"]
    room = per_block - RING - align16(9 * 48 + 4 * 180)
    tris = room // 80
    fits = plan(**dict(CONFIG2, triCount=tris))
    assert fits["shadeLdsTables"] == 1 and fits["shadeLdsBytes"] == RING + align16(tris * 80 + 9 * 48 + 4 * 180) <= per_block
    over = plan(**dict(CONFIG2, triCount=tris + 1))          # one record more than the budget allows
    assert (over["shadeLdsTables"], over["shadeTableBytes"], over["shadeLdsBytes"]) == (0, 0, RING)
    # ... and the same boundary in materials
    room = per_block - RING - 38 * 80 - 9 * 48
    mats = max(m for m in range(1, room // 180 + 1) if RING + align16(38 * 80 + 9 * 48 + m * 180) <= per_block)
    assert plan(**dict(CONFIG2, materialCount=mats))["shadeLdsTables"] == 1
    assert plan(**dict(CONFIG2, materialCount=mats + 1))["shadeLdsTables"] == 0


def test_global_tables_otherwise(plan):
    assert plan(**CONFIG2, noShadeLdsTables=1)["shadeLdsTables"] == 0            # HRPT_WF_SHADE_LDS_TABLES=0
    assert plan(**CONFIG2, noShadeLdsTables=1)["shadeLdsBytes"] == RING
    # the two-level structure: per-mesh records, instance and material from the hit
    assert plan(**dict(CONFIG2, hasInstances=1, twoLevelStackNeed=20))["shadeLdsTables"] == 0
    # counts unknown (a caller that does not pass them)
    for unknown in ("instanceCount", "materialCount", "triCount"):
        assert plan(**dict(CONFIG2, **{unknown: 0}))["shadeLdsTables"] == 0, unknown
    # general variants (textures, transmission, point lights) and several lights: only the SIMPLE single-light variants have an LDS instantiation
    for general in (dict(hasTextures=1), dict(hasTransmissiveOrBlend=1), dict(directionalLightsOnly=0), dict(lights=3), dict(lights=9)):
        p = plan(**CONFIG2, **general)
        assert (p["shadeLdsTables"], p["shadeTableBytes"]) == (0, 0), general
