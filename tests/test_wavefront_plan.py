"""The launch policy of the wavefront pipeline (hobbyrenderer_amd/csrc/pt_wavefront_plan.h) without a GPU: a small driver compiled with plain
g++ against the header prints the plan for given scene traits, tree sizes and knobs; the expected values are the documented defaults
(the measured choices in the header's comments and DESIGN.md section 4), so flipping one of them fails here before a benchmark moves."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hobbyrenderer_amd", "csrc")

TRAITS = ["hasMedium", "hasStochasticAlpha", "hasTextures", "hasTransmissiveOrBlend", "directionalLightsOnly", "hasNonOpaque", "bvhMaxDepth",
          "bvh4MaxDepth", "quantisedNodes", "twoLevelStackNeed"]
TREE = ["nodeCount", "node4Count", "triCount", "hasNodesQ", "hasInstances"]
KNOBS = ["blocksPerCu", "extendBlocksPerCu", "refillMin", "segmentShift", "segmentSize", "drainSegments", "serialShadow", "padLdsBytes", "bvhWidth",
         "nodeLoopMin", "noFusedPrimary", "noSlimShadow", "shadeSort", "shadowPath"]

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include "pt_wavefront_plan.h"
using namespace hrt;
static void variant(const char* name, const Variant& v)
{
    printf("\"%s\": {\"lds\": %d, \"depth\": %d, \"width\": %d, \"ldsBytes\": %zu, \"twoLevel\": %d, \"twoLevelCandidates\": %d, \"quantised\": %d}, ",
           name, v.lds, v.depth, v.width, v.ldsBytes, v.twoLevel, v.twoLevelCandidates, v.quantised);
}
static void trace(const char* name, const TraceRaysPlan& p)
{
    printf("\"%s\": {", name); variant("v", p.v);
    printf("\"grid\": %u, \"refillMin\": %u, \"nodeLoopMin\": %u, \"spillEntries\": %u, \"spillThreads\": %zu}, ", p.grid, p.refillMin, p.nodeLoopMin, p.spillEntries, p.spillThreads);
}
int main(int argc, char** argv)
{
    SceneTraits t; TreeCounts c; WavefrontKnobs k;
    unsigned long long lights = 1, cus = 256, samples = 1, rays = 1;
    for (int i = 1; i < argc; ++i) {
        const std::string s = argv[i], name = s.substr(0, s.find('='));
        const long long v = atoll(s.c_str() + s.find('=') + 1);
        if (name == "lights") lights = v; else if (name == "cus") cus = v; else if (name == "samples") samples = v; else if (name == "rays") rays = v;
#define FIELD(obj, f) else if (name == #f) obj.f = (decltype(obj.f))v;
        @FIELDS@
        else { fprintf(stderr, "unknown input %s\n", name.c_str()); return 2; }
    }
    const RenderPlan p = plan_render(t, c, (uint32_t)lights, (uint32_t)cus, k);
    const BatchPlan b = plan_batch(p, k, (uint32_t)samples);
    printf("{"); variant("vE", p.vE); variant("vS", p.vS); variant("vA", p.vA);
    printf("\"shadowMode\": %d, \"slim\": %d, \"simpleScene\": %d, \"fusedPrimary\": %d, \"sortShade\": %u, \"nodeLoopMin\": %u, \"blocksPerCu\": %u, \"extendBlocksPerCu\": %u,\n",
           p.shadowMode, p.slim, p.simpleScene, p.fusedPrimary, p.sortShade, p.nodeLoopMin, p.blocksPerCu, p.extendBlocksPerCu);
    printf("\"spillEntries\": %u, \"spillThreads\": %zu, \"pathRecordBytes\": %u, \"bytesPerSample\": %llu,\n", p.spillEntries, p.spillThreads, p.pathRecordBytes, (unsigned long long)p.bytesPerSample);
    printf("\"segSize\": %u, \"numSegments\": %u, \"grid\": %u, \"gridExtend\": %u,\n", b.segSize, b.numSegments, b.grid, b.gridExtend);
    trace("closest", plan_trace_rays(t, c, rays, false, (uint32_t)cus, k)); trace("shadow", plan_trace_rays(t, c, rays, true, (uint32_t)cus, k));
    printf("\"traceRaysSupported\": %d, \"kLdsBudget\": %zu, \"kMaxStackNeed\": %u, \"kMaxLights\": %u, \"kBlock\": %u}\n", wavefront_trace_rays_supported(t), kLdsBudget, kMaxStackNeed, kMaxLights, kBlock);
    return 0;
}
"""

OPAQUE, BUFFERED, RESOLVE, SLIM = 0, 1, 2, 3      # kShadow* mode codes
KIB = 1024                                        # one stack entry of a 256-thread block: 256 lanes x 4 bytes


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
    fields = "".join(f"FIELD({o}, {f}) " for o, names in (("t", TRAITS), ("c", TREE), ("k", KNOBS)) for f in names)
    (d / "driver.cpp").write_text(DRIVER.replace("@FIELDS@", fields))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(d / "driver"), str(d / "driver.cpp")])

    def run(**inputs):
        out = subprocess.check_output([str(d / "driver")] + [f"{k}={int(v)}" for k, v in inputs.items()]).decode()
        return json.loads(out)
    return run


# Cornell-class scene: 12 four-wide nodes (35 two-wide) + 36 triangles, all opaque, one directional light, no textures
CORNELL = dict(nodeCount=35, node4Count=12, triCount=36, bvhMaxDepth=5, bvh4MaxDepth=3)
CORNELL_TREE4, CORNELL_TREE2 = 12 * 128 + 36 * 48, 35 * 64 + 36 * 48
# 100 k triangles in global memory, opaque, textured; stack need 3 * (9 + 1) = 30 -> class 32
BIG = dict(nodeCount=100000, node4Count=40000, triCount=100000, bvhMaxDepth=24, bvh4MaxDepth=9, hasTextures=1)


def variant(v):
    return (v["lds"], v["depth"], v["width"], v["ldsBytes"], v["quantised"], v["twoLevel"])


def test_cornell_class_defaults(plan):
    for serial in (0, 1):       # one lane of a frames-in-flight loop changes nothing for a tree in LDS
        p = plan(**CORNELL, serialShadow=serial, samples=8 << 20)
        assert variant(p["vE"]) == (1, 16, 4, 16 * KIB + CORNELL_TREE4, 0, 0)
        assert variant(p["vS"]) == (1, 8, 2, 8 * KIB + CORNELL_TREE2, 0, 0)       # the small opaque any-hit kernel over an LDS tree is faster 2-wide
        assert (p["shadowMode"], p["slim"], p["simpleScene"], p["fusedPrimary"], p["sortShade"]) == (SLIM, 1, 1, 1, 0)
        assert (p["nodeLoopMin"], p["blocksPerCu"], p["extendBlocksPerCu"]) == (16, 16, 12)
        assert (p["spillEntries"], p["pathRecordBytes"], p["bytesPerSample"]) == (0, 48, 16 * 14)     # 2 x 3 path streams + hit + 5 + 1 shadow + radiance
        assert (p["segSize"], p["numSegments"], p["grid"], p["gridExtend"]) == (512, 16384, 256 * 16, 256 * 12)
    assert plan(**CORNELL, samples=(8 << 20) - 1)["segSize"] == 256
    small = plan(**CORNELL, samples=1000)
    assert (small["segSize"], small["numSegments"], small["grid"], small["gridExtend"]) == (256, 4, 1, 1)
    assert plan(**CORNELL, noSlimShadow=1)["shadowMode"] == OPAQUE and plan(**CORNELL, noFusedPrimary=1)["fusedPrimary"] == 0


def test_big_textured_scene(plan):
    for q in (0, 1):
        p = plan(**BIG, quantisedNodes=q, hasNodesQ=1, samples=16 << 20)
        assert variant(p["vE"]) == (0, 32, 4, 16 * KIB, q, 0) and variant(p["vS"]) == (0, 32, 4, 32 * KIB, q, 0)
        assert (p["shadowMode"], p["slim"], p["simpleScene"], p["fusedPrimary"], p["sortShade"]) == (OPAQUE, 0, 0, 0, 1)
        assert (p["nodeLoopMin"], p["blocksPerCu"], p["extendBlocksPerCu"], p["segSize"]) == (24, 16, 6, 256)
        assert (p["spillEntries"], p["spillThreads"]) == (30 - 16, 256 * 16 * 256)
        s = plan(**BIG, quantisedNodes=q, hasNodesQ=1, serialShadow=1)
        assert (s["blocksPerCu"], s["extendBlocksPerCu"], s["spillThreads"]) == (8, 6, 256 * 8 * 256)
    assert plan(**BIG, quantisedNodes=1, hasNodesQ=0)["vE"]["quantised"] == 0


def test_shadow_schedule(plan):
    glass = plan(**BIG, hasNonOpaque=1, hasTransmissiveOrBlend=1)
    assert glass["shadowMode"] == RESOLVE
    assert variant(glass["vS"]) == (0, 32, 4, 16 * KIB, 0, 0)       # resolve only: the extend stack size, no candidate columns
    assert variant(glass["vA"]) == (0, 32, 4, 16 * KIB, 0, 0)
    assert glass["bytesPerSample"] == 16 * 14 + 16 + 16 + 4 + 4 + 8 * 8
    foliage = plan(**BIG, hasNonOpaque=1)
    assert foliage["shadowMode"] == BUFFERED and variant(foliage["vS"]) == (0, 32, 4, 32 * KIB, 0, 0)
    lights3 = plan(**CORNELL, lights=3)
    assert (lights3["shadowMode"], lights3["vS"]["lds"], lights3["vS"]["width"], lights3["fusedPrimary"]) == (OPAQUE, 1, 2, 0)
    assert plan(**BIG, lights=3)["shadowMode"] == RESOLVE
    # HRPT_WF_SHADOW_PATH
    forced1 = plan(**BIG, hasNonOpaque=1, hasTransmissiveOrBlend=1, shadowPath=1)
    assert forced1["shadowMode"] == BUFFERED and variant(forced1["vS"]) == (0, 32, 4, 32 * KIB, 0, 0)
    assert plan(**BIG, lights=3, shadowPath=1)["shadowMode"] == OPAQUE
    assert plan(**BIG, hasNonOpaque=1, shadowPath=2)["shadowMode"] == RESOLVE
    assert plan(**CORNELL, hasNonOpaque=1, shadowPath=2)["shadowMode"] == RESOLVE
    assert plan(**BIG, shadowPath=2)["shadowMode"] == OPAQUE and plan(**CORNELL, shadowPath=2)["shadowMode"] == SLIM


def test_forced_width(plan):
    w2, w4 = plan(**CORNELL, bvhWidth=2), plan(**CORNELL, bvhWidth=4)
    assert [w2[v]["width"] for v in ("vE", "vS", "vA")] == [2, 2, 2] and w2["fusedPrimary"] == 0 and w2["shadowMode"] == SLIM
    assert [w4[v]["width"] for v in ("vE", "vS", "vA")] == [4, 4, 4] and w4["fusedPrimary"] == 1
    assert variant(w4["vS"]) == (1, 16, 4, 16 * KIB + CORNELL_TREE4, 0, 0)


def test_deepest_supported_tree(plan):
    deep = dict(BIG, bvhMaxDepth=70)
    p = plan(**dict(deep, bvh4MaxDepth=41))         # stack need 3 * 42 = 126 <= kMaxStackNeed
    assert p["kMaxStackNeed"] == 128 and p["traceRaysSupported"] == 1
    assert variant(p["vE"]) == (0, 64, 4, 16 * KIB, 0, 0) and variant(p["vS"]) == (0, 64, 4, 32 * KIB, 0, 0) and p["spillEntries"] == 126 - 16
    p = plan(**dict(deep, bvh4MaxDepth=42))         # 129: the 2-wide tree
    assert p["traceRaysSupported"] == 0
    assert variant(p["vE"]) == (0, 64, 2, 16 * KIB, 0, 0) and variant(p["vS"]) == (0, 64, 2, 32 * KIB, 0, 0) and p["spillEntries"] == 72 - 16
    assert plan(twoLevelStackNeed=128, hasInstances=1)["traceRaysSupported"] == 1 and plan(twoLevelStackNeed=129, hasInstances=1)["traceRaysSupported"] == 0


def test_depth_classes(plan):
    def stacks(p, cls, trace=True):
        assert (p["vE"]["depth"], p["vS"]["depth"]) == (cls, cls)
        assert (p["vE"]["ldsBytes"], p["vS"]["ldsBytes"]) == (min(cls, 16) * KIB, min(cls, 32) * KIB)      # LDS entries of the extend / shadow kernel class
        assert not trace or (p["closest"]["v"]["depth"], p["closest"]["v"]["ldsBytes"]) == (cls, min(cls, 16) * KIB)
    for need, cls in ((16, 16), (17, 32), (32, 32), (33, 64)):
        stacks(plan(twoLevelStackNeed=need, hasInstances=1, node4Count=100, triCount=100), cls)
    for depth4, cls in ((4, 16), (5, 32), (9, 32), (10, 64)):          # need 3 * (depth4 + 1) = 15 / 18 / 30 / 33
        stacks(plan(**dict(BIG, bvh4MaxDepth=depth4)), cls)
    for depth2, cls in ((6, 8), (7, 16), (14, 16), (15, 32), (30, 32), (31, 64)):       # need depth + 2
        stacks(plan(**dict(BIG, bvhMaxDepth=depth2, bvhWidth=2)), cls, trace=False)       # (ray queries walk the 4-wide tree whatever the knob says)


def test_lds_budget_boundary(plan):
    fits = dict(node4Count=192, nodeCount=2000, triCount=512, bvh4MaxDepth=4, bvhMaxDepth=12)      # 24 576 + 24 576 B of tree
    p = plan(**fits)
    assert p["kLdsBudget"] == 64 * KIB == 192 * 128 + 512 * 48 + 16 * KIB
    assert variant(p["vE"]) == (1, 16, 4, 64 * KIB, 0, 0) and p["nodeLoopMin"] == 16 and p["extendBlocksPerCu"] == 12
    assert variant(p["vA"]) == (0, 16, 4, 16 * KIB, 0, 0)       # the any-hit pass adds 16 KiB of candidate columns
    assert p["closest"]["v"]["lds"] == 1 and p["shadow"]["v"]["lds"] == 0
    p = plan(**dict(fits, triCount=513))
    assert variant(p["vE"]) == (0, 16, 4, 16 * KIB, 0, 0) and p["nodeLoopMin"] == 24 and p["extendBlocksPerCu"] == 6
    assert p["closest"]["v"]["lds"] == 0
    assert plan(**dict(fits, padLdsBytes=4096))["vE"] == dict(p["vE"], lds=1, ldsBytes=64 * KIB + 4096)     # padding is added to the launch, not counted


def test_two_level(plan):
    tl = dict(twoLevelStackNeed=20, hasInstances=1, node4Count=10, triCount=20, hasTextures=1, quantisedNodes=1, hasNodesQ=1)
    for non_opaque in (0, 1):
        p = plan(**tl, hasNonOpaque=non_opaque, hasTransmissiveOrBlend=non_opaque)
        for v, entries in (("vE", 16), ("vS", 32)):
            assert variant(p[v]) == (0, 32, 4, entries * KIB, 0, 1) and p[v]["twoLevelCandidates"] == non_opaque
        assert p["shadowMode"] == OPAQUE and (p["extendBlocksPerCu"], p["nodeLoopMin"]) == (6, 24)
        assert (p["spillEntries"], p["bytesPerSample"]) == (4, 16 * 14 + 4 + (104 if non_opaque else 0))
        for q in ("closest", "shadow"):
            assert variant(p[q]["v"]) == (0, 32, 4, 16 * KIB, 0, 1) and p[q]["spillEntries"] == 4
    assert plan(**dict(tl, hasTextures=0))["shadowMode"] == SLIM and plan(**dict(tl, hasTextures=0))["fusedPrimary"] == 1


def test_fused_primary_conditions(plan):
    assert plan(**CORNELL)["fusedPrimary"] == 1 and plan(**CORNELL)["kMaxLights"] == 8
    for off in (dict(lights=9), dict(lights=2), dict(hasMedium=1), dict(hasStochasticAlpha=1), dict(hasTextures=1), dict(directionalLightsOnly=0)):
        assert plan(**CORNELL, **off)["fusedPrimary"] == 0, off
    assert plan(**CORNELL, hasMedium=1)["pathRecordBytes"] == 80 and plan(**CORNELL, hasMedium=1)["bytesPerSample"] == 16 * 18


def test_trace_rays(plan):
    def both(**inputs):
        p = plan(**inputs)
        return p["closest"], p["shadow"]
    c, s = both(**CORNELL, rays=1000)
    assert variant(c["v"]) == variant(s["v"]) == (1, 16, 4, 16 * KIB + CORNELL_TREE4, 0, 0)       # (the launch adds the shadow query's candidate columns)
    assert (c["grid"], c["refillMin"], c["nodeLoopMin"], c["spillEntries"]) == (1, 12, 16, 0)        # ceil(ceil(1000 / 256) / 4) blocks
    assert both(**CORNELL, rays=1000, padLdsBytes=4096, bvhWidth=2) == (c, s)
    for q in (0, 1):
        c, s = both(**BIG, quantisedNodes=q, hasNodesQ=1, rays=10_000_000)
        assert variant(c["v"]) == variant(s["v"]) == (0, 32, 4, 16 * KIB, q, 0)
        assert (c["grid"], c["nodeLoopMin"], c["spillEntries"], c["spillThreads"]) == (256 * 16, 24, 30 - 16, 256 * 16 * 256)
    assert both(**BIG, rays=4096 * 1024 - 1024)[0]["grid"] == 4095 and both(**BIG, rays=5000, blocksPerCu=8, cus=2)[1]["grid"] == 5
