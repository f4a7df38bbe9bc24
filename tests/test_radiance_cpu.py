"""hrpt_trace_radiance without a GPU: the ABI surface and the launch plan -- plan_radiance is plan_render with the two
bounce-0 forms off that derive rays from the sample index, and nothing else changed; the batch arithmetic of radiance_batch_rays."""
import json
import os
import subprocess

import numpy as np
import pytest

from hobbyrenderer_amd import native, structs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hobbyrenderer_amd", "csrc")


def test_symbol_is_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "hobbyrt_pt.h")).read()
    assert "hrpt_trace_radiance" in native.EXPORTS and native.lib.hrpt_trace_radiance is not None
    assert "hrpt_trace_radiance(" in hdr
    assert callable(native.PathTracerContext.trace_radiance) and callable(native.PathTracerContext.trace_radiance_device)


def test_flag_values_match_header():
    # that the C header gives the mirrored names the same values, and HrptRay the same size: test_binding_contract.py
    assert (S.RADIANCE_DEVICE_POINTERS, S.RADIANCE_THREAD_PER_RAY, S.RADIANCE_ACCUMULATE, S.ABI_VERSION) == (0x100, 0x200, 0x400, 3)
    # the same meaning keeps the same bit as in hrpt_trace_rays; the new one is a bit of its own, clear of that call's query kinds too
    assert S.RADIANCE_DEVICE_POINTERS == S.RAYS_DEVICE_POINTERS and S.RADIANCE_THREAD_PER_RAY == S.RAYS_THREAD_PER_RAY
    assert S.RADIANCE_ACCUMULATE & (S.RAYS_DEVICE_POINTERS | S.RAYS_THREAD_PER_RAY | 0xFF) == 0
    assert len({S.RADIANCE_DEVICE_POINTERS, S.RADIANCE_THREAD_PER_RAY, S.RADIANCE_ACCUMULATE}) == 3


def test_null_context_without_a_device():
    rays, out, cb = np.zeros(4, S.Ray), np.zeros((4, 4), np.float32), np.zeros((), S.PathTracerConstants)
    for flags in (0, S.RADIANCE_ACCUMULATE, S.RADIANCE_THREAD_PER_RAY, 0x800):
        assert native.lib.hrpt_trace_radiance(None, rays.ctypes.data, out.ctypes.data, 4, cb.ctypes.data, flags) == -1
    assert native.lib.hrpt_trace_radiance(None, None, None, 0, None, 0) == -1
    assert not out.any()


# ---------------------------------------------------------------- the plan
PLAN_FIELDS = ["shadowMode", "slim", "simpleScene", "sortShade", "nodeLoopMin", "maxLights", "cus", "blocksPerCu", "extendBlocksPerCu", "spillEntries",
               "spillThreads", "pathRecordBytes", "bytesPerSample", "shadeLdsTables", "shadeTableBytes", "shadeLdsBytes"]
TRAITS = ["hasMedium", "hasStochasticAlpha", "hasTextures", "hasTransmissiveOrBlend", "directionalLightsOnly", "hasNonOpaque", "bvhMaxDepth",
          "bvh4MaxDepth", "quantisedNodes", "twoLevelStackNeed"]
TREE = ["nodeCount", "node4Count", "triCount", "hasNodesQ", "hasInstances", "instanceCount", "materialCount"]
KNOBS = ["blocksPerCu", "segmentSize", "serialShadow", "bvhWidth", "noFusedPrimary", "noFusedBounce0", "noSlimShadow", "noShadeLdsTables", "shadeSort",
         "shadowPath", "radianceBatch"]

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include "pt_wavefront_plan.h"
using namespace hrt;
static void variant(const char* name, const Variant& v)
{
    printf("\"%s\": [%d, %d, %d, %zu, %d, %d, %d], ", name, v.lds, v.depth, v.width, v.ldsBytes, v.twoLevel, v.twoLevelCandidates, v.quantised);
}
static void plan(const char* name, const RenderPlan& p, const WavefrontKnobs& k, unsigned samples)
{
    printf("\"%s\": {", name); variant("vE", p.vE); variant("vS", p.vS); variant("vA", p.vA);
#define OUT(f) printf("\"" #f "\": %llu, ", (unsigned long long)p.f);
    @OUT@
    const BatchPlan b = plan_batch(p, k, samples);
    printf("\"batch\": [%u, %u, %u, %u], \"fusedPrimary\": %d, \"fusedBounce0\": %d, \"bounce0LdsBytes\": %zu}, ", b.segSize, b.numSegments, b.grid, b.gridExtend,
           p.fusedPrimary, p.fusedBounce0, p.bounce0LdsBytes);
}
int main(int argc, char** argv)
{
    SceneTraits t; TreeCounts c; WavefrontKnobs k;
    unsigned long long lights = 1, cus = 256, samples = 1, count = 1, budget = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string s = argv[i], name = s.substr(0, s.find('='));
        const long long v = atoll(s.c_str() + s.find('=') + 1);
        if (name == "lights") lights = v; else if (name == "cus") cus = v; else if (name == "samples") samples = v; else if (name == "count") count = v;
        else if (name == "budget") budget = v;
#define FIELD(obj, f) else if (name == #f) obj.f = (decltype(obj.f))v;
        @FIELDS@
        else { fprintf(stderr, "unknown input %s\n", name.c_str()); return 2; }
    }
    const RenderPlan r = plan_radiance(t, c, (uint32_t)lights, (uint32_t)cus, k);
    WavefrontKnobs off = k; off.noFusedPrimary = true;
    printf("{"); plan("render", plan_render(t, c, (uint32_t)lights, (uint32_t)cus, k), k, (unsigned)samples);
    plan("renderNoFusedPrimary", plan_render(t, c, (uint32_t)lights, (uint32_t)cus, off), off, (unsigned)samples);
    plan("radiance", r, k, (unsigned)samples);
    const uint64_t batch = radiance_batch_rays(count, r, budget, k);
    printf("\"batchRays\": %llu, \"capacity\": %llu, \"batches\": %llu, \"kMaxSegment\": %u}\n", (unsigned long long)batch,
           (unsigned long long)radiance_capacity(batch), (unsigned long long)((count + batch - 1) / batch), kMaxSegment);
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("radiance_plan")
    fields = "".join(f"FIELD({o}, {f}) " for o, names in (("t", TRAITS), ("c", TREE), ("k", KNOBS)) for f in names)
    (d / "driver.cpp").write_text(DRIVER.replace("@FIELDS@", fields).replace("@OUT@", " ".join(f"OUT({f})" for f in PLAN_FIELDS)))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(d / "driver"), str(d / "driver.cpp")])

    def run(**inputs):
        return json.loads(subprocess.check_output([str(d / "driver")] + [f"{k}={int(v)}" for k, v in inputs.items()]).decode())
    return run


# Cornell-class: tree and shade tables in LDS, one directional light -> a render fuses the primary rays and bounce 0
CORNELL = dict(nodeCount=35, node4Count=12, triCount=36, bvhMaxDepth=5, bvh4MaxDepth=3, instanceCount=9, materialCount=4)
# SIMPLE scene whose tree does not fit LDS: fused primary rays, but no fused bounce 0
MEDIUM = dict(nodeCount=9000, node4Count=3500, triCount=9000, bvhMaxDepth=16, bvh4MaxDepth=8, instanceCount=20, materialCount=6)
BIG = dict(nodeCount=100000, node4Count=40000, triCount=100000, bvhMaxDepth=24, bvh4MaxDepth=9, hasTextures=1)
GLASS = dict(BIG, hasNonOpaque=1, hasTransmissiveOrBlend=1, hasMedium=1, hasStochasticAlpha=1, directionalLightsOnly=0)
TWO_LEVEL = dict(BIG, twoLevelStackNeed=40, hasInstances=1, hasNonOpaque=1)


def test_plan_radiance_is_the_render_plan_without_the_fused_bounce0_forms(plan):
    fused = {"cornell": (1, 1), "medium": (1, 0)}
    for name, traits in (("cornell", CORNELL), ("medium", MEDIUM), ("big", BIG), ("glass", GLASS), ("two-level", TWO_LEVEL)):
        for extra in (dict(), dict(lights=3), dict(serialShadow=1), dict(noSlimShadow=1, noShadeLdsTables=1), dict(shadowPath=2), dict(bvhWidth=2)):
            p = plan(**traits, **extra, samples=20011)
            render, off, rad = p["render"], p["renderNoFusedPrimary"], p["radiance"]
            assert (rad["fusedPrimary"], rad["fusedBounce0"], rad["bounce0LdsBytes"]) == (0, 0, 0), (name, extra)
            if not extra:
                assert (render["fusedPrimary"], render["fusedBounce0"]) == fused.get(name, (0, 0)), name       # the traits where plan_render sets them
            assert rad == off, (name, extra)                                                            # every field, variants and batch included
            for f in PLAN_FIELDS + ["vE", "vS", "vA", "batch"]:                                         # ... which is the render's own choice
                assert rad[f] == render[f], (name, extra, f)
    assert plan(**CORNELL, noFusedPrimary=1)["radiance"] == plan(**CORNELL)["radiance"]


def test_batch_arithmetic(plan):
    for count in (1, 63, 64, 1025):
        p = plan(**CORNELL, count=count)
        assert (p["batchRays"], p["batches"]) == (count, 1) and p["capacity"] == (1024 if count <= 1024 else 2048) and p["kMaxSegment"] == 1024
    # HRPT_RADIANCE_BATCH
    p = plan(**CORNELL, count=20011, radianceBatch=1024)
    assert (p["batchRays"], p["capacity"], p["batches"]) == (1024, 1024, 20) and 20011 - 19 * 1024 == 555
    for count, batches in ((1, 1), (63, 1), (64, 1), (1025, 17)):
        p = plan(**CORNELL, count=count, radianceBatch=64)
        assert (p["batchRays"], p["capacity"], p["batches"]) == (min(count, 64), 1024, batches)
    assert plan(**CORNELL, count=1025, radianceBatch=1000)["batches"] == 2
    # 64 Mi rays at most, less when the pool budget says so or 32-bit (entry, light) slot ids would run out
    assert plan(**CORNELL, count=1 << 31)["batchRays"] == 64 << 20
    per = plan(**CORNELL)["radiance"]["bytesPerSample"]
    assert plan(**CORNELL, count=1 << 31, budget=per * 5000 + 7)["batchRays"] == 5000
    assert plan(**CORNELL, count=1 << 31, budget=1)["batchRays"] == 1
    assert plan(**BIG, count=1 << 31, lights=300)["batchRays"] == 0xFFFFFFFF // 300
