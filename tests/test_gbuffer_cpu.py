"""First-hit G-buffer (hrpt_render_gbuffer) without a GPU: the ABI surface, the launch plan, and the NumPy reference
(tests/gbuffer_reference.py) checked against itself on the cube scene."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from hobbyrenderer_amd import native, scenes, structs as S
import gbuffer_reference as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hobbyrenderer_amd", "csrc")
SYMBOLS = ("hrpt_render_gbuffer", "hrpt_read_gbuffer", "hrpt_get_gbuffer_device")


def test_symbols_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "hobbyrt_pt.h")).read()
    for name in SYMBOLS:
        assert name in native.EXPORTS and getattr(native.lib, name) is not None
        assert name + "(" in hdr


def test_null_context_and_bad_arguments_without_a_device():
    p = np.zeros((), S.FrameParams)
    p["accumCount"] = 1
    buf = np.zeros(16, np.float32)
    ptr = C.c_void_p()
    # NULL context: -1 whatever the other arguments say (no context can exist without a device, so every other code needs one: GPU suite)
    for mask in (0, 1, S.GB_ALL_PLANES, 1 << S.GB_PLANES, 0xFFFFFFFF):
        assert native.lib.hrpt_render_gbuffer(None, p.ctypes.data, mask) == -1
        assert native.lib.hrpt_render_gbuffer(None, None, mask) == -1
    for plane in (0, S.GB_IDS, S.GB_PLANES, 99):
        assert native.lib.hrpt_read_gbuffer(None, plane, buf.ctypes.data, buf.nbytes) == -1
        assert native.lib.hrpt_read_gbuffer(None, plane, None, 0) == -1
        assert native.lib.hrpt_get_gbuffer_device(None, plane, C.byref(ptr)) == -1
        assert native.lib.hrpt_get_gbuffer_device(None, plane, None) == -1


def test_plane_constants_match_header(tmp_path):
    """The two status codes the calls return, which have no mirror, from a C program compiled from include/hobbyrt_pt.h; the mirrored
    HRPT_GB_* names and sizeof(HrptFrameParams) are compared with the header in test_binding_contract.py."""
    names = ["HRPT_ERR_NO_SCENE", "HRPT_ERR_INVALID_ARGUMENT"]
    src = tmp_path / "gb.c"
    src.write_text('#include <stdio.h>\n#include "hobbyrt_pt.h"\nint main(void){\n' + "".join(f'printf("%ld\\n", (long)({n}));\n' for n in names) + 'return 0;}\n')
    exe = tmp_path / "gb"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).decode().split()] == [-4, -1]
    assert (S.GB_PLANES, S.GB_ALL_PLANES, S.ABI_VERSION) == (6, 0x3F, 3)            # six planes, and the ABI version this addition keeps


PLAN_DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include "pt_wavefront_plan.h"
using namespace hrt;
static void variant(const Variant& v) { printf("[%d, %d, %d, %zu, %d, %d, %d]", v.lds, v.depth, v.width, v.ldsBytes, v.twoLevel, v.twoLevelCandidates, v.quantised); }
int main(int argc, char** argv)
{
    SceneTraits t; TreeCounts c; WavefrontKnobs k;
    unsigned long long lights = 1, cus = 256, samples = 1;
    for (int i = 1; i < argc; ++i) {
        const std::string s = argv[i], name = s.substr(0, s.find('='));
        const long long v = atoll(s.c_str() + s.find('=') + 1);
        if (name == "lights") lights = v; else if (name == "cus") cus = v; else if (name == "samples") samples = v;
#define FIELD(obj, f) else if (name == #f) obj.f = (decltype(obj.f))v;
        FIELD(t, hasMedium) FIELD(t, hasStochasticAlpha) FIELD(t, hasTextures) FIELD(t, hasTransmissiveOrBlend) FIELD(t, directionalLightsOnly)
        FIELD(t, hasNonOpaque) FIELD(t, bvhMaxDepth) FIELD(t, bvh4MaxDepth) FIELD(t, quantisedNodes) FIELD(t, twoLevelStackNeed)
        FIELD(c, nodeCount) FIELD(c, node4Count) FIELD(c, triCount) FIELD(c, hasNodesQ) FIELD(c, hasInstances)
        FIELD(k, bvhWidth) FIELD(k, segmentShift) FIELD(k, blocksPerCu) FIELD(k, extendBlocksPerCu)
        else { fprintf(stderr, "unknown input %s\n", name.c_str()); return 2; }
    }
    const RenderPlan p = plan_render(t, c, (uint32_t)lights, (uint32_t)cus, k);
    const BatchPlan b = plan_batch(p, k, (uint32_t)samples);
    const GBufferPlan g = plan_gbuffer(t, c, (uint32_t)cus, k, (uint32_t)samples);
    printf("{\"render\": {\"vE\": "); variant(p.vE);
    printf(", \"batch\": [%u, %u, %u, %u], \"nodeLoopMin\": %u, \"spill\": [%u, %zu], \"pathRecordBytes\": %u},\n", b.segSize, b.numSegments, b.grid, b.gridExtend, p.nodeLoopMin,
           p.spillEntries, p.spillThreads, p.pathRecordBytes);
    printf("\"gbuffer\": {\"vE\": "); variant(g.vE);
    printf(", \"batch\": [%u, %u, %u, %u], \"nodeLoopMin\": %u, \"spill\": [%u, %zu], \"pathRecordBytes\": %u}, \"bytesPerSample\": %llu}\n", g.batch.segSize, g.batch.numSegments,
           g.batch.grid, g.batch.gridExtend, g.nodeLoopMin, g.spillEntries, g.spillThreads, g.pathRecordBytes, (unsigned long long)g.bytesPerSample);
    return 0;
}
"""

# the scene classes of tests/test_wavefront_plan.py
CORNELL = dict(nodeCount=35, node4Count=12, triCount=36, bvhMaxDepth=5, bvh4MaxDepth=3)                                    # config 2: tree in LDS
BIG = dict(nodeCount=100000, node4Count=40000, triCount=100000, bvhMaxDepth=24, bvh4MaxDepth=9, hasTextures=1)             # tree in global memory
BIG_Q = dict(BIG, quantisedNodes=1, hasNodesQ=1)                                                                           # ... through quantised nodes
TWO_LEVEL = dict(nodeCount=0, node4Count=5000, triCount=20000, bvhMaxDepth=0, bvh4MaxDepth=0, twoLevelStackNeed=40, hasInstances=1, hasNonOpaque=1)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("gbplan")
    (d / "driver.cpp").write_text(PLAN_DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(d / "driver"), str(d / "driver.cpp")])

    def run(**inputs):
        return json.loads(subprocess.check_output([str(d / "driver")] + [f"{k}={int(v)}" for k, v in inputs.items()]).decode())
    return run


@pytest.mark.parametrize("scene", ["cornell", "global", "global_quantised", "two_level"])
@pytest.mark.parametrize("samples", [61 * 37, 1920 * 1080, 9 << 20])
@pytest.mark.parametrize("knobs", [dict(), dict(bvhWidth=2), dict(segmentShift=7, blocksPerCu=8)])
def test_plan_gbuffer_is_the_renders_front_end(plan, scene, samples, knobs):
    """Same closest-hit variant, LDS bytes, segments and grids as plan_render + plan_batch give a single-light render of the scene."""
    traits = dict(cornell=CORNELL, **{"global": BIG}, global_quantised=BIG_Q, two_level=TWO_LEVEL)[scene]
    p = plan(**traits, **knobs, samples=samples)
    r, g = p["render"], p["gbuffer"]
    assert g == r, (r, g)
    lds, depth, width, lds_bytes, two_level, _, quantised = g["vE"]
    assert bool(lds) == (scene == "cornell") and bool(two_level) == (scene == "two_level")
    assert bool(quantised) == (scene == "global_quantised" and knobs.get("bvhWidth") != 2)
    assert g["batch"][1] == -(-samples // g["batch"][0])
    assert p["bytesPerSample"] == 48 + 16 + 16 + (4 if scene == "two_level" else 0)


# ---------------------------------------------------------------- the reference against itself, cube scene
W, H, INDEX, JITTER = 61, 37, 3, (0.25, -0.125)
# Largest distance, in pixels, between (px + 0.5 + jitter) and the float64 re-projection of the reference's own float32 hit point o + d * t on this
# scene, measured on the CPU by this test (it prints the figure): 1.104e-4. The bound below is four times that.
REPROJECTION_MEASURED = 1.104e-4
REPROJECTION_BOUND = 4 * REPROJECTION_MEASURED


@pytest.fixture(scope="module")
def cube(luts):
    from oracle.binding import Oracle
    sc, cb = G.cube_case(luts, W, H, INDEX, JITTER)
    o = Oracle(sc)
    verts = G.unpacked_vertices(sc)
    tr = G.trace(sc, o, cb, W, H)
    planes = G.gbuffer(sc, o, cb, W, H, verts, tr)
    o.close()
    return sc, cb, verts, tr, planes


def test_reference_hit_flags_and_miss_values(cube):
    sc, cb, verts, tr, planes = cube
    depth, ids = planes[S.GB_DEPTH], planes[S.GB_IDS]
    hit = (ids[..., 3] & S.GB_FLAG_HIT) != 0
    assert np.array_equal(hit, depth[..., 0] < np.float32(1e10)) and np.array_equal(hit, tr["hit"])
    assert 200 < hit.sum() < W * H - 200                      # the cube covers part of the frame: both branches are exercised
    miss = ~hit
    for k in (S.GB_ALBEDO, S.GB_NORMAL, S.GB_GEO_NORMAL, S.GB_EMISSIVE):
        assert not planes[k][miss].any()
    assert np.array_equal(depth[miss], np.broadcast_to(np.array([1e10, 1e10, 0, 0], np.float32), (miss.sum(), 4)))
    assert np.array_equal(ids[miss], np.broadcast_to(np.array([0xFFFFFFFF] * 3 + [0], np.uint32), (miss.sum(), 4)))
    assert (planes[S.GB_EMISSIVE][hit][:, 3] == 1).all() and (planes[S.GB_NORMAL][hit][:, 3] >= np.float32(0.04)).all()


def test_reference_geometric_normal(cube):
    sc, cb, verts, tr, planes = cube
    ids = planes[S.GB_IDS]
    ys, xs = np.nonzero(ids[..., 3] & S.GB_FLAG_HIT)
    ng = planes[S.GB_GEO_NORMAL][ys, xs, :3]
    # unit length to 4 ulp of 1.0 (float32 ulp at 1 = 2^-23)
    length = np.sqrt((ng.astype(np.float64) ** 2).sum(1))
    assert np.abs(length - 1.0).max() <= 4 * 2.0 ** -23
    d = tr["d"][ys, xs].astype(np.float64)
    for i in range(len(ys)):
        p = G.world_triangle(sc, verts, ids[ys[i], xs[i], 0], ids[ys[i], xs[i], 1])
        face = np.cross(p[1] - p[0], p[2] - p[0]); face /= np.linalg.norm(face)
        # quantised vertex normals of a flat mesh sit well inside 0.99; a missing or transposed transform does not
        assert ng[i].astype(np.float64) @ face >= 0.99, (ys[i], xs[i])
        front = bool(ids[ys[i], xs[i], 3] & S.GB_FLAG_FRONT_FACE)
        assert front == (ng[i].astype(np.float64) @ d[i] < 0) and front == (face @ d[i] < 0)
    # no normal map, front-facing: the shading normal is the geometric one, bit for bit
    front = (ids[ys, xs, 3] & S.GB_FLAG_FRONT_FACE) != 0
    assert front.any()
    n = planes[S.GB_NORMAL][ys, xs, :3]
    assert np.array_equal(n[front].view(np.uint32), ng[front].view(np.uint32))


def test_reference_reprojection(cube):
    sc, cb, verts, tr, planes = cube
    ids, depth = planes[S.GB_IDS], planes[S.GB_DEPTH]
    ys, xs = np.nonzero(ids[..., 3] & S.GB_FLAG_HIT)
    o = tr["o"].astype(np.float32)
    wp = (o + tr["d"][ys, xs] * depth[ys, xs, 0:1]).astype(np.float64)              # the reference's float32 hit point
    m = np.asarray(cb["m_View"]["m_MatWorldToClipNoOffset"], np.float64)
    clip = np.concatenate([wp, np.ones((len(wp), 1))], 1) @ m
    wx = (clip[:, 0] / clip[:, 3] * 0.5 + 0.5) * W
    wy = (0.5 - clip[:, 1] / clip[:, 3] * 0.5) * H
    dev = np.hypot(wx - (xs + 0.5 + JITTER[0]), wy - (ys + 0.5 + JITTER[1])).max()
    print(f"largest re-projection deviation of the reference on the cube scene: {dev:.3e} px")
    assert dev <= REPROJECTION_BOUND
    # viewDepth is that product's w, in float32, to a few ulp
    assert np.abs(depth[ys, xs, 1].astype(np.float64) / clip[:, 3] - 1.0).max() < 1e-6
