"""The kernels' hits against geometry: hrpt_trace_rays (persistent and one-thread-per-ray kernels, both query kinds), the two node formats, the
three builders, the two-level structure, a refitted tree and the first-hit G-buffer (wf_extend<PRIMARY>, the megakernel's own walk) are judged
by tests/ray_reference.py -- float64 triple products with a derived error bound of the fp32 watertight test -- on the cases of
tests/ray_cases.py. The oracle plays no part here (tests/test_ray_geometry_cpu.py holds it to the same verdict). Besides the verdict every
variant must equal the persistent default kernel bit for bit. DESIGN.md "Hit definition: independent check"."""
import os
import re

import numpy as np
import pytest

from hobbyrenderer_amd import structs as S

import ray_cases as RC

pytestmark = pytest.mark.gpu

f32 = np.float32
FRAMES = list(RC.SOUP_FRAMES)
BUILDERS = [("host", S.BVH_BUILDER_HOST_SAH), ("lbvh", S.BVH_BUILDER_GPU_LBVH), ("ploc", S.BVH_BUILDER_GPU_PLOC)]


def _plan_constants():
    """kLdsBudget, kBlock, kExtendLdsStack and the LDS node stride, read from csrc/pt_wavefront_plan.h."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hobbyrenderer_amd", "csrc", "pt_wavefront_plan.h")).read()
    budget = re.search(r"kLdsBudget\s*=\s*(\d+)\s*\*\s*(\d+)", src)
    return dict(budget=int(budget.group(1)) * int(budget.group(2)), block=int(re.search(r"kBlock\s*=\s*(\d+)", src).group(1)),
                stack=int(re.search(r"kExtendLdsStack\s*=\s*(\d+)", src).group(1)), stride=int(re.search(r"define HRPT_LDS_NODE4_STRIDE (\d+)", src).group(1)))


def _tree_in_lds(bi):
    """pick_variant for the closest-hit class of hrpt_trace_rays (width 4, no extra bytes), from build_info() counts."""
    k = _plan_constants()
    need = 3 * bi.maxDepth4 + 3
    depth = 16 if need <= 16 else (32 if need <= 32 else 64)
    bvh = bi.node4Count * k["stride"] + bi.triangleCount * 48
    return bvh > 0 and min(depth, k["stack"]) * k["block"] * 4 + bvh <= k["budget"]


def _context(scene, builder=None, structure=None):
    from hobbyrenderer_amd.native import PathTracerContext
    ctx = PathTracerContext(0)
    try:
        if builder is not None:
            ctx.set_bvh_builder(builder)
        if structure is not None:
            ctx.set_acceleration_structure(structure)
        ctx.upload_scene(scene)
    except Exception:
        ctx.close()
        raise
    return ctx


def _judge(case, ctx, label, base=None, watertight=False, thread_per_ray=(False, True)):
    """Both query kinds through the persistent and the thread-per-ray kernel: the verdict, and bit equality with `base` (or with this call's
    persistent result). Returns that (closest, shadow) pair of records."""
    for tpr in thread_per_ray:
        name = f"{case.name} {label} {'thread-per-ray' if tpr else 'persistent'}"
        hits = ctx.trace_rays(case.rays, thread_per_ray=tpr)
        vis = ctx.trace_rays(case.rays, shadow=True, thread_per_ray=tpr)
        rep = case.table.judge_closest(hits)
        srep = case.table.judge_shadow(vis["t"], case.rays["tmax"])
        print(f"{name}: {rep.stats} vacuous {rep.vacuous_share:.4f} bounded {rep.bounded_share:.4f} headroom {rep.headroom}; "
              f"shadow {srep.stats} unjudged {srep.unjudged_share:.4f}")
        assert not rep, f"{name}: {rep}"
        assert not srep, f"{name}: {srep}"
        if watertight:
            assert hits["hit"].all(), f"{name}: {int((hits['hit'] == 0).sum())} rays leave the closed mesh, first {int(np.argmin(hits['hit']))}"
            assert (vis["t"] == 0).all(), f"{name}: {int((vis['t'] != 0).sum())} shadow rays leave the closed mesh, first {int(np.argmax(vis['t'] != 0))}"
        if base is None:
            base = (hits, vis)
        else:
            for kind, got, want in (("closest", hits, base[0]), ("shadow", vis, base[1])):
                diff = (got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1)).any(1)
                assert not diff.any(), f"{name} {kind}: {int(diff.sum())} records differ from the persistent default, first ray {int(np.argmax(diff))}"
    return base


def _soup_variants(case, size, monkeypatch):
    ctx = _context(case.scene)
    try:
        bi = ctx.build_info()
        assert bi.triangleCount == RC.SOUP_SIZES[size]
        assert _tree_in_lds(bi) == (size == "lds"), (bi.node4Count, bi.triangleCount, bi.maxDepth4)
        base = _judge(case, ctx, "default")
    finally:
        ctx.close()
    if size != "global":
        return
    for fmt in (1, 2):
        monkeypatch.setenv("HRPT_BVH_NODE_FORMAT", str(fmt))
        ctx = _context(case.scene)
        try:
            assert ctx.build_info().nodeFormat == fmt
            _judge(case, ctx, f"node format {fmt}", base, thread_per_ray=(False,))
        finally:
            ctx.close()
    monkeypatch.delenv("HRPT_BVH_NODE_FORMAT")
    for name, builder in BUILDERS:
        ctx = _context(case.scene, builder=builder)
        try:
            assert ctx.build_info().usedBuilder == builder
            _judge(case, ctx, name, base)
        finally:
            ctx.close()


@pytest.mark.parametrize("size", list(RC.SOUP_SIZES))
@pytest.mark.parametrize("frame", FRAMES)
def test_soups_at_scale_and_offset(luts, frame, size, monkeypatch):
    _soup_variants(RC.soup_case(luts, size, frame), size, monkeypatch)


@pytest.mark.parametrize("size", list(RC.SOUP_SIZES))
@pytest.mark.parametrize("frame", FRAMES)
def test_edge_and_vertex_rays(luts, frame, size, monkeypatch):
    _soup_variants(RC.edge_case(luts, size, frame), size, monkeypatch)


@pytest.mark.parametrize("variant", ["flat", "two-level", "refitted", "offset1e3", "offset1e3-two-level"])
def test_closed_mesh_is_watertight(luts, variant):
    """Every closest-hit query from inside hits, every visibility query returns exactly 0: no tolerance involved."""
    offset = 1e3 if variant.startswith("offset1e3") else 0.0
    flat_case = RC.closed_case(luts, offset)
    ctx = _context(flat_case.scene)
    try:
        assert ctx.build_info().structure == S.ACCEL_FLAT
        base = _judge(flat_case, ctx, "flat", watertight=True)
    finally:
        ctx.close()
    if variant.endswith("two-level"):
        ctx = _context(flat_case.scene, structure=S.ACCEL_TWO_LEVEL)
        try:
            assert ctx.build_info().structure == S.ACCEL_TWO_LEVEL
            _judge(flat_case, ctx, "two-level", base, watertight=True)
        finally:
            ctx.close()
    if variant == "refitted":
        moved = RC.closed_case(luts, 0.0, moved=True)
        for name, builder in BUILDERS[1:]:
            ctx = _context(flat_case.scene, builder=builder)
            try:
                ctx.refit_instances(moved.scene.instances)
                assert ctx.build_info().usedBuilder == (builder | S.BVH_BUILDER_REFITTED)
                refit = _judge(moved, ctx, f"refitted {name}", watertight=True)
            finally:
                ctx.close()
            ctx = _context(moved.scene)                       # the refitted tree reports what a fresh build of the moved scene reports
            try:
                _judge(moved, ctx, "fresh build of the moved scene", refit, watertight=True, thread_per_ray=(False,))
            finally:
                ctx.close()


@pytest.mark.parametrize("path,flags", [("wavefront", S.FRAME_WAVEFRONT), ("megakernel", S.FRAME_MEGAKERNEL)])
def test_gbuffer_from_inside_the_closed_mesh(luts, path, flags):
    """64 x 36 primary rays from inside the mesh: every pixel carries HRPT_GB_FLAG_HIT and (instance, primitive, t, u, v) passes the closest-hit
    verdict for the pixel's ray. This reaches wf_extend<PRIMARY> and the megakernel's own walk, which hrpt_trace_rays does not."""
    sc, cb, case = RC.gbuffer_case(luts)
    ctx = _context(sc)
    try:
        ctx.resize(64, 36)
        ctx.render_gbuffer(cb, planes=(1 << S.GB_IDS) | (1 << S.GB_DEPTH), flags=flags)
        ids, depth = ctx.read_gbuffer(S.GB_IDS).reshape(-1, 4), ctx.read_gbuffer(S.GB_DEPTH).reshape(-1, 4)
        traced = ctx.trace_rays(case.rays)
    finally:
        ctx.close()
    assert ((ids[:, 3] & S.GB_FLAG_HIT) != 0).all(), f"{path}: {int(((ids[:, 3] & S.GB_FLAG_HIT) == 0).sum())} pixels see through the closed mesh"
    hits = np.zeros(len(ids), S.RayHit)
    hits["hit"] = 1
    hits["instance"], hits["primitive"] = ids[:, 0], ids[:, 1]
    hits["t"], hits["u"], hits["v"] = depth[:, 0], depth[:, 2], depth[:, 3]
    rep = case.table.judge_closest(hits)
    print(f"{case.name} {path}: {rep.stats} vacuous {rep.vacuous_share:.4f} headroom {rep.headroom}")
    assert not rep, f"{path}: {rep}"
    for f in ("instance", "primitive", "t", "u", "v"):        # and the same records as the stand-alone query on the same rays
        assert np.array_equal(hits[f].view(np.uint32), traced[f].view(np.uint32)), (path, f)


def test_axis_parallel_and_denormal_directions(luts):
    case = RC.axis_case(luts)
    ctx = _context(case.scene)
    try:
        _judge(case, ctx, "default")
    finally:
        ctx.close()


@pytest.mark.parametrize("which", ["planar", "zero_area"])
def test_degenerate_sets(luts, which):
    """A ray in (or parallel to) a triangle's plane misses it; a triangle of zero area is never hit."""
    case = RC.degenerate_case(luts, which)
    ctx = _context(case.scene)
    try:
        hits, _ = _judge(case, ctx, "default")
    finally:
        ctx.close()
    assert (hits["hit"] == 0).all() if which == "planar" else (hits["hit"] != 0).sum() > 100


def test_interval_ends_are_exact(luts):
    """Hits at t == 2.0 exactly (tests/test_ray_geometry_cpu.py checks the construction in rational arithmetic): tmax = 2 misses, the next float
    hits; tmin = 2 misses, the float before hits; tmin >= tmax misses; tmax = +inf behaves as a large tmax."""
    rays, want, label = RC.interval_rays()
    ctx = _context(RC.interval_scene(luts))
    try:
        for tpr in (False, True):
            got = ctx.trace_rays(rays, thread_per_ray=tpr)
            bad = np.flatnonzero((got["hit"] != 0) != want)
            assert len(bad) == 0, (tpr, [label[i] for i in bad])
            assert (got["t"][want] == 2.0).all() and (got["primitive"][want] % 2 == 0).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("size", list(RC.SOUP_SIZES))
def test_non_finite_and_zero_rays_miss(luts, size):
    """NaN or +-inf in origin or direction, direction (0, 0, 0): hit == 0 and visibility 1.0, among ordinary rays of the same launch. A ray with a
    non-finite component is not walked at all (pt_traverse.h all_finite: with 1 / inf == 0 the far-away box of an unused node slot would pass the
    slab test, and its child reference is no node -- this test hung over the tree in global memory before the kernels checked). A zero
    direction is walked: traversal_rcp caps 1 / 0 at 1e20, unused slots are 1e50 away, and the walk only follows child references of an
    acyclic tree with stacks sized for a ray that finds every child of every node."""
    case = RC.soup_case(luts, size, "unit")
    bad = RC.nonfinite_rays()
    rays = np.concatenate([case.rays[:200], bad, case.rays[200:400]])
    ctx = _context(case.scene)
    try:
        for tpr in (False, True):
            hits, vis = ctx.trace_rays(rays, thread_per_ray=tpr), ctx.trace_rays(rays, shadow=True, thread_per_ray=tpr)
            sel = slice(200, 200 + len(bad))
            assert (hits["hit"][sel] == 0).all(), (tpr, np.flatnonzero(hits["hit"][sel]))
            assert (vis["t"][sel] == 1.0).all(), (tpr, np.flatnonzero(vis["t"][sel] != 1.0))
            alone = ctx.trace_rays(case.rays[:400], thread_per_ray=tpr)
            assert np.array_equal(np.concatenate([hits[:200], hits[200 + len(bad):]]).view(np.uint8), alone.view(np.uint8))
    finally:
        ctx.close()
