"""Structure of the acceleration structures the kernels actually walk, read back with hrpt_selftest_read_bvh and checked by the validator of
tests/bvh_reference.py: every builder, rebuilds and refits, the two-level structure, every build variant the code reads from the environment,
the Morton-bit fallback -- and, independently of the validator, one ray per triangle that must find its triangle."""
import numpy as np
import pytest

from hobbyrenderer_amd import native, scenes, structs as S

import bvh_reference as R
import bvh_scenes as B
from scene_helpers import random_soup

pytestmark = pytest.mark.gpu

BUILDERS = {"host": S.BVH_BUILDER_HOST_SAH, "lbvh": S.BVH_BUILDER_GPU_LBVH, "ploc": S.BVH_BUILDER_GPU_PLOC}


def check_capacities(d):
    """k_emit4 writes nodes4[index] unchecked and the last record of the nodesQ buffer is the leaf-area accumulator: both need room."""
    if d["nodes4Capacity"]:
        assert d["node4Count"] <= d["nodes4Capacity"], (d["node4Count"], d["nodes4Capacity"])
    if d["hasNodesQ"]:
        assert d["node4Count"] < d["nodesQCapacity"], (d["node4Count"], d["nodesQCapacity"])


def check_flat_context(ctx, sc, max_leaf=2):
    bi = ctx.build_info()
    d = ctx.read_bvh()
    assert d["structure"] == S.ACCEL_FLAT and bi.structure == S.ACCEL_FLAT
    assert (d["nodeCount"], d["node4Count"], d["triangleCount"]) == (bi.nodeCount, bi.node4Count, bi.triangleCount)
    check_capacities(d)
    host = (bi.usedBuilder & 0xff) == S.BVH_BUILDER_HOST_SAH
    rep = R.validate_flat(d, sc, builder="host" if host else "gpu", max_leaf=4 if host else max_leaf)
    print(f"builder {bi.usedBuilder:#x} tris {bi.triangleCount} nodes {bi.nodeCount}/{bi.node4Count} cap {d['nodes4Capacity']}/{d['nodesQCapacity']} "
          f"mortonBits {bi.mortonBits} {rep.stats}")
    assert not rep, str(rep)
    assert ctx.selftest_bvh() == 0
    return d, bi, rep


def sorted_records(d):
    order = np.lexsort((d["triangles"]["prim"], d["triangles"]["inst"]))
    return [d[k][order].tobytes() if d[k] is not None else None for k in ("triangles", "attributes", "tangents")]


def small_scenes(luts):
    out = {"cornell": scenes.cornell_scene(luts), "n8": B.triangle_scene(luts, B.random_triangles(8, 108)),
           "n9": B.triangle_scene(luts, B.random_triangles(9, 109)), "cubes": B.coincident_cubes(luts, 12),
           "soup": random_soup(luts, 600, 2, blend_fraction=0.3, mask_fraction=0.2, textured=True), "sponza_reduced": scenes.sponza_class_scene(luts, 0.25, 8)}
    for k, v in B.degenerate_sets().items():
        out[k] = B.triangle_scene(luts, v)
    return out


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_every_builder_on_the_small_scenes(luts, builder):
    for name, sc in small_scenes(luts).items():
        ctx = native.PathTracerContext(0)
        try:
            ctx.set_bvh_builder(BUILDERS[builder])
            ctx.upload_scene(sc)
            print(name, end=" ")
            d, bi, _ = check_flat_context(ctx, sc)
            if builder != "host":       # all triangles, not only the visible ones: the records of both builders are the same bits
                assert sorted_records(d) == sorted_records(native.host_build_bvh(sc)), name
        finally:
            ctx.close()


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("detail", [1.0, 3.4], ids=["101k", "1.17M"])
def test_every_builder_on_the_large_scenes(luts, builder, detail):
    sc = scenes.sponza_class_scene(luts, detail, 8)
    ctx = native.PathTracerContext(0)
    try:
        ctx.set_bvh_builder(BUILDERS[builder])
        ctx.upload_scene(sc)
        d, bi, _ = check_flat_context(ctx, sc)
        assert bi.triangleCount > (1000000 if detail > 3 else 100000)
        if builder != "host":
            assert (bi.usedBuilder & 0xff) != S.BVH_BUILDER_HOST_SAH
            assert sorted_records(d) == sorted_records(native.host_build_bvh(sc))
    finally:
        ctx.close()


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_after_rebuild_refit_and_material_change(luts, builder):
    sc = B.instanced_scene(luts, 60, detail=8)
    rng = np.random.default_rng(4)
    ctx = native.PathTracerContext(0)
    try:
        ctx.set_bvh_builder(BUILDERS[builder])
        ctx.set_acceleration_structure(S.ACCEL_FLAT)
        ctx.upload_scene(sc)
        check_flat_context(ctx, sc)
        sc.instances["m_World"][:, 3, :3] += rng.uniform(-3, 3, (len(sc.instances), 3)).astype(np.float32)       # a large move: rebuild
        ctx.update_instances(sc.instances)
        check_flat_context(ctx, sc)
        sc.instances["m_World"][:, 3, :3] += rng.uniform(-0.05, 0.05, (len(sc.instances), 3)).astype(np.float32)  # a small one: refit
        ctx.refit_instances(sc.instances)
        _, bi, _ = check_flat_context(ctx, sc)
        if builder != "host":
            assert bi.usedBuilder & S.BVH_BUILDER_REFITTED, hex(bi.usedBuilder)
        sc.materials["m_AlphaMode"][0] = S.ALPHA_MODE_MASK          # structural: the opaque bit of every triangle of that material changes
        sc.materials["m_BaseColor"][0, 3] = 0.9
        ctx.update_materials(sc.materials[:1])
        d, _, _ = check_flat_context(ctx, sc)
        assert (d["triangles"]["flags"] & 1).min() == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt", ["1", "2"])
def test_forced_node_format(luts, fmt, monkeypatch):
    monkeypatch.setenv("HRPT_BVH_NODE_FORMAT", fmt)
    sc = scenes.sponza_class_scene(luts, 0.5, 8)
    ctx = native.PathTracerContext(0)
    try:
        ctx.set_bvh_builder(S.BVH_BUILDER_GPU_PLOC)
        ctx.upload_scene(sc)
        d, bi, _ = check_flat_context(ctx, sc)
        assert bi.nodeFormat == int(fmt) and d["hasNodesQ"] == 1
    finally:
        ctx.close()


VARIANTS = [(b, v) for b in ("lbvh", "ploc") for v in ("MAX_LEAF=3", "MAX_LEAF=4", "COLLAPSE=fixed", "CUBE_MORTON=1", "HOST_COLLAPSE=1")] + \
    [("ploc", "PLOC_RADIUS=1"), ("ploc", "PLOC_RADIUS=256")]            # (the radix tree has no search radius)
_default_trees = {}


def _default_tree(luts, builder):
    """The same scene through the same builder with no variant set: what a variant's tree is compared with."""
    if builder not in _default_trees:
        ctx = native.PathTracerContext(0)
        try:
            ctx.set_bvh_builder(BUILDERS[builder])
            ctx.upload_scene(scenes.sponza_class_scene(luts, 0.5, 8))
            _default_trees[builder] = ctx.read_bvh()
        finally:
            ctx.close()
    return _default_trees[builder]


@pytest.mark.parametrize("builder,variant", VARIANTS, ids=[f"{b}-{v}" for b, v in VARIANTS])
def test_build_variants_from_the_environment(luts, builder, variant, monkeypatch):
    default = _default_tree(luts, builder)              # (built before the variable is set)
    key, value = variant.split("=")
    monkeypatch.setenv("HRPT_GPU_PLOC_RADIUS" if key == "PLOC_RADIUS" else "HRPT_GPU_BVH_" + key, value)
    sc = scenes.sponza_class_scene(luts, 0.5, 8)
    ctx = native.PathTracerContext(0)
    try:
        ctx.set_bvh_builder(BUILDERS[builder])
        ctx.upload_scene(sc)
        d, bi, _ = check_flat_context(ctx, sc, max_leaf=int(value) if key == "MAX_LEAF" else 2)
        assert (bi.usedBuilder & 0xff) in (BUILDERS[builder], S.BVH_BUILDER_GPU_LBVH)
        # the variant really ran: its tree is not the default one
        if key == "MAX_LEAF":
            assert R.decode_leaf(d["nodes"]["left"][d["nodes"]["left"] < 0])[1].max() > 2
        if key in ("MAX_LEAF", "PLOC_RADIUS", "CUBE_MORTON"):        # another hierarchy
            assert d["nodes"].tobytes() != default["nodes"].tobytes()
        else:                                                         # the same 2-wide tree, collapsed differently
            assert d["nodes"].tobytes() == default["nodes"].tobytes()
            assert d["nodes4"].tobytes() != default["nodes4"].tobytes()
        if key == "HOST_COLLAPSE":
            assert d["nodes4Capacity"] == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("builder", ["lbvh", "ploc"])
@pytest.mark.parametrize("collapse", ["greedy", "fixed"])
def test_single_triangle_leaves_fit_the_node_buffer(luts, builder, collapse, monkeypatch):
    """HRPT_GPU_BVH_MAX_LEAF=1: up to 3 n / 4 four-wide nodes. The buffer is sized for it and the count is checked before the emission."""
    monkeypatch.setenv("HRPT_GPU_BVH_MAX_LEAF", "1")
    if collapse == "fixed":
        monkeypatch.setenv("HRPT_GPU_BVH_COLLAPSE", "fixed")
    for sc in (B.triangle_scene(luts, B.random_triangles(32, 7)), scenes.sponza_class_scene(luts, 0.5, 8)):
        ctx = native.PathTracerContext(0)
        try:
            ctx.set_bvh_builder(BUILDERS[builder])
            ctx.upload_scene(sc)
            d, bi, _ = check_flat_context(ctx, sc, max_leaf=1)
            assert (bi.usedBuilder & 0xff) != S.BVH_BUILDER_HOST_SAH and d["nodes4Capacity"] >= d["triangleCount"]
            assert d["node4Count"] <= d["nodes4Capacity"]
            ctx.refit_instances(sc.instances)
            check_flat_context(ctx, sc, max_leaf=1)
        finally:
            ctx.close()


def test_rebuild_that_exactly_fills_the_quantised_node_buffer(luts):
    """The last record of the nodesQ buffer is the leaf-area accumulator. An upload sizes the buffer to node4Count + node4Count / 8 + 64; a
    rebuild (hrpt_update_instances keeps the buffer) whose tree has EXACTLY that many nodes used to keep it, and the accumulator then lay on
    the last node. The host builder is deterministic: the pair is searched with hrpt_selftest_host_build (found at 396 moved instances)."""
    sc, far = B.huddled_instances(luts)
    first = native.host_build_bvh(sc)["node4Count"]
    capacity = first + first // 8 + 64
    base = sc.instances["m_World"].copy()
    for moved in range(1, len(far)):
        sc.instances["m_World"][moved - 1, 3, :3] = far[moved - 1]
        count = native.host_build_bvh(sc)["node4Count"]
        if count == capacity or count > capacity + 30:
            break
    assert count == capacity, f"no rebuild with {capacity} nodes found (last: {count} after {moved} moves)"
    after = sc.instances["m_World"].copy()
    ctx = native.PathTracerContext(0)
    try:
        ctx.set_bvh_builder(S.BVH_BUILDER_HOST_SAH)
        sc.instances["m_World"] = base
        ctx.upload_scene(sc)
        d, _, _ = check_flat_context(ctx, sc)
        assert d["node4Count"] == first and d["nodesQCapacity"] == capacity
        sc.instances["m_World"] = after
        ctx.update_instances(sc.instances)
        d, _, _ = check_flat_context(ctx, sc)           # (node4Count < nodesQCapacity, and the last node's quantised record is a node)
        assert d["node4Count"] == capacity
    finally:
        ctx.close()


def caterpillar_triangles():
    """Centroids whose 63-bit Morton codes (k_morton: 21 bits per axis over the centroid bounds, x most significant) are 0 (sixteen times:
    ties are split by position, four more levels), 1, 2, 4, ..., 2^62 and 2^63 - 1: the full-code radix tree is a caterpillar deeper than the
    traversal stacks allow. Grid coordinate g of an axis sits at g + 0.5 (0 at 0, the far corner at 2097151), so (c - lo) / ext * 2097151 truncates to g."""
    cent = [np.zeros(3)] * 16
    for k in range(63):
        c = np.zeros(3)
        c[2 - k % 3] = float(1 << (k // 3)) + 0.5
        cent.append(c)
    cent.append(np.full(3, 2097151.0))
    cent = np.array(cent, np.float32)
    h = np.float32(0.0625)
    offs = np.array([[-h, -h, -h], [h, -h, h], [-h, h, h]], np.float32)        # box centre = the centroid, exactly
    return cent[:, None, :] + offs[None]


def test_morton_bit_fallback(luts):
    from oracle.binding import Oracle
    tris = caterpillar_triangles()
    # the construction, checked on the host with the formula of k_morton
    lo, hi = tris.min(1), tris.max(1)
    c = np.float32(0.5) * lo + np.float32(0.5) * hi
    q = ((c - c.min(0)) / (c.max(0) - c.min(0)) * np.float32(2097151.0)).astype(np.uint32).astype(object)
    spread = lambda v: sum(((int(v) >> b) & 1) << (3 * b) for b in range(21))
    codes = sorted((spread(x) << 2) | (spread(y) << 1) | spread(z) for x, y, z in q)
    assert codes == [0] * 16 + [1 << k for k in range(63)] + [(1 << 63) - 1]
    sc = B.triangle_scene(luts, tris)
    ctx = native.PathTracerContext(0)
    try:
        ctx.set_bvh_builder(S.BVH_BUILDER_GPU_LBVH)
        ctx.upload_scene(sc)
        d, bi, rep = check_flat_context(ctx, sc)
        assert bi.mortonBits < 63 or bi.usedBuilder == S.BVH_BUILDER_HOST_SAH, (bi.mortonBits, bi.usedBuilder)      # the fallback really ran
        assert bi.maxDepth + 2 <= 64
        view, pos = scenes.planar_view(64, 36, position=(-3.0, 2.0, -6.0), yaw=0.4)
        ctx.resize(64, 36)
        ctx.render(scenes.fill_constants(view, pos, sc, 0, 3), accum_count=1)
        acc = ctx.read_accumulation()
        o = Oracle(sc)
        oacc, _ = o.render_accumulated(lambda i: scenes.fill_constants(view, pos, sc, i, 3), 64, 36, 1)
        o.close()
        assert np.array_equal(acc.view(np.uint32), oacc.view(np.uint32))
    finally:
        ctx.close()


def test_morton_bit_fallback_is_remembered(luts):
    """What the builder keeps between builds, on the fallback path: a rebuild starts at the Morton-bit budget that fitted last time and gives
    the same trees; a refit works on the hierarchy of that rebuild and, from unchanged transforms, gives the same 2-wide nodes (the fit is a
    min / max over the same boxes: order-independent)."""
    sc = B.triangle_scene(luts, caterpillar_triangles())
    ctx = native.PathTracerContext(0)
    try:
        ctx.set_bvh_builder(S.BVH_BUILDER_GPU_LBVH)
        ctx.upload_scene(sc)
        first, bi, _ = check_flat_context(ctx, sc)
        assert bi.usedBuilder == S.BVH_BUILDER_GPU_LBVH and bi.mortonBits < 63, (hex(bi.usedBuilder), bi.mortonBits)
        ctx.update_instances(sc.instances)
        again, bi2, _ = check_flat_context(ctx, sc)
        assert bi2.mortonBits == bi.mortonBits
        assert again["nodes"].tobytes() == first["nodes"].tobytes() and again["nodes4"].tobytes() == first["nodes4"].tobytes()
        ctx.refit_instances(sc.instances)
        refitted, bi3, _ = check_flat_context(ctx, sc)
        assert bi3.usedBuilder & S.BVH_BUILDER_REFITTED, hex(bi3.usedBuilder)
        assert refitted["nodes"].tobytes() == first["nodes"].tobytes()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ two-level structure
def check_two_level_context(ctx, sc, gpu_tree):
    bi = ctx.build_info()
    d = ctx.read_bvh()
    assert d["structure"] == S.ACCEL_TWO_LEVEL and bi.structure == S.ACCEL_TWO_LEVEL
    assert ((bi.usedBuilder & 0xff) != S.BVH_BUILDER_HOST_SAH) == gpu_tree, hex(bi.usedBuilder)
    rep = R.validate_two_level(d, sc, native.host_build_bvh(sc), gpu_instance_tree=gpu_tree)
    print(f"builder {bi.usedBuilder:#x} instances {d['instanceCount']} nodes {d['instanceNodeCount']}/{d['node4Count']} {rep.stats}")
    assert not rep, str(rep)
    assert rep.stats["two_level_worst_stack_occupancy"] <= rep.stats["two_level_stack_need"] <= 128      # (what the kernels' stacks hold at most)
    return d, bi


@pytest.mark.parametrize("tree", ["host", "gpu_ploc", "gpu_lbvh"])
def test_two_level_structure(luts, tree, monkeypatch):
    gpu = tree != "host"
    if gpu:
        monkeypatch.setenv("HRPT_TLAS_BUILDER", "gpu")
        monkeypatch.setenv("HRPT_TLAS_LBVH", "1" if tree == "gpu_lbvh" else "0")
    sc = B.instanced_scene(luts, 1100 if gpu else 70, detail=4)
    rng = np.random.default_rng(8)
    ctx = native.PathTracerContext(0)
    try:
        if not gpu:
            ctx.set_bvh_builder(S.BVH_BUILDER_HOST_SAH)
        ctx.set_acceleration_structure(S.ACCEL_TWO_LEVEL)
        ctx.upload_scene(sc)
        check_two_level_context(ctx, sc, gpu)
        sc.instances["m_World"][:, 3, :3] += rng.uniform(-4, 4, (len(sc.instances), 3)).astype(np.float32)
        ctx.update_instances(sc.instances)
        check_two_level_context(ctx, sc, gpu)
        sc.instances["m_World"][:, 3, :3] += rng.uniform(-0.05, 0.05, (len(sc.instances), 3)).astype(np.float32)
        ctx.refit_instances(sc.instances)
        _, bi = check_two_level_context(ctx, sc, gpu)
        if gpu:
            assert bi.usedBuilder & S.BVH_BUILDER_REFITTED, hex(bi.usedBuilder)
    finally:
        ctx.close()


def test_flattened_instance_comes_back_flat(luts):
    sc = B.instanced_scene(luts, 30, flattened=True)
    ctx = native.PathTracerContext(0)
    try:
        ctx.set_acceleration_structure(S.ACCEL_TWO_LEVEL)
        ctx.upload_scene(sc)
        check_flat_context(ctx, sc)
    finally:
        ctx.close()


def test_two_level_structure_with_tangents(luts):
    """A material that samples a normal map: the per-mesh tangent records are uploaded with the two-level structure. Eight instances of one
    cube (12 triangles: more than two leaves, so the mesh has a tree of its own), the host's instance tree."""
    b = scenes.SceneBuilder()
    cube = b.add_mesh(*scenes.generate_default_cube())
    normal_map = b.add_texture(np.full((4, 4, 4), (128, 128, 255, 255), np.uint8))
    mat = b.add_material(m_TextureFlags=S.TEXFLAG_NORMAL, m_NormalTextureIndex=normal_map)
    for i in range(8):
        b.add_instance(cube, mat, scenes._mat((1.0, 1.0 + 0.1 * i, 1.0), None, (2.5 * (i % 4), 0.0, 2.5 * (i // 4))))
    sc = b.finalize(luts)
    ctx = native.PathTracerContext(0)
    try:
        ctx.set_bvh_builder(S.BVH_BUILDER_HOST_SAH)
        ctx.set_acceleration_structure(S.ACCEL_TWO_LEVEL)
        ctx.upload_scene(sc)
        d, _ = check_two_level_context(ctx, sc, False)
        assert d["hasTangents"] and d["tangents"] is not None and len(d["tangents"]) == d["triangleCount"] == 12
        assert d["tangents"].tobytes() == native.host_build_bvh(sc, S.ACCEL_TWO_LEVEL)["tangents"].tobytes()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ every triangle can be found
def oracle_hits(o, rays):
    out = np.zeros(len(rays), S.RayHit)
    for i, r in enumerate(rays):
        ok, inst, prim, u, v, t, rng = o.trace_standard(r["origin"], r["direction"], float(r["tmin"]), float(r["tmax"]), int(r["rng"]))
        out[i] = (t, u, v, inst, prim, 1, rng, 0) if ok else (0, 0, 0, 0, 0, 0, rng, 0)
    return out


def same_hits(a, b):
    both = (a["hit"] != 0) & (b["hit"] != 0)
    same = (a["hit"] != 0) == (b["hit"] != 0)
    same &= a["rng"] == b["rng"]
    for k in ("t", "u", "v"):
        same &= ~both | (a[k].view(np.uint32) == b[k].view(np.uint32))
    for k in ("instance", "primitive"):
        same &= ~both | (a[k] == b[k])
    return same


@pytest.fixture(scope="module", params=["101k", "1.17M"])
def find_case(luts, request):
    """101 k triangles: a ray for every triangle; 1.17 M: for a fixed random subset of 100 000."""
    from oracle.binding import Oracle
    big = request.param == "1.17M"
    sc = scenes.sponza_class_scene(luts, 3.4 if big else 1.0, 8)
    sc.materials["m_AlphaMode"] = S.ALPHA_MODE_OPAQUE          # opaque materials: every hit is the closest triangle, no alpha test, no RNG draw
    sc.materials["m_TransmissionFactor"] = 0.0
    rays, owner, axial = B.find_rays(sc, subset=100000 if big else None, seed=1)
    axial = axial[:: max(1, len(axial) // 20000)]
    o = Oracle(sc)
    try:
        want, want_axial = oracle_hits(o, rays), oracle_hits(o, axial)
    finally:
        o.close()
    own = (want["hit"] != 0) & (want["instance"] == owner[:, 0]) & (want["primitive"] == owner[:, 1])
    print(f"{len(rays)} per-triangle rays, own triangle closest in the oracle for {own.mean():.4f}; {len(axial)} axis-parallel rays, {int((want_axial['hit'] != 0).sum())} hit")
    assert own.mean() >= 0.95                                   # the inputs cannot pass by missing
    assert (want_axial["hit"] != 0).mean() >= 0.95
    return sc, rays, axial, want, want_axial


@pytest.mark.parametrize("kernel", ["thread_per_ray_2wide", "persistent_fp32", "persistent_quantised"])
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_every_triangle_can_be_found(find_case, builder, kernel, monkeypatch):
    sc, rays, axial, want, want_axial = find_case
    monkeypatch.setenv("HRPT_BVH_NODE_FORMAT", "2" if kernel == "persistent_quantised" else "1")
    ctx = native.PathTracerContext(0)
    try:
        ctx.set_bvh_builder(BUILDERS[builder])
        ctx.upload_scene(sc)
        assert ctx.build_info().nodeFormat == (2 if kernel == "persistent_quantised" else 1)
        if kernel == "persistent_quantised":       # the decode that kernel evaluates, restated, on rays of both kinds over every node
            d = ctx.read_bvh()
            rng = np.random.default_rng(3)
            n = 3 if d["node4Count"] > 100000 else 12
            sample = np.concatenate([rays[rng.choice(len(rays), n, replace=False)], axial[rng.choice(len(axial), n, replace=False)]])
            child, _, _ = R.tree_arrays4(d["nodes4"])
            depth, _ = R.walk(R.Report(), "", child, [0])
            rep = R.Report()
            R.check_folded_decode(rep, d["nodes4"], d["nodesQ"], depth, sample)
            print(builder, rep.stats)
            assert not rep, str(rep)
            assert rep.stats["q_folded_hit_slots"] > 50
        for r, w, what in ((rays, want, "per-triangle"), (axial, want_axial, "axis-parallel")):
            got = ctx.trace_rays(r, thread_per_ray=kernel == "thread_per_ray_2wide")
            same = same_hits(got, w)
            assert same.all(), f"{what}: {int((~same).sum())} of {len(r)} rays differ from the oracle, first ray {int(np.flatnonzero(~same)[0])}"
    finally:
        ctx.close()
