"""Structure of the HOST-built acceleration structures, read back through hrpt_selftest_host_build (no context, no device) and checked by
the validator of tests/bvh_reference.py -- and the validator itself, which must report each hand-made corruption (twelve of the flat structure, six of the two-level one, the folded decode) by name."""
import ctypes as C
import os

import numpy as np
import pytest

from hobbyrenderer_amd import native, scenes, structs as S

import bvh_reference as R
import bvh_scenes as B
from scene_helpers import random_soup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = S.BVH_EMPTY_CHILD


def check_flat(scene, **kw):
    """Host build with the builder's own collapse and with collapse_bvh2_on_host: both valid, and the same tree."""
    own = native.host_build_bvh(scene)
    sep = native.host_build_bvh(scene, separate_collapse=True)
    for d in (own, sep):
        rep = R.validate_flat(d, scene, builder="host", **kw)
        assert not rep, str(rep)
    assert own["nodes4"].tobytes() == sep["nodes4"].tobytes() and own["maxDepth4"] == sep["maxDepth4"]
    return own


def test_cornell(luts):
    d = check_flat(scenes.cornell_scene(luts))
    assert d["triangleCount"] == 38 and d["nodeCount"] > 0 and d["node4Count"] > 0


@pytest.mark.parametrize("n", range(1, 10))
def test_few_triangles(luts, n):
    """Around the leaf size and the GPU builders' lower limit of 8: one leaf (rootLeaf) up to the first real trees."""
    d = check_flat(B.triangle_scene(luts, B.random_triangles(n, 100 + n)))
    assert d["triangleCount"] == n
    if n <= 2:
        assert d["nodeCount"] == 0 and d["node4Count"] == 0 and d["rootLeaf"] == ~(n - 1)


def test_empty_scene(luts):
    sc = B.empty_scene(luts)
    d = check_flat(sc)
    assert (d["triangleCount"], d["nodeCount"], d["node4Count"], d["rootLeaf"]) == (0, 0, 0, 0)
    t = native.host_build_bvh(sc, S.ACCEL_TWO_LEVEL)
    assert (t["triangleCount"], t["node4Count"], t["instanceCount"]) == (0, 0, 0)


def test_coincident_cubes(luts):
    check_flat(B.coincident_cubes(luts, 12))


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_soup(luts, seed):
    check_flat(random_soup(luts, 150 * seed * seed, seed, blend_fraction=0.3 if seed & 1 else 0.0, mask_fraction=0.2, textured=seed == 2))


@pytest.mark.parametrize("name", ["zero_area", "planar", "same_centroid", "huge_and_tiny", "near_1e6"])
def test_degenerate_sets(luts, name):
    check_flat(B.triangle_scene(luts, B.degenerate_sets()[name]))


def test_reduced_sponza_class_scene(luts):
    d = check_flat(scenes.sponza_class_scene(luts, 0.25, 8))
    assert d["hasTangents"] == 1 and d["triangleCount"] > 5000


def test_sponza_class_scene_full_size(luts):
    """The 101 k-triangle scene: the parallel build (ranges above 8192 primitives are split over threads and spliced) against the same rules."""
    d = check_flat(scenes.sponza_class_scene(luts, 1.0, 8))
    assert d["triangleCount"] > 100000


def test_two_level_instanced_scene(luts):
    """Instance tree + mesh trees + instance records, with a mirrored (negative determinant) instance."""
    sc = B.instanced_scene(luts, 40, mirrored=True)
    assert np.linalg.det(sc.instances["m_World"][:, :3, :3].astype(np.float64)).min() < 0
    rep = R.validate_two_level(native.host_build_bvh(sc, S.ACCEL_TWO_LEVEL), sc, native.host_build_bvh(sc))
    assert not rep, str(rep)
    one = B.instanced_scene(luts, 1, mirrored=False)       # a single instance: no instance tree, rootLeaf names it
    d = native.host_build_bvh(one, S.ACCEL_TWO_LEVEL)
    assert d["instanceNodeCount"] == 0 and d["rootLeaf"] == ~0
    rep = R.validate_two_level(d, one, native.host_build_bvh(one))
    assert not rep, str(rep)


def _two_level_scenes(luts):
    out = {"cornell": scenes.cornell_scene(luts), "cubes": B.coincident_cubes(luts, 12), "soup": random_soup(luts, 300, 3, blend_fraction=0.3, mask_fraction=0.2),
           "sponza_reduced": scenes.sponza_class_scene(luts, 0.25, 8)}
    for n in range(1, 10):
        out[f"n{n}"] = B.triangle_scene(luts, B.random_triangles(n, 100 + n))
    for k, v in B.degenerate_sets().items():
        out[k] = B.triangle_scene(luts, v)
    return out


def test_two_level_on_the_flat_scenes(luts):
    """The two-level host build of every scene the flat tests use: mesh trees of one triangle up to the Sponza-class meshes, instance trees of
    one instance (rootLeaf), of 12 coincident instances and of 43 instances."""
    for name, sc in _two_level_scenes(luts).items():
        d = native.host_build_bvh(sc, S.ACCEL_TWO_LEVEL)
        rep = R.validate_two_level(d, sc, native.host_build_bvh(sc))
        assert not rep, f"{name}: {rep}"
        assert d["instanceCount"] == len(sc.instances), name


def test_two_level_refuses_a_flattened_instance(luts):
    """An instance flattened to a plane has no inverse: the two-level builder says so (hrpt_upload_scene then builds flat), the flat one holds it."""
    sc = B.instanced_scene(luts, 12, flattened=True)
    with pytest.raises(native.HrptError) as e:
        native.host_build_bvh(sc, S.ACCEL_TWO_LEVEL)
    assert e.value.code == -1 and "singular" in str(e.value)
    check_flat(sc)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_vertices_stay_refused(luts, bad):
    t = B.random_triangles(20, 9)
    t[7, 1, 2] = bad
    sc = B.triangle_scene(luts, t)
    for structure in (S.ACCEL_FLAT, S.ACCEL_TWO_LEVEL):
        with pytest.raises(native.HrptError) as e:
            native.host_build_bvh(sc, structure)
        assert e.value.code == -1 and "non-finite" in str(e.value)


def test_host_build_argument_checks(luts):
    sc = scenes.cornell_scene(luts)
    desc, keep = sc.desc()
    d = S.BvhDump()
    assert native.lib.hrpt_selftest_host_build(None, S.ACCEL_FLAT, 0, C.byref(d)) == -1
    assert native.lib.hrpt_selftest_host_build(C.byref(desc), S.ACCEL_AUTO, 0, C.byref(d)) == -1
    assert native.lib.hrpt_selftest_host_build(C.byref(desc), S.ACCEL_TWO_LEVEL, S.HOST_BUILD_SEPARATE_COLLAPSE, C.byref(d)) == -1
    assert native.lib.hrpt_selftest_read_bvh(None, C.byref(d)) == -1


# ------------------------------------------------------------------------------------------------ the validator under test
@pytest.fixture(scope="module")
def valid_dump(luts):
    sc = random_soup(luts, 400, 11, textured=True)
    d = native.host_build_bvh(sc)
    d["nodesQ"] = R.quantise_reference(d["nodes4"])
    d["hasNodesQ"] = 1
    rep = R.validate_flat(d, sc, builder="host")
    assert not rep, str(rep)
    return sc, d


def _copy(d):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def _slot(n4, leaf, skip=0):
    """(node, slot) of the skip-th leaf / inner reference of the 4-wide tree."""
    ch = n4["child"]
    m = (ch < 0) if leaf else ((ch >= 0) & (ch != EMPTY))
    node, slot = np.nonzero(m)
    return int(node[skip]), int(slot[skip])


def _set_box(n4, node, slot, mn, mx):
    for a, k in enumerate("xyz"):
        n4["min" + k][node, slot] = mn[a]; n4["max" + k][node, slot] = mx[a]


def c_leaf_dropped(d):
    n, s = _slot(d["nodes4"], True, 5)
    d["nodes4"]["child"][n, s] = EMPTY; _set_box(d["nodes4"], n, s, [1e30] * 3, [1e30] * 3)
    d["nodesQ"] = R.quantise_reference(d["nodes4"])
    return "n4_triangle_unreferenced"


def c_triangle_in_two_leaves(d):
    (n, s), (m, t) = _slot(d["nodes4"], True, 3), _slot(d["nodes4"], True, 9)
    for k in ("minx", "maxx", "miny", "maxy", "minz", "maxz", "child"):
        d["nodes4"][k][n, s] = d["nodes4"][k][m, t]
    d["nodesQ"] = R.quantise_reference(d["nodes4"])
    return "n4_triangle_in_two_leaves"


def c_orphan_node(d):
    d["nodes4"] = np.concatenate([d["nodes4"], d["nodes4"][-1:]])
    d["nodesQ"] = np.concatenate([d["nodesQ"], d["nodesQ"][-1:]])
    d["node4Count"] += 1
    return "n4_node_unreachable"


def c_cycle(d):
    n, s = _slot(d["nodes4"], False, 7)
    d["nodes4"]["child"][n, s] = 0
    d["nodesQ"]["child"][n, s] = 0
    return "n4_child_back_reference"


def c_plane_one_ulp_inward(d):
    n, s = _slot(d["nodes4"], False, 4)
    d["nodes4"]["miny"][n, s] = np.nextafter(d["nodes4"]["miny"][n, s], np.float32(np.inf))
    return "n4_box_not_containing"


def c_plane_one_ulp_inward_2wide(d):
    k = int(np.flatnonzero(d["nodes"]["right"] >= 0)[3])
    d["nodes"]["rmax"][k, 2] = np.nextafter(d["nodes"]["rmax"][k, 2], np.float32(-np.inf))
    return "n2_box_not_containing"


def c_leaf_pad_removed(d):
    n, s = _slot(d["nodes4"], True, 6)
    first, count = R.decode_leaf(d["nodes4"]["child"][n, s:s + 1])
    t = d["triangles"][int(first[0]):int(first[0] + count[0])]
    p = np.concatenate([t["p0"], t["p1"], t["p2"]])
    _set_box(d["nodes4"], n, s, p.min(0), p.max(0))       # still contains every vertex: hrpt_selftest_bvh would pass it
    d["nodesQ"] = R.quantise_reference(d["nodes4"])
    return "n4_leaf_pad"


def c_quantised_plane_one_step_inward(d):
    n, s = _slot(d["nodes4"], True, 2)
    d["nodesQ"]["loz"][n] += np.uint32(1 << (8 * s))
    return "q_plane_inside"


def c_quantised_child_mismatch(d):
    n, s = _slot(d["nodes4"], True, 8)
    d["nodesQ"]["child"][n, s] = d["nodesQ"]["child"][n, s] - 4          # the leaf one triangle further on
    return "q_child_mismatch"


def c_depth_too_small(d):
    d["maxDepth4"] -= 1
    return "depth4_too_small"


def c_depth2_too_small(d):
    d["maxDepth"] -= 2          # (the host builder reports the leaf depth, one above what the stacks need)
    return "depth2_too_small"


def c_swapped_prim(d):
    t = d["triangles"]
    i = int(np.flatnonzero((t["inst"][:-1] == t["inst"][1:]))[0])
    t["prim"][i], t["prim"][i + 1] = t["prim"][i + 1], t["prim"][i]
    return "tri_position"


CORRUPTIONS = [c_leaf_dropped, c_triangle_in_two_leaves, c_orphan_node, c_cycle, c_plane_one_ulp_inward, c_plane_one_ulp_inward_2wide,
               c_leaf_pad_removed, c_quantised_plane_one_step_inward, c_quantised_child_mismatch, c_depth_too_small, c_depth2_too_small,
               c_swapped_prim]


@pytest.mark.parametrize("corrupt", CORRUPTIONS, ids=lambda f: f.__name__[2:])
def test_validator_reports_each_corruption_by_name(valid_dump, corrupt):
    sc, d = valid_dump
    d = _copy(d)
    want = corrupt(d)
    rep = R.validate_flat(d, sc, builder="host")
    assert want in rep.names(), f"{corrupt.__name__}: expected {want}, got: {rep}"
    assert str(rep.violations[want][0]) in rep.violations[want][1] and "first" in rep.violations[want][1] or want.startswith("depth")


def test_validator_two_level_corruptions(luts):
    sc = B.instanced_scene(luts, 40)
    flat = native.host_build_bvh(sc)
    good = native.host_build_bvh(sc, S.ACCEL_TWO_LEVEL)

    def names(edit):
        d = _copy(good)
        edit(d)
        return R.validate_two_level(d, sc, flat).names()

    def drop_instance(d):
        n, s = np.argwhere(d["nodes4"]["child"][:d["instanceNodeCount"]] < 0)[3]
        d["nodes4"]["child"][n, s] = ~(5 << 2) if d["nodes4"]["child"][n, s] != ~(5 << 2) else ~(6 << 2)
    assert {"tlas_instance_unreferenced", "tlas_instance_in_two_leaves"} <= names(drop_instance)

    def shrink_instance_box(d):
        n, s = np.argwhere(d["nodes4"]["child"][:d["instanceNodeCount"]] < 0)[2]
        d["nodes4"]["maxx"][n, s] = np.nextafter(d["nodes4"]["maxx"][n, s], np.float32(-np.inf))
    assert "tlas_leaf_pad" in names(shrink_instance_box)

    def wrong_inverse(d):
        d["instances"]["inv"][4, 1, 1] *= np.float32(1.001)
    assert "inst_inverse" in names(wrong_inverse)

    def wrong_material(d):
        d["instances"]["material"][3] ^= 1
    assert "inst_material" in names(wrong_material)

    def wrong_slack(d):
        d["instances"]["boxEps"][7] *= np.float32(0.5)
    assert "inst_box_eps" in names(wrong_slack)

    def levels_too_small_for_the_stack(d):          # both level counts halved: the stack need computed from them no longer covers the trees
        d["maxDepth4Blas"] = 0; d["maxDepth4Tlas"] = 0; d["maxDepth4"] = 0
    assert "two_level_stack_need" in names(levels_too_small_for_the_stack)

    def blas_levels(d):
        d["maxDepth4Blas"] -= 1
        d["maxDepth4"] -= 1
    assert "depth4_blas_too_small" in names(blas_levels)

    def mesh_leaf_lost(d):
        n, s = np.argwhere(d["nodes4"]["child"][d["instanceNodeCount"]:] < 0)[4]
        d["nodes4"]["child"][d["instanceNodeCount"] + n, s] = EMPTY
    assert "blas_triangle_unreferenced" in names(mesh_leaf_lost)


def test_stack_occupancy_is_taken_from_the_tree(valid_dump):
    """The worst case the stacks are sized for, from the dumped nodes: a full 4-wide node leaves three entries, a path of them three each; a
    reported depth that is too small makes the plan's stack smaller than that."""
    sc, d = valid_dump
    child, _, _ = R.tree_arrays4(d["nodes4"])
    depth, _ = R.walk(R.Report(), "", child, [0])
    occ = R.worst_stack_occupancy(child, depth)
    assert 3 <= occ <= 3 * (int(depth.max()) + 1)
    assert R.validate_flat(d, sc).stats["n4_worst_stack_occupancy"] == occ
    e = _copy(d)
    e["maxDepth4"] = (occ - 3) // 3 - 1 if occ >= 6 else 0           # 3 * (maxDepth4 + 1) < occ
    if occ >= 6:
        assert "n4_stack_bound" in R.validate_flat(e, sc).names()


def _rays_for(sc, n, seed):
    rays, _, axial = B.find_rays(sc)
    rng = np.random.default_rng(seed)
    return np.concatenate([rays[rng.choice(len(rays), n, replace=False)], axial[rng.choice(len(axial), n, replace=False)]])


def test_folded_decode_of_the_quantised_nodes(luts):
    """inner_step's own decode of the 64-byte nodes (q * (s * inv) + (o * inv + noi)) restated in binary32, on per-triangle and axis-parallel
    rays over every node of a host-built tree with reference-quantised nodes; and the check's own sensitivity."""
    sc = scenes.sponza_class_scene(luts, 0.25, 8)
    d = native.host_build_bvh(sc)
    nq = R.quantise_reference(d["nodes4"])
    child, _, _ = R.tree_arrays4(d["nodes4"])
    depth, _ = R.walk(R.Report(), "", child, [0])
    rays = _rays_for(sc, 24, 2)
    rep = R.Report()
    R.check_folded_decode(rep, d["nodes4"], nq, depth, rays)
    assert not rep, str(rep)
    assert rep.stats["q_folded_hit_slots"] > 500 and rep.stats["q_folded_strict_far_violations"] == 0
    swapped = nq.copy()                                   # near and far words of an axis exchanged: every box turns inside out
    swapped["loy"], swapped["hiy"] = nq["hiy"], nq["loy"]
    rep = R.Report()
    R.check_folded_decode(rep, d["nodes4"], swapped, depth, rays)
    assert {"q_folded_near", "q_folded_far", "q_folded_rejects_hit"} <= rep.names(), str(rep)
    shifted = nq.copy()                                   # origin moved by a thousandth of the node: every near plane inside its box
    shifted["o"] = nq["o"] + np.float32(0.3) * np.stack([nq["sx"], nq["sy"], nq["sz"]], 1) * np.float32(254 * 1e-2)
    rep = R.Report()
    R.check_folded_decode(rep, d["nodes4"], shifted, depth, rays)
    assert "q_folded_near" in rep.names(), str(rep)
