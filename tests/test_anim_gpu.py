"""Keyframe animation on the device (hrpt_animate): the kernels against the host executor, as bytes, on every case
of tests/anim_cases.py; the commit against a second context that receives the host executor's instances through hrpt_update_instances /
hrpt_refit_instances (images on both kernel paths, ray queries, the read-back structure, motion vectors) and against the oracle on a
scene built with those matrices; the joint palette and morph weights handed to hrpt_update_vertices_skinned without leaving the device;
and the error paths. tests/test_anim_cpu.py ties the host executor to the NumPy statement and to float64."""
import copy

import numpy as np
import pytest

from hobbyrenderer_amd import native, scenes, structs as S
import anim_cases as K
import deform_cases as D
import skin_cases as SK
from test_bvh_structure_gpu import sorted_records
from test_deform_gpu import _context, _u32
from test_parity_gpu import _assert_parity
from test_ray_queries_gpu import _rays
from test_skin_gpu import OnDevice, _same_products
from test_update_instances_gpu import _render_pair

pytestmark = pytest.mark.gpu
W, H = 64, 36


def _same(got, want):
    return np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes()


# ---------------------------------------------------------------- 1. the kernels against the host executor
@pytest.fixture(scope="module")
def ctx():
    c = _context()
    yield c
    c.close()


@pytest.mark.parametrize("name", list(K.cases()))
def test_kernels_equal_the_host_executor(ctx, name):
    """No scene: HRPT_ANIMATE_NO_COMMIT evaluates node worlds, palette and weights. Every time vector of the case in sequence on one device
    copy: the result is a function of the times alone."""
    case = K.cases()[name]
    anim = native.Animation(**case["tables"])
    try:
        for times in case["times"] + case["times"][:1]:
            anim.set_times(times)
            ctx.animate(anim, S.ANIMATE_NO_COMMIT)
            palette, weights, worlds = ctx.read_animation(anim)
            _, want_palette, want_weights, want_worlds = anim.evaluate_host()
            bad = np.nonzero((worlds != want_worlds).any((1, 2)))[0]
            assert _same(worlds, want_worlds), (name, times, len(bad), bad[:8])
            assert _same(palette, want_palette) and _same(weights, want_weights), (name, times)
        pointers = ctx.animation_device(anim)
        assert [p is not None for p in pointers] == [anim.joint_count > 0, anim.morph_weight_count > 0, anim.node_count > 0]
        assert all(p is None or p % 256 == 0 for p in pointers)
    finally:
        ctx.release_animation(anim)
        anim.close()


# ---------------------------------------------------------------- 2. the commit against hrpt_update_instances with the host executor's matrices
def _cube_scene(luts, worlds):
    b = scenes.SceneBuilder()
    mesh, mat = b.add_mesh(*scenes.generate_default_cube()), b.add_material()
    for w in worlds:
        b.add_instance(mesh, mat, w)
    return b.finalize(luts)


def _family():
    """Seven nodes: an animated root, two children, three grandchildren (one of them animated itself), and a static sibling of the root;
    one cube each, and two cubes no node lists."""
    b = K.Builder(31)
    small = lambda: (b.rng.uniform(-1.2, 1.2, 3).astype(np.float32), K.random_quaternion(b.rng), b.rng.uniform(0.45, 0.7, 3).astype(np.float32))
    root = b.node(trs=small(), instances=1)
    a, c = b.node(root, trs=small(), instances=1), b.node(root, trs=small(), instances=1)
    a1, a2, c1 = b.node(a, trs=small(), instances=1), b.node(a, trs=small(), instances=1), b.node(c, trs=small(), instances=1)
    b.node(trs=small(), instances=1)
    b.channel(S.ANIM_PATH_ROTATION, b.sampler(S.ANIM_SLERP, [0, 1, 2], K.key_values(b.rng, S.ANIM_PATH_ROTATION, 3)), [root])
    b.channel(S.ANIM_PATH_TRANSLATION, b.sampler(S.ANIM_CATMULLROM, [0, 0.5, 1.5, 2], 0.8 * K.key_values(b.rng, S.ANIM_PATH_TRANSLATION, 4)), [root, a2])
    tables, count = b.tables()
    assert count == 9
    return tables, [[0.3], [1.1], [1.85]]


def _family_scene(luts, tables):
    worlds = [scenes._mat(scale=(0.5, 0.5, 0.5), translate=(3.0 - k, -1.5, 1.0)) for k in range(9)]      # the unlisted cubes keep these
    for n in tables["nodes"]:
        worlds[tables["node_instances"][n["firstInstance"]]] = n["baseWorld"]
    return _cube_scene(luts, worlds)


def _same_structure(a, b, what):
    """hrpt_selftest_read_bvh of both contexts: the flat structure's records in a canonical order (a GPU build's node order is not fixed);
    the two-level structure's header and instance records, and every array where the host built all of it."""
    da, db = a.read_bvh(), b.read_bvh()
    assert da["structure"] == db["structure"], what
    if da["structure"] == S.ACCEL_FLAT:
        assert sorted_records(da) == sorted_records(db), what
        return
    host_built = (a.build_info().usedBuilder & 0xff) == S.BVH_BUILDER_HOST_SAH
    for k, v in da.items():
        if isinstance(v, np.ndarray):
            assert (not host_built and k != "instances") or _same(v, db[k]), (what, k)
        elif v is not None and k != "sahCost":
            assert v == db[k], (what, k)


def _same_scene_products(a, b, cb, view, what):
    for flags in (S.FRAME_DEFAULT, S.FRAME_MEGAKERNEL):
        images = []
        for c in (a, b):
            c.render(cb, accum_count=2, flags=flags)
            images.append(c.read_accumulation())
        assert _same(_u32(images[0]), _u32(images[1])), (what, flags)
    rays = _rays(np.random.default_rng(17), 2000, extent=4.0)
    assert _same(a.trace_rays(rays), b.trace_rays(rays)), what
    _same_structure(a, b, what)
    motion = []
    for c in (a, b):
        c.render_motion_vectors(cb, view)
        motion.append(c.read_motion_vectors())
    assert _same(_u32(motion[0]), _u32(motion[1])), what
    return motion[0]


@pytest.mark.parametrize("refit", [False, True], ids=["rebuild", "refit"])
@pytest.mark.parametrize("builder", ["host", "lbvh"])
@pytest.mark.parametrize("structure", [S.ACCEL_FLAT, S.ACCEL_TWO_LEVEL], ids=["flat", "two-level"])
def test_commit_equals_update_instances_with_the_host_matrices(luts, structure, builder, refit):
    tables, sequence = _family()
    sc = _family_scene(luts, tables)
    view, pos = scenes.planar_view(W, H, position=(0.0, 1.0, -11.0))
    cb = scenes.fill_constants(view, pos, sc, 0, 3)
    anim = native.Animation(**tables)
    a, b = _context(builder, structure), _context(builder, structure)
    try:
        for c in (a, b):
            c.upload_scene(sc)
            c.resize(W, H)
        assert a.build_info().structure == structure
        now = sc.instances.copy()
        for step, times in enumerate(sequence):
            anim.set_times(times)
            a.animate(anim, S.ANIMATE_REFIT if refit else 0)
            before, (now, _, _, worlds) = now, anim.evaluate_host(now)
            (b.refit_instances if refit else b.update_instances)(now)
            assert a.build_info().usedBuilder == b.build_info().usedBuilder and a.build_info().structure == b.build_info().structure
            motion = _same_scene_products(a, b, cb, view, (step, times))
            # m_PrevWorld is last frame's world everywhere; an instance no composed node lists has prev == world
            assert _same(now["m_PrevWorld"], before["m_World"]) and not _same(now["m_World"], before["m_World"])
            listed = tables["node_instances"][[n["firstInstance"] for n in tables["nodes"][:6]]]
            still = np.setdiff1d(np.arange(9), listed)
            assert len(still) == 3 and _same(now["m_World"][still], sc.instances["m_World"][still])
            assert np.abs(motion[..., :2]).max() > 0.5
            if step == 1:                                                 # ... and both are the scene built with those matrices
                fresh = copy.copy(sc)
                fresh.instances = now
                _assert_parity(*_render_pair(a, fresh, view, pos, W, H, 2, 3, S.FRAME_DEFAULT))
                a.resize(W, H)
    finally:
        a.close(); b.close(); anim.close()


def test_commit_of_a_wide_hierarchy(luts):
    """The hierarchy case: 300 children in one depth group, 340-odd instance records in the closed range, among them static and unlisted
    ones: more than one workgroup in the compose and the emit kernels, committed and compared as above."""
    case = K.cases()["hierarchy"]
    inst = K.scene_instances(case)
    sc = _cube_scene(luts, inst["m_World"])
    anim = native.Animation(**case["tables"])
    a, b = _context("lbvh"), _context("lbvh")
    try:
        for c in (a, b):
            c.upload_scene(sc)
        now = sc.instances.copy()
        for times in case["times"]:
            anim.set_times(times)
            a.animate(anim)
            now = anim.evaluate_host(now)[0]
            b.update_instances(now)
            _same_structure(a, b, times)
        rays = _rays(np.random.default_rng(18), 2000, extent=4.0)
        assert _same(a.trace_rays(rays), b.trace_rays(rays))
        b.update_instances(sc.instances[5:9], 5)                         # somebody else writes instances: the device copy is refreshed
        a.update_instances(sc.instances[5:9], 5)
        now[5:9] = sc.instances[5:9]
        anim.set_times(case["times"][0])
        a.animate(anim)
        b.update_instances(anim.evaluate_host(now)[0])
        _same_structure(a, b, "after an update from outside")
    finally:
        a.close(); b.close(); anim.close()


# ---------------------------------------------------------------- 3. palette and weights stay on the device: animate -> skin -> quantise -> rebuild
def _skeleton(joint_count, seed):
    """A gentle skeleton: joints four to a parent under a static armature, inverse bind matrices of the rest pose (palette = identity at
    rest), every third joint turning by a few degrees, and two morph-weight slots."""
    b = K.Builder(seed)
    rng = b.rng
    b.morph_weight_count = 2

    def near_identity():
        q = np.array([*rng.uniform(-0.03, 0.03, 3), 1.0])
        return rng.uniform(-0.05, 0.05, 3).astype(np.float32), (q / np.linalg.norm(q)).astype(np.float32), rng.uniform(0.98, 1.02, 3).astype(np.float32)

    armature = b.node(trs=near_identity())
    nodes = []
    for j in range(joint_count):
        nodes.append(b.node(armature if j == 0 else nodes[(j - 1) // 4], trs=near_identity()))
        b.joint(nodes[-1], np.linalg.inv(b.nodes[nodes[-1]]["baseWorld"].astype(np.float64)).astype(np.float32))
        if j % 3 == 0:
            keys = [near_identity()[1] for _ in range(3)]
            b.channel(S.ANIM_PATH_ROTATION, b.sampler(S.ANIM_SLERP, [0, 1, 2], keys), [nodes[-1]])
    b.channel(S.ANIM_PATH_WEIGHTS, b.sampler(S.ANIM_LINEAR, [0, 2], [[0.1, 0, 0, 0], [0.7, 0, 0, 0]]), [0])
    b.channel(S.ANIM_PATH_WEIGHTS, b.sampler(S.ANIM_STEP, [0, 1, 2], [[0.0, 0, 0, 0], [0.3, 0, 0, 0], [0.5, 0, 0, 0]]), [1])
    return b.tables(extra_instances=0)[0]


@pytest.mark.parametrize("joint_count", [5, 300])
def test_animate_into_skinned_update_equals_the_host_route(luts, joint_count):
    assert (joint_count > S.SKIN_LDS_MAX_JOINTS) == (joint_count == 300)
    sc, view, pos, cfg = scenes.config_cornell(luts, W, H)
    cb = scenes.fill_constants(view, pos, sc, 0, cfg["max_bounces"])
    anim = native.Animation(**_skeleton(joint_count, 40 + joint_count))
    device, host = _context("lbvh"), _context("lbvh")
    try:
        for c in (device, host):
            c.upload_scene(sc)
            c.resize(W, H)
        _, bind = D.deformed(sc, 0, 28, 1, 0.02)
        case = SK.gentle_pose(bind, joint_count, 9, targets=2)
        dev = OnDevice(case)
        for times in ([0.4], [1.0], [1.7]):
            anim.set_times(times)
            device.animate(anim, S.ANIMATE_NO_COMMIT)
            palette_ptr, weights_ptr, _ = device.animation_device(anim)
            args = list(dev.args)
            args[3], args[5] = palette_ptr, weights_ptr
            device.update_vertices_skinned(*args, 0, 0)
            _, palette, weights, _ = anim.evaluate_host()
            assert np.abs(palette - np.eye(4, dtype=np.float32)[:3]).max() < 0.5 and palette.std(0).max() > 1e-3 and (weights > 0).any()
            posed = native.quantize_vertices_host(native.skin_vertices_host(case["base"], case["joints"], case["weights"], palette, case["deltas"], weights))
            host.update_vertices(posed, 0)
            _same_products(device, host, cb, times)
    finally:
        device.close(); host.close(); anim.close()


# ---------------------------------------------------------------- 4. error paths
def test_errors_release_and_separate_state(luts):
    tables, sequence = _family()
    sc = _family_scene(luts, tables)
    view, pos = scenes.planar_view(W, H, position=(0.0, 1.0, -11.0))
    cb = scenes.fill_constants(view, pos, sc, 0, 3)
    anim = native.Animation(**tables)
    other = native.Animation(**K.cases()["skin5"]["tables"])
    c = _context("host")
    try:
        c.resize(W, H)
        with pytest.raises(native.HrptError) as e:                       # no scene: what hrpt_update_instances answers
            c.animate(anim)
        assert e.value.code == -1 and "no scene" in str(e.value)
        with pytest.raises(native.HrptError):
            c.read_animation(anim)                                       # nothing evaluated yet
        with pytest.raises(native.HrptError):
            c.animate(anim, 4)                                           # unknown flag
        c.upload_scene(_cube_scene(luts, [np.eye(4)] * 5))               # too few instances for the animation
        c.render(cb, accum_count=1)
        before = c.read_accumulation()
        with pytest.raises(native.HrptError) as e:
            c.animate(anim)
        assert e.value.code == -1 and "instance" in str(e.value)
        c.render(cb, accum_count=1)
        assert _same(c.read_accumulation(), before)
        c.upload_scene(sc)
        images = []
        for times in sequence[:2]:                                       # two animations in turn keep separate device state
            anim.set_times(times)
            other.set_times([times[0], 0.5])
            c.animate(anim)
            c.animate(other, S.ANIMATE_NO_COMMIT)
            for x in (anim, other):
                got, want = c.read_animation(x), x.evaluate_host()[1:]
                assert all(_same(g, w) for g, w in zip(got, want))
            c.render(cb, accum_count=1)
            images.append(c.read_accumulation())
        assert not _same(images[0], images[1])
        c.animate(other)                                                 # lists no instance: commits and builds nothing
        c.render(cb, accum_count=1)
        assert _same(c.read_accumulation(), images[1])
        # release, then the same frame again from a fresh upload of the scene: the tables are uploaded again, the result is the same
        c.release_animation(anim)
        with pytest.raises(native.HrptError):
            c.read_animation(anim)
        c.upload_scene(sc)
        for times in sequence[:2]:
            anim.set_times(times)
            c.animate(anim)
        c.render(cb, accum_count=1)
        assert _same(c.read_accumulation(), images[1])
        assert all(_same(g, w) for g, w in zip(c.read_animation(anim), anim.evaluate_host()[1:]))
        c.release_animation(anim); c.release_animation(anim)             # releasing twice is harmless
    finally:
        c.close(); anim.close(); other.close()
