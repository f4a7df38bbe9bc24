"""Skinning and morph targets on the device (hrpt_skin_vertices_device / hrpt_update_vertices_skinned): the kernels
against the host executor, as bytes, on both sides of the LDS-palette threshold; the one-call update against a second context that takes the
host route (hrpt_skin_vertices_host + hrpt_quantize_vertices_host + hrpt_update_vertices) and against the oracle on a scene built with
those vertices; refits; the two-call route; the previous-position protocol of the motion vectors; bad input that changes nothing; and
argument errors. tests/test_skin_cpu.py ties the host executor to the NumPy statement and to float64."""
import copy

import numpy as np
import pytest

from hobbyrenderer_amd import native, scenes, structs as S
import deform_cases as D
import deform_reference as DR
import gbuffer_reference as G
import skin_cases as K
import test_gbuffer_gpu as TG
from test_bvh_structure_gpu import sorted_records
from test_deform_gpu import BUILDERS, CORNELL_UPDATES, _check_cornell, _context, _read_motion, _same_motion, _u32

pytestmark = pytest.mark.gpu

JOINT_COUNTS = [1, 4, S.SKIN_LDS_MAX_JOINTS, S.SKIN_LDS_MAX_JOINTS + 1]


class OnDevice:
    """The arrays of a case in device memory (torch tensors, kept alive here) and what the context calls take: their addresses and counts."""

    def __init__(self, case):
        import torch
        arrays, self.count, self.joint_count, self.target_count = native.skin_arrays(**case)
        self.tensors = [None if a is None else torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0") for a in arrays]
        self.args = tuple(0 if t is None or t.numel() == 0 else t.data_ptr() for t in self.tensors) + (self.count, self.joint_count, self.target_count)


def _host_route(case):
    return native.quantize_vertices_host(native.skin_vertices_host(**case))


def _with_vertices(sc, first, records):
    out = copy.copy(sc)
    out.vertices = sc.vertices.copy()
    out.vertices[first:first + len(records)] = records
    return out


# ---------------------------------------------------------------- 1. the kernels against the host executor
_CASES = {}


def _case(joint_count):
    if joint_count not in _CASES:
        _CASES[joint_count] = K.random_case(joint_count=joint_count)
    return _CASES[joint_count]


@pytest.fixture(scope="module")
def ctx():
    c = _context()
    yield c
    c.close()


@pytest.mark.parametrize("joint_count", JOINT_COUNTS)
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257, K.COUNT])
def test_kernel_equals_the_host_executor(ctx, count, joint_count):
    import torch
    own = torch.cuda.Stream()
    for targets in (0, 1, 3):                                            # three targets: the middle weight is exactly zero
        case = K.select(_case(joint_count), count, targets=targets)
        want = native.skin_vertices_host(**case)
        dev = OnDevice(case)
        for stream, offset in ((own, 1), (torch.cuda.current_stream(), 5)):
            with torch.cuda.stream(stream):
                dst = torch.full(((count + offset + 1) * 48,), 0xCD, dtype=torch.uint8, device="cuda:0")
                status = torch.zeros(2, dtype=torch.int32, device="cuda:0")
                ctx.skin_vertices_device(*dev.args, dst.data_ptr() + 48 * offset, status.data_ptr(), stream.cuda_stream)
                staged = torch.full(((count + offset + 1) * 24,), 0xCD, dtype=torch.uint8, device="cuda:0")
                ctx.quantize_vertices_device(dst.data_ptr() + 48 * offset, count, staged.data_ptr() + 24 * offset, stream.cuda_stream)
            stream.synchronize()
            out = dst.cpu().numpy()
            assert out[48 * offset:48 * (offset + count)].tobytes() == want.tobytes(), (count, joint_count, targets)
            assert (out[:48 * offset] == 0xCD).all() and (out[48 * (offset + count):] == 0xCD).all()       # nothing outside the range
            assert status.cpu().tolist() == [0, 0]
            assert staged.cpu().numpy()[24 * offset:24 * (offset + count)].tobytes() == native.quantize_vertices_host(want).tobytes()


@pytest.mark.parametrize("morph", [False, True], ids=["neither", "morph"])
def test_kernel_without_joints(ctx, morph):
    import torch
    case = K.select(_case(4), 321, skin=False, morph=morph)
    dev = OnDevice(case)
    dst = torch.zeros(321 * 48, dtype=torch.uint8, device="cuda:0")
    ctx.skin_vertices_device(*dev.args, dst.data_ptr())                 # no status array, the default stream
    torch.cuda.synchronize()
    assert dst.cpu().numpy().tobytes() == native.skin_vertices_host(**case).tobytes()


def test_edge_rows_on_the_device(ctx):
    import torch
    case = K.edge_case()
    dev = OnDevice(case)
    dst = torch.zeros(dev.count * 48, dtype=torch.uint8, device="cuda:0")
    ctx.skin_vertices_device(*dev.args, dst.data_ptr())
    torch.cuda.synchronize()
    assert dst.cpu().numpy().tobytes() == native.skin_vertices_host(**case).tobytes()


# ---------------------------------------------------------------- 2. the one-call update (`fused`) against the host route and the oracle
def _same_products(a, b, cb, what):
    for flags in (S.FRAME_DEFAULT, S.FRAME_MEGAKERNEL):
        images = []
        for c in (a, b):
            c.render(cb, accum_count=2, flags=flags)
            images.append(c.read_accumulation())
        assert _u32(images[0]).tobytes() == _u32(images[1]).tobytes(), (what, flags)
    ia, ib = a.build_info(), b.build_info()
    for name, _ in S.BuildInfo._fields_:
        if name not in ("buildMs", "deviceBuildMs", "sahCost"):
            assert getattr(ia, name) == getattr(ib, name), (what, name)
    # sahCost of a GPU build is a sum by atomic additions in no fixed order: each context is within the bound tests/bvh_reference.py
    # derives, (8 + 6 + nodeCount / 64 + 8) * 2^-24 relative, of the exact sum, so two of them are within twice that of each other
    gpu_built = (ia.usedBuilder & 0xff) != S.BVH_BUILDER_HOST_SAH
    bound = 2 * (22 + ia.nodeCount / 64.0) * 2.0 ** -24 * max(ia.sahCost, ib.sahCost) if gpu_built else 0.0
    assert abs(ia.sahCost - ib.sahCost) <= bound, (what, ia.sahCost, ib.sahCost, bound)
    assert sorted_records(a.read_bvh()) == sorted_records(b.read_bvh()), what


@pytest.mark.parametrize("builder,own_stream", [("host", False), ("lbvh", False), ("ploc", False), ("lbvh", True)],
                         ids=["host", "lbvh", "ploc", "lbvh-stream"])
def test_skinned_update_equals_the_host_route(luts, builder, own_stream):
    import torch
    sc, view, pos, cfg = scenes.config_cornell(luts, 96, 54)
    assert len(sc.vertices) == 28
    cb = scenes.fill_constants(view, pos, sc, 0, cfg["max_bounces"])
    fused, host = _context(builder), _context(builder)
    stream = torch.cuda.Stream() if own_stream else torch.cuda.current_stream()
    try:
        for c in (fused, host):
            c.upload_scene(sc)
            c.resize(96, 54)
        now = sc
        for step, (first, count) in enumerate(CORNELL_UPDATES, start=1):
            _, bind = D.deformed(now, first, count, step, 0.02)
            case = K.gentle_pose(bind, 4, step)
            posed = _host_route(case)
            now = _with_vertices(now, first, posed)
            with torch.cuda.stream(stream):
                dev = OnDevice(case)                                     # (the copies run on `stream`: the call has to wait for them)
                fused.update_vertices_skinned(*dev.args, first, 0, stream.cuda_stream)
            host.update_vertices(posed, first)
            assert fused.build_info().usedBuilder == BUILDERS[builder]
            _same_products(fused, host, cb, step)
        _check_cornell(fused, now, view, pos, cfg["max_bounces"])       # ... and both are the scene built with those vertices
    finally:
        fused.close(); host.close()


def test_skinned_update_of_a_larger_scene_and_refit(luts):
    """415 vertices (two blocks), a palette one joint past the LDS threshold, then small poses with HRPT_VERTICES_REFIT on a partial range."""
    sc, view, pos, cfg = scenes.config_sponza_class(luts, 96, 54, detail=0.25, tex_size=8)
    assert len(sc.vertices) == 415
    cb = scenes.fill_constants(view, pos, sc, 0, 4)
    fused, host = _context("lbvh"), _context("lbvh")
    try:
        for c in (fused, host):
            c.upload_scene(sc)
            c.resize(96, 54)
        now = sc
        for step, (first, count, joint_count, flags) in enumerate([(0, 415, S.SKIN_LDS_MAX_JOINTS + 1, 0), (101, 300, S.SKIN_LDS_MAX_JOINTS, S.VERTICES_REFIT),
                                                                   (0, 415, 7, S.VERTICES_REFIT)], start=1):
            _, bind = D.deformed(now, first, count, step, 0.01)
            case = K.gentle_pose(bind, joint_count, step, amplitude=0.01)
            posed = _host_route(case)
            now = _with_vertices(now, first, posed)
            fused.update_vertices_skinned(*OnDevice(case).args, first, flags)
            host.update_vertices(posed, first, flags)
            kept = S.BVH_BUILDER_REFITTED if flags else 0
            assert fused.build_info().usedBuilder == (S.BVH_BUILDER_GPU_LBVH | kept), hex(fused.build_info().usedBuilder)
            _same_products(fused, host, cb, step)
        assert sorted_records(fused.read_bvh()) == sorted_records(native.host_build_bvh(now))
    finally:
        fused.close(); host.close()


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_refit_keeps_the_hierarchy(luts, builder):
    sc, view, pos, cfg = scenes.config_cornell(luts, 96, 54)
    c = _context(builder)
    try:
        c.upload_scene(sc)
        now = sc
        for step in (1, 2):
            _, bind = D.deformed(now, 0, 28, step, 0.02)
            case = K.gentle_pose(bind, 4, step, amplitude=0.02)
            now = _with_vertices(now, 0, _host_route(case))
            c.update_vertices_skinned(*OnDevice(case).args, 0, S.VERTICES_REFIT)
            kept = S.BVH_BUILDER_REFITTED if builder != "host" else 0
            assert c.build_info().usedBuilder == (BUILDERS[builder] | kept), hex(c.build_info().usedBuilder)
        _check_cornell(c, now, view, pos, cfg["max_bounces"])
    finally:
        c.close()


# ---------------------------------------------------------------- 3. the two-call route
def test_two_call_route_gives_the_same_records(luts):
    import torch
    sc = scenes.cornell_scene(luts)
    _, bind = D.deformed(sc, 0, 28, 1, 0.02)
    case = K.gentle_pose(bind, 4, 3)
    dev = OnDevice(case)
    fused, two = _context("lbvh"), _context("lbvh")
    try:
        fused.upload_scene(sc); two.upload_scene(sc)
        fused.update_vertices_skinned(*dev.args, 0)
        floats = torch.zeros(28 * 48, dtype=torch.uint8, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream
        two.skin_vertices_device(*dev.args, floats.data_ptr(), 0, stream)
        two.update_vertices_device(floats.data_ptr(), 0, 28, 0, stream)
        assert sorted_records(fused.read_bvh()) == sorted_records(two.read_bvh())
    finally:
        fused.close(); two.close()


# ---------------------------------------------------------------- 4. motion vectors: pose A, then pose B
W, H = 64, 36


def test_motion_vectors_between_two_poses(luts):
    from oracle.binding import Oracle
    label, flags = TG.PATHS[0]
    sc, cb = G.cube_case(luts, W, H, 0, (0.0, 0.0))
    sc.instances["m_PrevWorld"] = sc.instances["m_World"]
    assert len(sc.vertices) == 24
    _, bind = D.deformed(sc, 0, 24, 1, 0.0)
    poses = [K.gentle_pose(bind, 4, seed, amplitude=0.15) for seed in (1, 2)]
    states = [_with_vertices(sc, 0, _host_route(p)) for p in poses]
    assert (states[0].vertices["m_Pos"] != states[1].vertices["m_Pos"]).any()
    o = Oracle(states[1])
    try:
        verts, trace = [G.unpacked_vertices(s) for s in states], G.trace(states[1], o, cb, W, H)
    finally:
        o.close()
    assert 100 < trace["hit"].sum() < W * H
    c = _context(structure=S.ACCEL_FLAT)
    try:
        c.upload_scene(sc)
        c.resize(W, H)
        for p in poses:
            c.update_vertices_skinned(*OnDevice(p).args, 0)
        ref = DR.motion(states[1], cb, cb["m_View"], W, H, verts[1], verts[0], trace)
        got = _read_motion(c, cb, flags)
        _same_motion(got, ref, f"pose A then pose B ({label})")
        assert _u32(ref)[..., :3].any(-1)[trace["hit"]].any()
    finally:
        c.close()


# ---------------------------------------------------------------- 5. bad input changes nothing
@pytest.mark.parametrize("builder", ["host", "lbvh"])
def test_bad_input_changes_nothing(luts, builder):
    """A palette holding inf raises status word 0; a joint index equal to jointCount raises word 1 (the kernel reads joint jointCount - 1
    instead: the clamp tests/test_skin_cpu.py and the sanitizer program establish). Either refuses the update."""
    import torch
    sc, view, pos, cfg = scenes.config_cornell(luts, 96, 54)
    cb = scenes.fill_constants(view, pos, sc, 0, cfg["max_bounces"])
    _, bind = D.deformed(sc, 0, 28, 1, 0.02)
    good = K.gentle_pose(bind, 4, 1)
    infinite = dict(good, joint_matrices=good["joint_matrices"].copy())
    infinite["joint_matrices"][int(good["joints"][13, 0]), 1, 3] = np.inf
    stray = dict(good, joints=good["joints"].copy())
    stray["joints"][27, 2] = 4
    c = _context(builder)
    try:
        c.upload_scene(sc)
        c.resize(96, 54)

        def frame():
            c.render(cb, accum_count=1)
            return c.read_accumulation().tobytes()

        image, records = frame(), sorted_records(c.read_bvh())
        for case, words, message in ((infinite, [1, 0], "non-finite"), (stray, [0, 1], "joint index out of range")):
            dev = OnDevice(case)
            with pytest.raises(native.HrptError) as e:
                c.update_vertices_skinned(*dev.args, 0)
            assert e.value.code == -1 and message in str(e.value)
            assert frame() == image and sorted_records(c.read_bvh()) == records
            floats = torch.zeros(28 * 48, dtype=torch.uint8, device="cuda:0")
            status = torch.zeros(2, dtype=torch.int32, device="cuda:0")
            c.skin_vertices_device(*dev.args, floats.data_ptr(), status.data_ptr())
            torch.cuda.synchronize()
            assert status.cpu().tolist() == words
        clamped = dict(stray, joints=good["joints"].copy())
        clamped["joints"][27, 2] = 3
        assert floats.cpu().numpy().tobytes() == native.skin_vertices_host(**clamped).tobytes()      # the stray index read joint jointCount - 1
        c.update_vertices_skinned(*OnDevice(good).args, 0)                # a valid update afterwards still works
        _check_cornell(c, _with_vertices(sc, 0, _host_route(good)), view, pos, cfg["max_bounces"])
    finally:
        c.close()


# ---------------------------------------------------------------- 6. argument errors
def test_argument_errors(luts):
    import torch
    sc = scenes.cornell_scene(luts)
    _, bind = D.deformed(sc, 0, 4, 1, 0.02)
    dev = OnDevice(K.gentle_pose(bind, 4, 1))
    base, joints, weights, matrices, deltas, mw, n, jc, tc = dev.args
    out = torch.zeros(4 * 48 + 16, dtype=torch.uint8, device="cuda:0")
    c = _context()
    try:
        def code(fn, *args):
            with pytest.raises(native.HrptError) as e:
                fn(*args)
            return e.value.code

        no_scene = code(c.update_instances, sc.instances)                  # before an upload: what hrpt_update_instances answers there
        assert code(c.update_vertices_skinned, *dev.args, 0) == no_scene
        c.upload_scene(sc)
        before = c.read_bvh()
        lib, h = native.lib, c._h
        assert lib.hrpt_update_vertices_skinned(h, None, 0, 0, None) == -1 and lib.hrpt_skin_vertices_device(h, None, out.data_ptr(), None, None) == -1
        for fn, tail in ((c.update_vertices_skinned, (0,)), (c.skin_vertices_device, (out.data_ptr(),))):
            assert code(fn, 0, joints, weights, matrices, deltas, mw, n, jc, tc, *tail) == -1              # NULL base
            assert code(fn, base + 8, joints, weights, matrices, deltas, mw, n, jc, tc, *tail) == -1      # misaligned
            assert code(fn, base, joints + 4, weights, matrices, deltas, mw, n, jc, tc, *tail) == -1
            assert code(fn, base, joints, weights + 8, matrices, deltas, mw, n, jc, tc, *tail) == -1
            assert code(fn, base, joints, weights, matrices + 8, deltas, mw, n, jc, tc, *tail) == -1
            assert code(fn, base, joints, weights, matrices, deltas + 2, mw, n, jc, tc, *tail) == -1
            assert code(fn, base, joints, 0, matrices, deltas, mw, n, jc, tc, *tail) == -1                # joints without weights
            assert code(fn, base, joints, weights, 0, deltas, mw, n, jc, tc, *tail) == -1                 # ... without matrices
            assert code(fn, base, joints, weights, matrices, deltas, mw, n, 0, tc, *tail) == -1           # ... with jointCount 0
            assert code(fn, base, joints, weights, matrices, 0, mw, n, jc, tc, *tail) == -1               # targets without deltas
            assert code(fn, base, joints, weights, matrices, deltas, 0, n, jc, tc, *tail) == -1           # ... without weights
        args = S.SkinArgs(base, joints, weights, matrices, deltas, mw, n, jc, tc, 1)                      # reserved
        assert lib.hrpt_update_vertices_skinned(h, args, 0, 0, None) == -1 and lib.hrpt_skin_vertices_device(h, args, out.data_ptr(), None, None) == -1
        assert code(c.update_vertices_skinned, *dev.args, 25) == -1                                        # 25 + 4 > 28
        assert code(c.update_vertices_skinned, *dev.args, 0xFFFFFFFE) == -1                                # the 64-bit sum
        assert code(c.update_vertices_skinned, *dev.args, 0, 8) == -1                                      # unknown flag bit
        assert code(c.skin_vertices_device, *dev.args, 0) == -1                                            # NULL out
        assert code(c.skin_vertices_device, *dev.args, out.data_ptr() + 8) == -1                           # misaligned out
        assert code(c.skin_vertices_device, *dev.args, base + 48) == -1                                    # out overlaps base
        c.update_vertices_skinned(base, joints, weights, matrices, deltas, mw, 0, jc, tc, 3)               # count 0: HRPT_OK, builds nothing
        c.update_vertices_skinned(0, 0, 0, 0, 0, 0, 0, 0, 0, 28, S.VERTICES_SAME_FRAME)
        c.skin_vertices_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        assert sorted_records(c.read_bvh()) == sorted_records(before)
    finally:
        c.close()
