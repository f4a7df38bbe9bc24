"""Deforming meshes on the device (hrpt_update_vertices / hrpt_update_vertices_device): the quantiser kernel against
the host executor and NumPy, as bytes; after every update the bits of a context that uploaded a scene BUILT with the new vertices (the
oracle gets a fresh scene), for every builder, both kernel paths, partial ranges, refits, the global-memory tree and the two-level structure;
ray queries, the G-buffer and the structure read-back follow; the previous-position protocol of the motion vectors against
tests/deform_reference.py; argument errors, and bad input that changes nothing."""
import numpy as np
import pytest

from hobbyrenderer_amd import native, scenes, structs as S
import bvh_scenes as B
import deform_cases as D
import deform_reference as DR
import gbuffer_reference as G
import motion_reference as M
import test_gbuffer_gpu as TG
from test_bvh_structure_gpu import check_flat_context, check_two_level_context, sorted_records
from test_parity_gpu import _assert_parity
from test_ray_queries_gpu import _rays
from test_update_instances_gpu import _render_pair

pytestmark = pytest.mark.gpu

BUILDERS = {"host": S.BVH_BUILDER_HOST_SAH, "lbvh": S.BVH_BUILDER_GPU_LBVH, "ploc": S.BVH_BUILDER_GPU_PLOC}
CORNELL_UPDATES = [(2, 8), (0, 28), (17, 1)]          # vertices 2..9 cross the boundary between the two meshes (0-3, 4-27); all; one


def _context(builder=None, structure=None):
    c = native.PathTracerContext(0)
    if builder is not None:
        c.set_bvh_builder(BUILDERS[builder])
    if structure is not None:
        c.set_acceleration_structure(structure)
    return c


def _on_device(records):
    import torch
    return torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).copy()).to("cuda:0")


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- 1. the quantiser kernel
@pytest.fixture(scope="module")
def quantiser_inputs():
    v = D.float_vertices()
    return v, D.numpy_quantised(v)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257, D.COUNT])
def test_quantiser_on_the_device(quantiser_inputs, count):
    import torch
    v, ref = quantiser_inputs
    host = native.quantize_vertices_host(v[:count])
    assert host.tobytes() == ref[:count].tobytes()
    ctx = _context()
    try:
        src = _on_device(v[:count])
        for offset in (1, 5):                                   # records into the output: 24-byte alignment only
            dst = torch.full(((count + offset + 1) * 24,), 0xCD, dtype=torch.uint8, device="cuda:0")
            ctx.quantize_vertices_device(src.data_ptr(), count, dst.data_ptr() + 24 * offset, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            out = dst.cpu().numpy()
            assert out[24 * offset:24 * (offset + count)].tobytes() == host.tobytes(), (count, offset)
            assert (out[:24 * offset] == 0xCD).all() and (out[24 * (offset + count):] == 0xCD).all()      # nothing outside the range
    finally:
        ctx.close()


def test_quantiser_nan_rows_host_equals_device():
    import torch
    rows, _, _ = D.nan_vertices()
    ctx = _context()
    try:
        src = _on_device(rows)
        dst = torch.zeros(len(rows) * 24, dtype=torch.uint8, device="cuda:0")
        ctx.quantize_vertices_device(src.data_ptr(), len(rows), dst.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert dst.cpu().numpy().tobytes() == native.quantize_vertices_host(rows).tobytes()
    finally:
        ctx.close()


# ---------------------------------------------------------------- 2. parity with a fresh scene
def _check_cornell(c, now, view, pos, bounces):
    _assert_parity(*_render_pair(c, now, view, pos, 96, 54, 2, bounces, S.FRAME_DEFAULT))
    _assert_parity(*_render_pair(c, now, view, pos, 96, 54, 1, 2, S.FRAME_MEGAKERNEL))
    assert c.build_info().triangleCount == 38 and c.selftest_bvh() == 0


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_updated_vertices_match_a_fresh_scene(luts, builder):
    sc, view, pos, cfg = scenes.config_cornell(luts, 96, 54)
    assert len(sc.vertices) == 28
    c = _context(builder)
    try:
        c.upload_scene(sc)
        now = sc
        for step, (first, count) in enumerate(CORNELL_UPDATES, start=1):
            now, _ = D.deformed(now, first, count, step)
            c.update_vertices(now.vertices[first:first + count], first)
            assert c.build_info().usedBuilder == BUILDERS[builder]
            _check_cornell(c, now, view, pos, cfg["max_bounces"])
    finally:
        c.close()


# ---------------------------------------------------------------- 3. the device variant equals the host variant
@pytest.mark.parametrize("builder,own_stream", [("host", False), ("lbvh", False), ("ploc", False), ("lbvh", True)],
                         ids=["host", "lbvh", "ploc", "lbvh-stream"])
def test_device_variant_equals_host_variant(luts, builder, own_stream):
    import torch
    sc, view, pos, cfg = scenes.config_cornell(luts, 96, 54)
    cb = scenes.fill_constants(view, pos, sc, 0, cfg["max_bounces"])
    ch, cd = _context(builder), _context(builder)
    stream = torch.cuda.Stream() if own_stream else torch.cuda.current_stream()
    try:
        for c in (ch, cd):
            c.upload_scene(sc)
            c.resize(96, 54)
        now = sc
        for step, (first, count) in enumerate(CORNELL_UPDATES, start=1):
            now, fv = D.deformed(now, first, count, step)
            ch.update_vertices(now.vertices[first:first + count], first)
            with torch.cuda.stream(stream):
                dev = _on_device(fv)                             # (the copy runs on `stream`: the call has to wait for it)
                cd.update_vertices_device(dev.data_ptr(), first, count, 0, stream.cuda_stream)
            images = []
            for c in (ch, cd):
                c.render(cb, accum_count=2)
                images.append(c.read_accumulation())
            assert _u32(images[0]).tobytes() == _u32(images[1]).tobytes(), step
            assert sorted_records(ch.read_bvh()) == sorted_records(cd.read_bvh()), step
        _check_cornell(cd, now, view, pos, cfg["max_bounces"])   # ... and both are the fresh scene's (case 2 holds the host variant to it)
    finally:
        ch.close(); cd.close()


# ---------------------------------------------------------------- 4. refit
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_refit_keeps_the_hierarchy_and_the_bits(luts, builder):
    sc, view, pos, cfg = scenes.config_cornell(luts, 96, 54)
    c = _context(builder)
    try:
        c.upload_scene(sc)
        now = sc
        for step, amplitude in enumerate([0.02, 0.03, 0.02, 1.0], start=1):        # three small deformations, then a large one
            now, _ = D.deformed(now, 0, 28, step, amplitude)
            c.update_vertices(now.vertices, 0, S.VERTICES_REFIT)
            kept = S.BVH_BUILDER_REFITTED if builder != "host" else 0
            assert c.build_info().usedBuilder == (BUILDERS[builder] | kept), hex(c.build_info().usedBuilder)
            _check_cornell(c, now, view, pos, cfg["max_bounces"])
    finally:
        c.close()


# ---------------------------------------------------------------- 5. structure of what the kernels walk
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_structure_after_update_and_refit(luts, builder):
    sc = scenes.sponza_class_scene(luts, 0.25, 8)              # tangents, textures, MASK foliage
    assert len(sc.vertices) == 415
    c = _context(builder)
    try:
        c.upload_scene(sc)
        now, _ = D.deformed(sc, 0, 415, 1)
        c.update_vertices(now.vertices)
        d, _, _ = check_flat_context(c, now)
        if builder != "host":
            assert sorted_records(d) == sorted_records(native.host_build_bvh(now))
        now, _ = D.deformed(now, 101, 200, 2, 0.02)
        c.update_vertices(now.vertices[101:301], 101, S.VERTICES_REFIT)
        d, bi, _ = check_flat_context(c, now)
        if builder != "host":
            assert bi.usedBuilder & S.BVH_BUILDER_REFITTED, hex(bi.usedBuilder)
            assert sorted_records(d) == sorted_records(native.host_build_bvh(now))
    finally:
        c.close()


# ---------------------------------------------------------------- 6. global-memory tree, textured
def _mesh_vertex_range(sc, mesh):
    md = sc.mesh_data[mesh]
    idx = sc.indices[md["m_IndexOffsets"][0]:md["m_IndexOffsets"][0] + md["m_IndexCounts"][0]]
    return int(idx.min()), int(idx.max()) - int(idx.min()) + 1


@pytest.mark.parametrize("builder", ["lbvh", "host"])
def test_large_textured_scene(luts, builder):
    sc, view, pos, cfg = scenes.config_sponza_class(luts, 96, 54, detail=1.0, tex_size=32)
    c = _context(builder)
    try:
        c.upload_scene(sc)
        first, count = _mesh_vertex_range(sc, 0)
        assert 0 < count < len(sc.vertices)
        now, _ = D.deformed(sc, first, count, 1)
        c.update_vertices(now.vertices[first:first + count], first)
        bi = c.build_info()
        assert bi.usedBuilder == BUILDERS[builder] and bi.triangleCount > 90000
        _assert_parity(*_render_pair(c, now, view, pos, 96, 54, 2, cfg["max_bounces"], S.FRAME_DEFAULT))
        c.update_vertices(sc.vertices[first:first + count], first)          # and back: the original tree, rebuilt in the same buffers
        _assert_parity(*_render_pair(c, sc, view, pos, 96, 54, 2, cfg["max_bounces"], S.FRAME_DEFAULT))
    finally:
        c.close()


# ---------------------------------------------------------------- 7. two-level structure
def test_two_level_structure_follows(luts):
    sc = B.instanced_scene(luts, 60, detail=8)
    assert len(sc.vertices) == 245
    first, count = _mesh_vertex_range(sc, 1)
    now, _ = D.deformed(sc, first, count, 1)
    view, pos = scenes.planar_view(96, 54, position=(7.0, 7.0, -7.0), pitch=0.55)
    cb = scenes.fill_constants(view, pos, now, 0, 4)
    frames = {}
    for structure in (S.ACCEL_TWO_LEVEL, S.ACCEL_FLAT):
        c = _context(structure=structure)
        try:
            c.upload_scene(sc)
            c.update_vertices(now.vertices[first:first + count], first)
            assert c.build_info().structure == structure
            if structure == S.ACCEL_TWO_LEVEL:
                check_two_level_context(c, now, False)
            c.resize(96, 54)
            c.render(cb, accum_count=2)
            frames[structure] = c.read_accumulation()
        finally:
            c.close()
    a, b = frames[S.ACCEL_TWO_LEVEL], frames[S.ACCEL_FLAT]
    assert _u32(a).tobytes() == _u32(b).tobytes()
    assert np.isfinite(a).all() and a[..., :3].max() > 0


# ---------------------------------------------------------------- 8. ray queries and the G-buffer follow
def test_ray_queries_and_gbuffer_follow(luts):
    from oracle.binding import Oracle
    sc, view, pos, cfg = scenes.config_cornell(luts, 64, 36)
    now, _ = D.deformed(sc, 0, 28, 1)
    rays = _rays(np.random.default_rng(7), 20000)
    cb = scenes.fill_constants(view, pos, now, 1, cfg["max_bounces"])
    fresh, c = _context(), _context()
    try:
        fresh.upload_scene(now)
        c.upload_scene(sc)
        c.update_vertices(now.vertices)
        for shadow in (False, True):
            assert c.trace_rays(rays, shadow=shadow).tobytes() == fresh.trace_rays(rays, shadow=shadow).tobytes(), shadow
        assert fresh.trace_rays(rays)["hit"].sum() > 2000            # (a tenth of the rays: the comparison is not over misses alone)
        c.resize(64, 36)
        c.render_gbuffer(cb)
        o = Oracle(now)
        try:
            ref = G.gbuffer(now, o, cb, 64, 36)
        finally:
            o.close()
        TG._assert_same(TG._read_all(c), ref, "G-buffer after an update vs reference on the deformed scene")
    finally:
        fresh.close(); c.close()


# ---------------------------------------------------------------- 9. motion vectors: the previous-position protocol
W, H = 64, 36
_MOTION = {}


def _motion_case(luts):
    """The cube scene through five deformations, with the reference trace and unpacked vertices of every state (computed once)."""
    if not _MOTION:
        from oracle.binding import Oracle
        sc, cb = G.cube_case(luts, W, H, 0, (0.0, 0.0))
        sc.instances["m_PrevWorld"] = sc.instances["m_World"]
        assert len(sc.vertices) == 24
        states = [sc]
        for step, (first, count) in enumerate([(0, 24), (0, 12), (12, 12), (0, 12), (12, 12)], start=1):
            states.append(D.deformed(states[-1], first, count, step)[0])
        verts, traces = [], []
        for s in states:
            o = Oracle(s)
            try:
                verts.append(G.unpacked_vertices(s))
                traces.append(G.trace(s, o, cb, W, H))
            finally:
                o.close()
            assert 100 < traces[-1]["hit"].sum() < W * H
        _MOTION["case"] = (states, cb, verts, traces)
    return _MOTION["case"]


def _read_motion(c, cb, flags):
    c.render_motion_vectors(cb, cb["m_View"], flags=flags)
    return c.read_motion_vectors()


def _same_motion(got, want, what):
    bad = (_u32(got) != _u32(want)).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} motion texels differ, first at {np.argwhere(bad)[0]}"


@pytest.mark.parametrize("structure", [S.ACCEL_FLAT, S.ACCEL_TWO_LEVEL], ids=["flat", "two-level"])
@pytest.mark.parametrize("label,flags", TG.PATHS)
def test_motion_vectors_of_a_deforming_mesh(luts, structure, label, flags):
    states, cb, verts, traces = _motion_case(luts)
    view = cb["m_View"]

    def moving(k):
        return _u32(ref)[..., :3].any(-1)[traces[k]["hit"]]

    c = _context(structure=structure)
    try:
        c.upload_scene(states[0])
        c.resize(W, H)
        # a context that never updates: the definition as it was
        _same_motion(_read_motion(c, cb, flags), M.motion(states[0], cb, view, W, H, verts[0], traces[0]), "before any update")
        # one update of everything: previous = the old vertices
        c.update_vertices(states[1].vertices)
        assert c.build_info().structure == structure
        ref = DR.motion(states[1], cb, view, W, H, verts[1], verts[0], traces[1])
        got = _read_motion(c, cb, flags)
        _same_motion(got, ref, "after an update")
        assert moving(1).all() and np.hypot(got[..., 0], got[..., 1])[traces[1]["hit"]].max() > 0.5
        # a frame in which nothing deforms: static camera and instance give zeros on hits apart from the valid flag
        c.end_vertex_frame()
        got = _read_motion(c, cb, flags)
        _same_motion(got, M.motion(states[1], cb, view, W, H, verts[1], traces[1]), "after end_vertex_frame")
        assert not _u32(got)[..., :3].any() and (got[..., 3][traces[1]["hit"]] == 1).all()
        # two ranges in one frame, the second with SAME_FRAME: both report their motion
        c.update_vertices(states[2].vertices[0:12], 0)
        c.update_vertices(states[3].vertices[12:24], 12, S.VERTICES_SAME_FRAME)
        ref = DR.motion(states[3], cb, view, W, H, verts[3], verts[1], traces[3])
        _same_motion(_read_motion(c, cb, flags), ref, "two ranges of one frame")
        assert moving(3).all()
        # the same second call without the flag starts a new frame: the first range reports none
        c.update_vertices(states[4].vertices[0:12], 0)
        c.update_vertices(states[5].vertices[12:24], 12)
        ref = DR.motion(states[5], cb, view, W, H, verts[5], verts[4], traces[5])
        _same_motion(_read_motion(c, cb, flags), ref, "a second call without SAME_FRAME")
        assert moving(5).any() and not moving(5).all()
    finally:
        c.close()


# ---------------------------------------------------------------- 10. errors and atomicity
def test_argument_errors(luts):
    sc = scenes.cornell_scene(luts)
    ok = sc.vertices[:4].copy()
    dev = _on_device(np.zeros(4, S.VertexFloat))
    c = _context()
    try:
        def code(fn, *args):
            with pytest.raises(native.HrptError) as e:
                fn(*args)
            return e.value.code

        no_scene = code(c.update_instances, sc.instances)                  # before an upload: what hrpt_update_instances answers there
        assert code(c.update_vertices, ok) == no_scene and code(c.update_vertices_device, dev.data_ptr(), 0, 4) == no_scene
        assert code(c.end_vertex_frame) == no_scene
        c.upload_scene(sc)
        before = c.read_bvh()
        lib, h = native.lib, c._h
        assert lib.hrpt_update_vertices(h, None, 0, 4, 0) == -1            # null array with count > 0
        assert lib.hrpt_update_vertices_device(h, None, 0, 4, 0, None) == -1
        assert code(c.update_vertices, ok, 25) == -1                        # 25 + 4 > 28
        assert code(c.update_vertices, ok, 0xFFFFFFFE) == -1                # the 64-bit sum
        assert code(c.update_vertices_device, dev.data_ptr(), 25, 4) == -1
        assert code(c.update_vertices_device, dev.data_ptr(), 0xFFFFFFFE, 4) == -1
        assert code(c.update_vertices, ok, 0, 4) == -1                      # unknown flag bit
        assert code(c.update_vertices_device, dev.data_ptr(), 0, 4, 8) == -1
        assert lib.hrpt_update_vertices(h, None, 0, 0, 4) == -1             # ... also with count 0
        c.update_vertices(ok[:0], 3)                                        # count 0: HRPT_OK, builds nothing
        c.update_vertices(ok[:0], 28, S.VERTICES_SAME_FRAME)
        c.end_vertex_frame()
        assert lib.hrpt_quantize_vertices_device(h, None, 4, dev.data_ptr(), None) == -1
        assert lib.hrpt_quantize_vertices_device(h, dev.data_ptr(), 4, None, None) == -1
        assert sorted_records(c.read_bvh()) == sorted_records(before)
    finally:
        c.close()


@pytest.mark.parametrize("builder", ["host", "lbvh"])
def test_bad_positions_change_nothing(luts, builder):
    sc, view, pos, cfg = scenes.config_cornell(luts, 96, 54)
    cb = scenes.fill_constants(view, pos, sc, 0, cfg["max_bounces"])
    now, fv = D.deformed(sc, 0, 28, 1)
    c = _context(builder)
    try:
        c.upload_scene(sc)
        c.resize(96, 54)

        def frame():
            c.render(cb, accum_count=1)
            return c.read_accumulation().tobytes()

        image, records = frame(), sorted_records(c.read_bvh())
        bad = now.vertices.copy()
        bad["m_Pos"][13, 1] = np.inf
        with pytest.raises(native.HrptError) as e:
            c.update_vertices(bad)
        assert e.value.code == -1 and "non-finite" in str(e.value)
        assert frame() == image and sorted_records(c.read_bvh()) == records
        bad = fv.copy()
        bad["pos"][27, 2] = np.nan
        with pytest.raises(native.HrptError) as e:
            c.update_vertices_device(_on_device(bad).data_ptr(), 0, 28)
        assert e.value.code == -1 and "non-finite" in str(e.value)
        assert frame() == image and sorted_records(c.read_bvh()) == records
        c.update_vertices_device(_on_device(fv).data_ptr(), 0, 28)           # a valid update afterwards still works
        _check_cornell(c, now, view, pos, cfg["max_bounces"])
    finally:
        c.close()
