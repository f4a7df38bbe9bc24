"""First-hit motion vectors on the device (hrpt_render_motion_vectors): the motion plane, bit for bit on uint32 views,
against the NumPy reference (tests/motion_reference.py) on both kernel paths, across acceleration structures, builders and node formats,
through the per-frame instance protocol, with plane masks, tiles and stripes, and without a trace in what renders leave behind.
Scenes, cached reference traces and device helpers are those of tests/test_gbuffer_gpu.py."""
import copy
import math

import numpy as np
import pytest

from hobbyrenderer_amd import scenes, structs as S
from scene_helpers import random_soup
import gbuffer_reference as G
import motion_reference as M
import test_gbuffer_gpu as TG
import test_motion_cpu as MC

pytestmark = pytest.mark.gpu

PATHS = TG.PATHS
SENTINEL = np.uint32(0xCDCDCDCD)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_same(got, want, what):
    a, b = _u32(got), _u32(want)
    bad = (a != b).any(-1)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} motion texels differ, first at (x={x}, y={y}): {got[y, x]} != {want[y, x]}")


def _device_motion(sc, cb, prev_view, w, h, flags=S.FRAME_DEFAULT, prepare=None):
    from hobbyrenderer_amd.native import PathTracerContext
    ctx = PathTracerContext(0)
    try:
        if prepare:
            prepare(ctx)
        ctx.upload_scene(sc)
        ctx.resize(w, h)
        ctx.render_motion_vectors(cb, prev_view, flags=flags)
        return ctx.read_motion_vectors(), ctx.build_info()
    finally:
        ctx.close()


def _rigid(rng, angle, shift):
    """A random rigid motion as a row-vector 4 x 4 matrix (float64): rotation by up to `angle` rad about a random axis, then a translation."""
    axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
    a = rng.uniform(-angle, angle)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    m = np.eye(4)
    m[:3, :3] = (np.eye(3) + math.sin(a) * k + (1 - math.cos(a)) * (k @ k)).T
    m[3, :3] = rng.uniform(-shift, shift, 3)
    return m


def _with_prev(sc, seed, angle=0.25, shift=0.2):
    """The scene with a different random rigid m_PrevWorld for every instance."""
    rng = np.random.default_rng(seed)
    out = copy.copy(sc)
    inst = sc.instances.copy()
    for k in range(len(inst)):
        inst["m_PrevWorld"][k] = (inst["m_World"][k].astype(np.float64) @ _rigid(rng, angle, shift)).astype(np.float32)
    out.instances = inst
    return out


def _reference(sc, cb, prev_view, w, h, tr):
    """NumPy motion plane; asserts the case stays away from prevClip.w == 0 and really moves."""
    mv, d = M.motion(sc, cb, prev_view, w, h, G.unpacked_vertices(sc), tr, details=True)
    assert d["prev_w"].min() > 0.25 and d["w"].min() > 0.25
    return mv


# ---------------------------------------------------------------- 1. cube, four scenarios
@pytest.mark.parametrize("name", ["static", "camera", "object", "both"])
def test_cube_equals_reference(luts, name):
    sc, cb, w, h, _, tr = TG._case(luts, "cube")
    assert (w, h) == (MC.W, MC.H)
    s, prev_view = MC.scenario(sc, cb, name)
    ref = _reference(s, cb, prev_view, w, h, tr)
    hit = tr["hit"]
    assert 0 < hit.sum() < hit.size
    for label, flags in PATHS:
        got, _ = _device_motion(s, cb, prev_view, w, h, flags)
        _assert_same(got, ref, f"cube, {name}, {label} vs reference")
        if name == "static":                                   # equal transforms and views: exactly (+0, +0, +0, 1) on hits, four zeros on misses
            g = _u32(got)
            assert not g[..., :3].any() and (got[..., 3][hit] == 1).all() and not g[..., 3][~hit].any()
        else:
            assert np.hypot(got[..., 0], got[..., 1])[hit].max() > 0.5


# ---------------------------------------------------------------- 2. instances, both structures; RNG-dependent first hits
_INSTANCED = {}


def _instanced_case(luts):
    if not _INSTANCED:
        from oracle.binding import Oracle
        w, h = 80, 48
        sc = _with_prev(TG._instanced(luts), 21)
        view, pos = scenes.planar_view(w, h, position=(0.3, 4.5, -8.0), pitch=0.45)
        prev_view, _ = scenes.planar_view(w, h, position=(0.1, 4.6, -8.2), yaw=0.03, pitch=0.43)
        cb = scenes.fill_constants(view, pos, sc, 1, 4)
        o = Oracle(sc)
        try:
            tr = G.trace(sc, o, cb, w, h)
        finally:
            o.close()
        _INSTANCED["case"] = (sc, cb, prev_view, w, h, tr, _reference(sc, cb, prev_view, w, h, tr))
    return _INSTANCED["case"]


def test_instanced_scene_flat_and_two_level(luts, monkeypatch):
    sc, cb, prev_view, w, h, tr, ref = _instanced_case(luts)
    assert len(np.unique(tr["inst"][tr["hit"]])) > 20
    for structure in (S.ACCEL_FLAT, S.ACCEL_TWO_LEVEL):
        monkeypatch.setenv("HRPT_ACCEL_STRUCTURE", str(structure))
        for label, flags in PATHS:
            got, bi = _device_motion(sc, cb, prev_view, w, h, flags)
            assert bi.structure == structure
            _assert_same(got, ref, f"instanced scene, structure {structure}, {label} vs reference")


def test_soup_with_rng_dependent_first_hits(luts):
    sc0, cb, w, h, _, tr = TG._case(luts, "soup-11-5")
    assert (w, h) == (80, 48) and (tr["rng"] != tr["seed"]).any()        # BLEND candidates drew from the path's RNG
    sc = _with_prev(sc0, 22)
    prev_view, _ = scenes.planar_view(w, h, position=(0.15, 0.35, -5.2), yaw=-0.04, pitch=0.02)
    ref = _reference(sc, cb, prev_view, w, h, tr)
    for label, flags in PATHS:
        got, _ = _device_motion(sc, cb, prev_view, w, h, flags)
        _assert_same(got, ref, f"soup-11-5, {label} vs reference")


# ---------------------------------------------------------------- 3. tree in global memory: node formats x builders
def test_tree_in_global_memory_formats_and_builders(luts, monkeypatch):
    from oracle.binding import Oracle
    w, h = 64, 40
    sc = _with_prev(random_soup(luts, 5000, 31, blend_fraction=.3, mask_fraction=.3, textured=True), 23)
    view, pos = TG._soup_view(w, h)
    prev_view, _ = scenes.planar_view(w, h, position=(0.2, 0.25, -5.1), yaw=0.05)
    cb = scenes.fill_constants(view, pos, sc, 2, 4)
    base, info = _device_motion(sc, cb, prev_view, w, h)
    assert info.triangleCount >= 4998 and info.node4Count * 128 + info.triangleCount * 48 > 64 * 1024
    o = Oracle(sc)
    try:
        tr = G.trace(sc, o, cb, w, h)
    finally:
        o.close()
    _assert_same(base, _reference(sc, cb, prev_view, w, h, tr), "5000-triangle soup vs reference")
    mega, _ = _device_motion(sc, cb, prev_view, w, h, S.FRAME_MEGAKERNEL)
    _assert_same(mega, base, "megakernel vs wavefront")
    for fmt in (1, 2):
        monkeypatch.setenv("HRPT_BVH_NODE_FORMAT", str(fmt))
        for builder in (S.BVH_BUILDER_HOST_SAH, S.BVH_BUILDER_GPU_LBVH, S.BVH_BUILDER_GPU_PLOC):
            got, bi = _device_motion(sc, cb, prev_view, w, h, prepare=lambda c: c.set_bvh_builder(builder))
            assert bi.usedBuilder == builder and bi.nodeFormat == fmt
            _assert_same(got, base, f"builder {builder}, node format {fmt}")


# ---------------------------------------------------------------- 4. the per-frame protocol
def _step(records, moved, rng, angle, shift):
    """One frame of the caller's protocol on a copy of `records`: m_PrevWorld <- m_World for ALL instances, then the instances in `moved` move."""
    out = records.copy()
    out["m_PrevWorld"] = out["m_World"]
    for k in moved:
        out["m_World"][k] = (out["m_World"][k].astype(np.float64) @ _rigid(rng, angle, shift)).astype(np.float32)
    return out


@pytest.mark.parametrize("structure", [S.ACCEL_FLAT, S.ACCEL_TWO_LEVEL])
def test_frame_protocol_keeps_the_tables_fresh(luts, monkeypatch, structure):
    """A: full-range hrpt_update_instances after the copy + move; B: hrpt_refit_instances with a GPU builder; C: a partial-range update of the
    moved instances only (the others keep the m_PrevWorld of step B). After each: motion == reference == a fresh context with the same records."""
    from hobbyrenderer_amd.native import PathTracerContext
    from oracle.binding import Oracle
    monkeypatch.setenv("HRPT_ACCEL_STRUCTURE", str(structure))
    w, h = 64, 40
    sc = TG._instanced(luts)
    view, pos = scenes.planar_view(w, h, position=(0.3, 4.5, -8.0), pitch=0.45)
    prev_view, _ = scenes.planar_view(w, h, position=(0.2, 4.5, -8.1), yaw=0.02, pitch=0.44)
    cb = scenes.fill_constants(view, pos, sc, 1, 4)
    rng = np.random.default_rng(5)
    n = len(sc.instances)
    third = list(range(1, n, 3))
    lo, hi = n - 40, n - 10                                      # step C's range
    ctx = PathTracerContext(0)
    try:
        ctx.set_bvh_builder(S.BVH_BUILDER_GPU_LBVH)
        ctx.upload_scene(sc)
        ctx.resize(w, h)
        ctx.render_motion_vectors(cb, prev_view)               # builds the tables before anything moves
        records = sc.instances.copy()
        for step in "ABC":
            if step == "A":
                records = _step(records, third, rng, 0.3, 0.2)
                ctx.update_instances(records, 0)
            elif step == "B":
                records = _step(records, third, rng, 0.02, 0.03)
                ctx.refit_instances(records, 0)
            else:
                nxt = _step(records, range(lo, hi), rng, 0.2, 0.15)
                records = records.copy(); records[lo:hi] = nxt[lo:hi]
                ctx.update_instances(records[lo:hi], lo)
            now = copy.copy(sc); now.instances = records.copy()
            ctx.render_motion_vectors(cb, prev_view)
            got = ctx.read_motion_vectors()
            fresh, _ = _device_motion(now, cb, prev_view, w, h, prepare=lambda c: c.set_bvh_builder(S.BVH_BUILDER_GPU_LBVH))
            _assert_same(got, fresh, f"step {step}, structure {structure}: updated context vs fresh upload")
            o = Oracle(now)
            try:
                tr = G.trace(now, o, cb, w, h)
            finally:
                o.close()
            _assert_same(got, _reference(now, cb, prev_view, w, h, tr), f"step {step}, structure {structure}: vs reference")
            moved_px = tr["hit"] & np.isin(tr["inst"], third if step != "C" else list(range(lo, hi)))
            assert moved_px.any()                               # moved instances are in view
    finally:
        ctx.close()


# ---------------------------------------------------------------- 5. planeMask
@pytest.mark.parametrize("label,flags", PATHS)
def test_plane_mask_shares_the_pass_with_the_gbuffer(luts, label, flags):
    from hobbyrenderer_amd.native import PathTracerContext
    sc0, cb, w, h, gref, tr = TG._case(luts, "soup-11-5")
    sc = _with_prev(sc0, 22)
    prev_view, _ = scenes.planar_view(w, h, position=(0.15, 0.35, -5.2), yaw=-0.04, pitch=0.02)
    nbytes = w * h * 16
    ctx = PathTracerContext(0)
    try:
        ctx.upload_scene(sc)
        ctx.resize(w, h)
        ctx.render_gbuffer(cb, flags=flags)
        planes = TG._read_all(ctx)
        TG._assert_same(planes, gref, f"hrpt_render_gbuffer, {label}")
        assert ctx.motion_vectors_device() is None              # ... and it never creates the motion plane
        # mask 0x3F: the six planes of hrpt_render_gbuffer, bit for bit, over sentinels
        for k in range(S.GB_PLANES):
            TG._fill_device(ctx.gbuffer_device(k), 0xCD, nbytes)
        ctx.render_motion_vectors(cb, prev_view, planes=S.GB_ALL_PLANES, flags=flags)
        mv_all = ctx.read_motion_vectors()
        TG._assert_same(TG._read_all(ctx), planes, f"planes written by the motion call, {label}")
        # mask 0: the planes keep the sentinels, the motion plane is the same
        for k in range(S.GB_PLANES):
            TG._fill_device(ctx.gbuffer_device(k), 0xCD, nbytes)
        TG._fill_device(ctx.motion_vectors_device(), 0xCD, nbytes)
        ctx.render_motion_vectors(cb, prev_view, flags=flags)
        mv = ctx.read_motion_vectors()
        _assert_same(mv, mv_all, f"motion with mask 0 vs mask 0x3F, {label}")
        for k in range(S.GB_PLANES):
            assert (_u32(ctx.read_gbuffer(k)) == SENTINEL).all(), TG.PLANE_NAMES[k]
        # a partial mask: only the named planes are written
        ctx.render_motion_vectors(cb, prev_view, planes=(1 << S.GB_NORMAL) | (1 << S.GB_IDS), flags=flags)
        for k in range(S.GB_PLANES):
            p = _u32(ctx.read_gbuffer(k))
            if k in (S.GB_NORMAL, S.GB_IDS):
                assert np.array_equal(p, _u32(planes[k])), TG.PLANE_NAMES[k]
            else:
                assert (p == SENTINEL).all(), TG.PLANE_NAMES[k]
        # hrpt_render_gbuffer leaves the motion plane alone
        TG._fill_device(ctx.motion_vectors_device(), 0xCD, nbytes)
        ctx.render_gbuffer(cb, flags=flags)
        assert (_u32(ctx.read_motion_vectors()) == SENTINEL).all()
    finally:
        ctx.close()
    _assert_same(mv, _reference(sc, cb, prev_view, w, h, tr), f"soup-11-5 through the shared pass, {label}")


# ---------------------------------------------------------------- 6. tiles and stripes
@pytest.mark.parametrize("label,flags", PATHS)
def test_tiles_stripes_and_sentinels(luts, label, flags):
    from hobbyrenderer_amd.native import PathTracerContext
    sc0, cb, w, h, _, tr = TG._case(luts, "cube")
    sc, prev_view = MC.scenario(sc0, cb, "both")
    ref = _u32(_reference(sc, cb, prev_view, w, h, tr))
    ctx = PathTracerContext(0)
    try:
        ctx.upload_scene(sc)
        ctx.resize(w, h)
        ctx.render_motion_vectors(cb, prev_view, flags=flags)
        ctx.synchronize()
        # one unaligned tile: everything outside keeps the sentinel written through the device pointer
        TG._fill_device(ctx.motion_vectors_device(), 0xCD, w * h * 16)
        tile = (13, 5, 42, 30)
        ctx.render_motion_vectors(cb, prev_view, tile=tile, flags=flags)
        inside = np.zeros((h, w), bool); inside[tile[1]:tile[3], tile[0]:tile[2]] = True
        g = _u32(ctx.read_motion_vectors())
        assert np.array_equal(g[inside], ref[inside]) and (g[~inside] == SENTINEL).all()
        # four unaligned tiles, the last one split into three stripes, reproduce the full frame
        TG._fill_device(ctx.motion_vectors_device(), 0xCD, w * h * 16)
        for t in ((0, 0, 27, 19), (27, 0, w, 19), (0, 19, 35, h)):
            ctx.render_motion_vectors(cb, prev_view, tile=t, flags=flags)
        for s in range(3):
            ctx.render_motion_vectors(cb, prev_view, tile=(35, 19, w, h), flags=flags, stripes=(3, s))
        assert np.array_equal(_u32(ctx.read_motion_vectors()), ref), f"tiles + stripes, {label}"
    finally:
        ctx.close()


# ---------------------------------------------------------------- 7. isolation
@pytest.mark.parametrize("label,flags", PATHS)
def test_renders_do_not_notice_a_motion_call(luts, label, flags):
    from hobbyrenderer_amd.native import PathTracerContext
    from oracle.binding import Oracle
    w, h = 64, 36
    sc, view, pos, cfg = scenes.config_cornell(luts, w, h, extra_lights=True)
    constants = lambda i: scenes.fill_constants(view, pos, sc, i, cfg["max_bounces"])       # noqa: E731
    prev_view, _ = scenes.planar_view(w, h, position=(0.05, 1.0, -3.4), yaw=0.02)
    ctx = PathTracerContext(0)
    try:
        ctx.upload_scene(sc)
        ctx.resize(w, h)
        ctx.render(constants(0), accum_count=2)
        before = (ctx.read_accumulation(), ctx.read_output(), ctx.stats())
        cb = constants(7); cb["m_Jitter"] = (0.0, 0.0)
        ctx.render_motion_vectors(cb, prev_view, planes=1 << S.GB_DEPTH, flags=flags)
        mv = ctx.read_motion_vectors()
        after = (ctx.read_accumulation(), ctx.read_output(), ctx.stats())
        assert np.array_equal(_u32(before[0]), _u32(after[0])) and np.array_equal(_u32(before[1]), _u32(after[1]))
        for field, _ in S.Stats._fields_:
            assert getattr(before[2], field) == getattr(after[2], field), field
        assert (mv[..., 3] == 1).all() and np.abs(mv[..., :2]).max() > 0.1                 # a closed room: every primary ray hits; the camera moved
        ctx.render(constants(2), accum_count=2)
        acc = ctx.read_accumulation()
    finally:
        ctx.close()
    o = Oracle(sc)
    try:
        oacc, _ = o.render_accumulated(constants, w, h, 4)
    finally:
        o.close()
    assert np.array_equal(_u32(acc), _u32(oacc))


# ---------------------------------------------------------------- 8. errors and resize
def test_errors_and_resize(luts):
    from hobbyrenderer_amd.native import PathTracerContext, HrptError, lib
    from oracle.binding import Oracle
    sc0, cb, w, h, _, _ = TG._case(luts, "cube")
    sc, prev_view = MC.scenario(sc0, cb, "both")
    pv = np.ascontiguousarray(prev_view)
    ctx = PathTracerContext(0)
    try:
        p = np.zeros((), S.FrameParams); p["constants"] = cb; p["accumCount"] = 1
        assert lib.hrpt_render_motion_vectors(ctx._h, p.ctypes.data, pv.ctypes.data, 0) == -4      # HRPT_ERR_NO_SCENE
        ctx.upload_scene(sc)
        ctx.resize(w, h)
        for mask in (1 << S.GB_PLANES, 0x80000000, 0xFFFFFFFF):
            assert lib.hrpt_render_motion_vectors(ctx._h, p.ctypes.data, pv.ctypes.data, mask) == -1
        assert lib.hrpt_render_motion_vectors(ctx._h, p.ctypes.data, None, 0) == -1                # NULL prevView
        assert lib.hrpt_render_motion_vectors(ctx._h, None, pv.ctypes.data, 0) == -1               # NULL params
        p["accumCount"] = 2
        assert lib.hrpt_render_motion_vectors(ctx._h, p.ctypes.data, pv.ctypes.data, 0) == -1
        p["accumCount"] = 0
        assert lib.hrpt_render_motion_vectors(ctx._h, p.ctypes.data, pv.ctypes.data, 0) == -1
        assert lib.hrpt_render_gbuffer(ctx._h, p.ctypes.data, 1 << S.GB_PLANES) == -1              # bit 6 stays an error of the G-buffer call
        # nothing requested so far: no plane, reading is an error
        assert ctx.motion_vectors_device() is None
        with pytest.raises(HrptError) as e:
            ctx.read_motion_vectors()
        assert e.value.code == -1 and "never requested" in str(e.value)
        assert all(ctx.gbuffer_device(k) is None for k in range(S.GB_PLANES))
        ctx.render_motion_vectors(cb, prev_view)
        assert ctx.motion_vectors_device() and all(ctx.gbuffer_device(k) is None for k in range(S.GB_PLANES))
        buf = np.zeros(4, np.float32)
        assert lib.hrpt_read_motion_vectors(ctx._h, buf.ctypes.data, buf.nbytes) == -1              # bytes != W * H * 16
        assert lib.hrpt_get_motion_vectors_device(ctx._h, None) == -1
        assert ctx.stats().queuePoolBytes == 0                                                     # a statistic of renders
        # hrpt_resize: the plane follows the new size, zeroed
        w2, h2 = 40, 24
        _, cb3 = G.cube_case(luts, w2, h2, 3, (0.25, -0.125))
        yaw, pitch = math.atan2(-2.0, 3.0), math.asin(1.5 / math.sqrt(15.25))
        prev3, _ = scenes.planar_view(w2, h2, position=(2.3, 1.2, -3.4), yaw=yaw + 0.06, pitch=pitch - 0.03)
        ctx.resize(w2, h2)
        assert ctx.read_motion_vectors().shape == (h2, w2, 4) and not _u32(ctx.read_motion_vectors()).any()
        o = Oracle(sc)
        try:
            tr3 = G.trace(sc, o, cb3, w2, h2)
        finally:
            o.close()
        ref3 = _reference(sc, cb3, prev3, w2, h2, tr3)
        for label, flags in PATHS:
            ctx.render_motion_vectors(cb3, prev3, flags=flags)
            _assert_same(ctx.read_motion_vectors(), ref3, f"after hrpt_resize, {label}")
    finally:
        ctx.close()
