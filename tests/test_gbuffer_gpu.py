"""First-hit G-buffer on the device (hrpt_render_gbuffer): all six planes, bit for bit on uint32 views, against the NumPy
reference (tests/gbuffer_reference.py), against the render path's own ray query, across acceleration structures, tiles and plane masks, and
without a trace in what renders leave behind."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

from hobbyrenderer_amd import scenes, structs as S
from scene_helpers import random_soup
import gbuffer_reference as G

pytestmark = pytest.mark.gpu

PLANE_NAMES = ["albedo", "normal", "geo_normal", "emissive", "depth", "ids"]
PATHS = [("wavefront", S.FRAME_WAVEFRONT), ("megakernel", S.FRAME_MEGAKERNEL)]


def _read_all(ctx):
    return [ctx.read_gbuffer(k) for k in range(S.GB_PLANES)]


def _device_planes(sc, cb, w, h, flags=S.FRAME_DEFAULT, prepare=None):
    from hobbyrenderer_amd.native import PathTracerContext
    ctx = PathTracerContext(0)
    try:
        if prepare:
            prepare(ctx)
        ctx.upload_scene(sc)
        ctx.resize(w, h)
        ctx.render_gbuffer(cb, flags=flags)
        return _read_all(ctx), ctx.build_info()
    finally:
        ctx.close()


def _assert_same(got, want, what):
    for k in range(S.GB_PLANES):
        a, b = np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)
        bad = (a != b).any(-1)
        if bad.any():
            y, x = np.argwhere(bad)[0]
            raise AssertionError(f"{what}: plane {PLANE_NAMES[k]}: {int(bad.sum())} of {bad.size} pixels differ, first at (x={x}, y={y}): "
                                 f"{got[k][y, x]} != {want[k][y, x]}")


def _soup_view(w, h):
    return scenes.planar_view(w, h, position=(0.0, 0.3, -5.0))


_CASES = {}


def _case(luts, name):
    """(scene, constants, w, h, reference planes, reference trace), computed once per session."""
    if name in _CASES:
        return _CASES[name]
    from oracle.binding import Oracle
    if name == "cube":
        w, h = 61, 37                                          # partial 8 x 8 tiles on both axes
        sc, cb = G.cube_case(luts, w, h, 3, (0.25, -0.125))
    elif name == "cornell":
        w, h = 96, 64
        sc, view, pos, cfg = scenes.config_cornell(luts, w, h, extra_lights=True)
        cb = scenes.fill_constants(view, pos, sc, 1, cfg["max_bounces"])
    else:                                                      # soup-<seed>-<index>
        _, seed, index = name.split("-")
        w, h = 80, 48
        sc = random_soup(luts, 600, int(seed), blend_fraction=.3, mask_fraction=.3, textured=True)
        view, pos = _soup_view(w, h)
        cb = scenes.fill_constants(view, pos, sc, int(index), 4)
    o = Oracle(sc)
    try:
        tr = G.trace(sc, o, cb, w, h)
        ref = G.gbuffer(sc, o, cb, w, h, traced=tr)
    finally:
        o.close()
    _CASES[name] = (sc, cb, w, h, ref, tr)
    return _CASES[name]


SOUPS = ["soup-11-0", "soup-11-5", "soup-12-0", "soup-12-5"]


@pytest.mark.parametrize("name", ["cube", "cornell"] + SOUPS)
def test_device_equals_reference(luts, name):
    sc, cb, w, h, ref, tr = _case(luts, name)
    hit = tr["hit"]
    assert 0.05 * hit.size < hit.sum() and (name == "cornell" or hit.sum() < 0.95 * hit.size), "the case must exercise hits and misses"
    if name.startswith("soup"):
        # first surfaces: the normal-mapped PBR material, textured MASK, textured stochastic BLEND, constant stochastic BLEND, thick glass
        seen = set(np.unique(ref[S.GB_IDS][hit][:, 2]).tolist())
        assert {1, 2, 3, 4, 5} <= seen, seen
        assert (tr["rng"] != tr["seed"]).any()                 # BLEND candidates drew from the path's RNG
        n, ng = ref[S.GB_NORMAL][hit][:, :3], ref[S.GB_GEO_NORMAL][hit][:, :3]
        assert (n != ng).any(1).sum() > 20                     # normal maps and flips at work
    for label, flags in PATHS:
        got, _ = _device_planes(sc, cb, w, h, flags)
        _assert_same(got, ref, f"{name}, {label} vs reference")


@pytest.mark.parametrize("name", ["soup-11-0", "soup-12-5"])
def test_gbuffer_is_the_surface_the_render_path_traces(luts, name):
    """The DEPTH / IDS planes against hrpt_trace_rays (closest hit, TraceRayStandard) on primary rays and seeds built here in NumPy."""
    from hobbyrenderer_amd.native import PathTracerContext
    sc, cb, w, h, ref, tr = _case(luts, name)
    o, d, seed = G.primary_rays(cb, w, h)
    rays = np.zeros(w * h, S.Ray)
    rays["origin"] = o; rays["direction"] = d.reshape(-1, 3); rays["tmin"] = 0.0; rays["tmax"] = np.float32(1e10); rays["rng"] = seed.reshape(-1)
    ctx = PathTracerContext(0)
    try:
        ctx.upload_scene(sc)
        ctx.resize(w, h)
        hits = ctx.trace_rays(rays).reshape(h, w)
        ctx.render_gbuffer(cb, planes=(1 << S.GB_DEPTH) | (1 << S.GB_IDS))
        depth, ids = ctx.read_gbuffer(S.GB_DEPTH), ctx.read_gbuffer(S.GB_IDS)
    finally:
        ctx.close()
    hit = hits["hit"] != 0
    assert np.array_equal(hit, (ids[..., 3] & S.GB_FLAG_HIT) != 0) and 0 < hit.sum() < hit.size
    for field, plane in (("t", depth[..., 0]), ("u", depth[..., 2]), ("v", depth[..., 3])):
        assert np.array_equal(hits[field][hit].view(np.uint32), plane[hit].view(np.uint32)), field
    assert np.array_equal(hits["instance"][hit], ids[..., 0][hit]) and np.array_equal(hits["primitive"][hit], ids[..., 1][hit])
    assert (depth[..., 0][~hit] == np.float32(1e10)).all() and (ids[..., :3][~hit] == 0xFFFFFFFF).all()


# ---------------------------------------------------------------- structures
def test_tree_in_global_memory_formats_builders_and_width(luts, monkeypatch):
    """A 5 000-triangle soup (its tree does not fit LDS): fp32 and quantised nodes, both GPU builders and the host builder, the 2-wide kernels --
    every structure gives the planes of the default one, and the default gives the reference's."""
    from oracle.binding import Oracle
    w, h = 64, 40
    sc = random_soup(luts, 5000, 31, blend_fraction=.3, mask_fraction=.3, textured=True)
    view, pos = _soup_view(w, h)
    cb = scenes.fill_constants(view, pos, sc, 2, 4)
    base, info = _device_planes(sc, cb, w, h)
    assert info.triangleCount >= 4998 and info.node4Count * 128 + info.triangleCount * 48 > 64 * 1024        # beyond the LDS budget of the trace kernels
    o = Oracle(sc)
    try:
        _assert_same(base, G.gbuffer(sc, o, cb, w, h), "5000-triangle soup vs reference")
    finally:
        o.close()
    mega, _ = _device_planes(sc, cb, w, h, S.FRAME_MEGAKERNEL)
    _assert_same(mega, base, "megakernel vs wavefront")
    for fmt in (1, 2):
        monkeypatch.setenv("HRPT_BVH_NODE_FORMAT", str(fmt))
        got, bi = _device_planes(sc, cb, w, h)
        assert bi.nodeFormat == fmt
        _assert_same(got, base, f"HRPT_BVH_NODE_FORMAT={fmt}")
        for builder in (S.BVH_BUILDER_GPU_LBVH, S.BVH_BUILDER_GPU_PLOC, S.BVH_BUILDER_HOST_SAH):
            got, bi = _device_planes(sc, cb, w, h, prepare=lambda c: c.set_bvh_builder(builder))
            assert bi.usedBuilder == builder and bi.nodeFormat == fmt
            _assert_same(got, base, f"builder {builder}, node format {fmt}")
    monkeypatch.delenv("HRPT_BVH_NODE_FORMAT")
    monkeypatch.setenv("HRPT_WF_BVH_WIDTH", "2")
    got, _ = _device_planes(sc, cb, w, h)
    _assert_same(got, base, "HRPT_WF_BVH_WIDTH=2")


def _instanced(luts):
    """64 instances of a 200-triangle sphere, every third alpha-tested against a texture, over a floor."""
    rng = np.random.default_rng(9)
    b = scenes.SceneBuilder()
    sphere = b.add_mesh(*scenes.mesh_sphere(10, 10, 0.5))
    quad = b.add_mesh(*scenes.generate_floor_quad())
    tex = b.add_texture(scenes.procedural_texture(rng, 32, "alpha"))
    mats = [b.add_material(m_BaseColor=(0.8, 0.3, 0.2, 1), m_RoughnessMetallic=(0.4, 0.0)),
            b.add_material(m_BaseColor=(0.9, 0.8, 0.3, 1), m_RoughnessMetallic=(0.2, 1.0), m_EmissiveFactor=(0.2, 0.1, 0.0, 1)),
            b.add_material(m_BaseColor=(1, 1, 1, 1), m_TextureFlags=S.TEXFLAG_ALBEDO, m_AlbedoTextureIndex=tex, m_AlphaMode=S.ALPHA_MODE_MASK, m_AlphaCutoff=0.5)]
    b.add_instance(quad, mats[0], scenes._mat((14, 1, 14), None, (0, 0, 0)))
    for i in range(8):
        for j in range(8):
            a = rng.uniform(0, 2 * math.pi)
            rot = [[math.cos(a), 0, -math.sin(a)], [0, 1, 0], [math.sin(a), 0, math.cos(a)]]
            b.add_instance(sphere, mats[(i * 8 + j) % 3], scenes._mat(tuple(rng.uniform(0.6, 1.2, 3)), rot, ((i - 3.5) * 1.3, 0.5 + rng.uniform(0, 1.0), (j - 3.5) * 1.3)))
    return b.finalize(luts)


def _moved(sc, first, count):
    out = copy.copy(sc)
    inst = sc.instances.copy()
    for k in range(first, first + count):
        a = 0.3 + 0.05 * k
        rot = np.array([[math.cos(a), 0, -math.sin(a), 0], [0, 1, 0, 0], [math.sin(a), 0, math.cos(a), 0], [0, 0, 0, 1]], np.float64)
        rot[3, :3] = (0.1, 0.05 * (k % 3), -0.08)
        inst["m_World"][k] = (inst["m_World"][k].astype(np.float64) @ rot).astype(np.float32)
    out.instances = inst
    return out


def test_instanced_scene_two_level_flat_and_instance_updates(luts, monkeypatch):
    from hobbyrenderer_amd.native import PathTracerContext
    from oracle.binding import Oracle
    w, h = 64, 40
    sc = _instanced(luts)
    view, pos = scenes.planar_view(w, h, position=(0.3, 4.5, -8.0), pitch=0.45)
    cb = scenes.fill_constants(view, pos, sc, 1, 4)
    planes = {}
    for structure in (S.ACCEL_FLAT, S.ACCEL_TWO_LEVEL):
        monkeypatch.setenv("HRPT_ACCEL_STRUCTURE", str(structure))
        for label, flags in PATHS:
            planes[structure, label], bi = _device_planes(sc, cb, w, h, flags)
            assert bi.structure == structure
    o = Oracle(sc)
    try:
        ref = G.gbuffer(sc, o, cb, w, h)
    finally:
        o.close()
    assert len(np.unique(ref[S.GB_IDS][..., 0])) > 20 and 2 in ref[S.GB_IDS][..., 2]          # many instances in view, alpha-tested ones among them
    for key, got in planes.items():
        _assert_same(got, ref, f"instanced scene, structure {key[0]}, {key[1]} vs reference")
    # hrpt_update_instances, then the same call: the planes of a fresh upload of the moved scene
    n = len(sc.instances)
    moved = _moved(sc, n - 40, 30)
    for structure in (S.ACCEL_FLAT, S.ACCEL_TWO_LEVEL):
        monkeypatch.setenv("HRPT_ACCEL_STRUCTURE", str(structure))
        fresh, _ = _device_planes(moved, cb, w, h)
        ctx = PathTracerContext(0)
        try:
            ctx.upload_scene(sc)
            ctx.resize(w, h)
            ctx.render_gbuffer(cb)
            ctx.update_instances(moved.instances[n - 40:n - 10], n - 40)
            ctx.render_gbuffer(cb)
            got = _read_all(ctx)
        finally:
            ctx.close()
        _assert_same(got, fresh, f"after hrpt_update_instances, structure {structure}")
        assert (np.ascontiguousarray(fresh[S.GB_DEPTH]).view(np.uint32) != np.ascontiguousarray(planes[structure, "wavefront"][S.GB_DEPTH]).view(np.uint32)).any()


# ---------------------------------------------------------------- tiles, masks, errors
def _fill_device(ptr, byte, nbytes):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    assert hip.hipMemset(C.c_void_p(ptr), byte, nbytes) == 0 and hip.hipDeviceSynchronize() == 0


@pytest.mark.parametrize("label,flags", PATHS)
def test_tiles_stripes_and_sentinels(luts, label, flags):
    from hobbyrenderer_amd.native import PathTracerContext
    sc, cb, w, h, ref, _ = _case(luts, "cube")
    sentinel = np.uint32(0xCDCDCDCD)
    ctx = PathTracerContext(0)
    try:
        ctx.upload_scene(sc)
        ctx.resize(w, h)
        ctx.render_gbuffer(cb, flags=flags)
        ctx.synchronize()
        # one unaligned tile: everything outside keeps the sentinel written through the device pointer
        for k in range(S.GB_PLANES):
            _fill_device(ctx.gbuffer_device(k), 0xCD, w * h * 16)
        tile = (13, 5, 42, 30)
        ctx.render_gbuffer(cb, tile=tile, flags=flags)
        inside = np.zeros((h, w), bool); inside[tile[1]:tile[3], tile[0]:tile[2]] = True
        for k, got in enumerate(_read_all(ctx)):
            g, r = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(ref[k]).view(np.uint32)
            assert np.array_equal(g[inside], r[inside]), PLANE_NAMES[k]
            assert (g[~inside] == sentinel).all(), PLANE_NAMES[k]
        # four unaligned tiles, the last one split into three stripes, reproduce the full frame
        for k in range(S.GB_PLANES):
            _fill_device(ctx.gbuffer_device(k), 0xCD, w * h * 16)
        for t in ((0, 0, 27, 19), (27, 0, w, 19), (0, 19, 35, h)):
            ctx.render_gbuffer(cb, tile=t, flags=flags)
        for s in range(3):
            ctx.render_gbuffer(cb, tile=(35, 19, w, h), flags=flags, stripes=(3, s))
        _assert_same(_read_all(ctx), ref, f"tiles + stripes, {label}")
    finally:
        ctx.close()


def test_plane_masks_errors_and_resize(luts):
    from hobbyrenderer_amd.native import PathTracerContext, HrptError, lib
    from oracle.binding import Oracle
    sc, cb, w, h, ref, _ = _case(luts, "cube")
    cb2 = cb.copy(); cb2["m_Jitter"] = (-0.375, 0.3125); cb2["m_AccumulationIndex"] = 4
    ctx = PathTracerContext(0)
    o = Oracle(sc)
    try:
        p = np.zeros((), S.FrameParams); p["constants"] = cb; p["accumCount"] = 1
        assert lib.hrpt_render_gbuffer(ctx._h, p.ctypes.data, S.GB_ALL_PLANES) == -4                  # no scene: hrpt_render's code
        ctx.upload_scene(sc)
        ctx.resize(w, h)
        assert ctx.stats().queuePoolBytes == 0
        for mask in (0, 1 << S.GB_PLANES, 0x80000001):
            assert lib.hrpt_render_gbuffer(ctx._h, p.ctypes.data, mask) == -1
        p["accumCount"] = 2
        assert lib.hrpt_render_gbuffer(ctx._h, p.ctypes.data, S.GB_ALL_PLANES) == -1
        assert lib.hrpt_render_gbuffer(ctx._h, None, S.GB_ALL_PLANES) == -1
        # nothing requested so far: no plane exists
        assert all(ctx.gbuffer_device(k) is None for k in range(S.GB_PLANES))
        ctx.render_gbuffer(cb, planes=(1 << S.GB_ALBEDO) | (1 << S.GB_DEPTH))
        with pytest.raises(HrptError) as e:
            ctx.read_gbuffer(S.GB_NORMAL)
        assert e.value.code == -1 and "never requested" in str(e.value)
        assert ctx.gbuffer_device(S.GB_NORMAL) is None and ctx.gbuffer_device(S.GB_ALBEDO)
        buf = np.zeros(4, np.float32)
        assert lib.hrpt_read_gbuffer(ctx._h, S.GB_ALBEDO, buf.ctypes.data, buf.nbytes) == -1          # bytes != W * H * 16
        assert lib.hrpt_read_gbuffer(ctx._h, S.GB_PLANES, buf.ctypes.data, buf.nbytes) == -1
        # a masked-out plane keeps its previous contents
        ctx.render_gbuffer(cb)
        ctx.render_gbuffer(cb2, planes=(1 << S.GB_ALBEDO) | (1 << S.GB_NORMAL))
        ref2 = G.gbuffer(sc, o, cb2, w, h)
        assert (ref2[S.GB_NORMAL].view(np.uint32) != ref[S.GB_NORMAL].view(np.uint32)).any()
        _assert_same(_read_all(ctx), [ref2[0], ref2[1]] + ref[2:], "second call with albedo + normal only")
        assert ctx.stats().queuePoolBytes == 0                                                        # a statistic of renders
        # hrpt_resize: the requested planes follow the new size
        w2, h2 = 40, 24
        _, cb3 = G.cube_case(luts, w2, h2, 3, (0.25, -0.125))
        ctx.resize(w2, h2)
        assert not ctx.read_gbuffer(S.GB_IDS).any()
        for label, flags in PATHS:
            ctx.render_gbuffer(cb3, flags=flags)
            _assert_same(_read_all(ctx), G.gbuffer(sc, o, cb3, w2, h2), f"after hrpt_resize, {label}")
    finally:
        o.close(); ctx.close()


# ---------------------------------------------------------------- isolation
@pytest.mark.parametrize("label,flags", PATHS)
def test_renders_do_not_notice_a_gbuffer_call(luts, label, flags):
    from hobbyrenderer_amd.native import PathTracerContext
    from oracle.binding import Oracle
    w, h = 64, 36
    sc, view, pos, cfg = scenes.config_cornell(luts, w, h, extra_lights=True)
    constants = lambda i: scenes.fill_constants(view, pos, sc, i, cfg["max_bounces"])       # noqa: E731
    ctx = PathTracerContext(0)
    try:
        ctx.upload_scene(sc)
        ctx.resize(w, h)
        ctx.render(constants(0), accum_count=2)
        before = (ctx.read_accumulation(), ctx.read_output(), ctx.stats())
        cb = constants(7); cb["m_Jitter"] = (0.0, 0.0)
        ctx.render_gbuffer(cb, flags=flags)
        planes = _read_all(ctx)
        after = (ctx.read_accumulation(), ctx.read_output(), ctx.stats())
        assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
        for field, _ in S.Stats._fields_:
            assert getattr(before[2], field) == getattr(after[2], field), field
        assert (planes[S.GB_IDS][..., 3] & S.GB_FLAG_HIT).all()                                   # a closed room: every primary ray hits
        ctx.render(constants(2), accum_count=2)
        acc = ctx.read_accumulation()
    finally:
        ctx.close()
    o = Oracle(sc)
    try:
        oacc, _ = o.render_accumulated(constants, w, h, 4)
    finally:
        o.close()
    assert np.array_equal(acc.view(np.uint32), oacc.view(np.uint32))
