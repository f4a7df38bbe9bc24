"""hrpt_trace_radiance: path-traced radiance along rays the caller made. Camera rays built here in NumPy reproduce the
oracle's render of the same index bit for bit, so do six-face interior probes in shuffled order and accumulated indices; the wavefront
pipeline and the one-thread-per-ray kernel agree byte for byte on random rays, in one batch and in many, over flat and two-level
structures; non-finite rays, device pointers, the argument checks, and nothing of it leaves a trace in what renders see.

Every comparison is of bits and covers every ray."""
import math

import numpy as np
import pytest

from hobbyrenderer_amd import scenes, structs as S
from scene_helpers import random_soup
import gbuffer_reference as G

pytestmark = pytest.mark.gpu

W, H = 61, 37                       # 2 257 rays: no multiple of 64, across 1 024-sample segments
PATHS = [("wavefront", False), ("thread-per-ray", True)]
SCENES = ["cornell", "soup", "glass"]
_CACHE = {}


def _scene(luts, name):
    """(scene, view, camera position, bounces) at W x H, built once per session."""
    key = ("scene", name)
    if key not in _CACHE:
        if name == "cornell":
            sc, view, pos, _ = scenes.config_cornell(luts, W, H, extra_lights=True)
            bounces = 4
        elif name == "soup":
            sc = random_soup(luts, 500, 21, 0.5, 0.3, True)       # BLEND (stochastic alpha, glass), MASK, textures, a point light
            view, pos = scenes.planar_view(W, H, position=(0.0, 0.3, -5.0))
            bounces = 4
        elif name == "glass":
            sc, view, pos, _ = scenes.config_glass(luts, W, H, detail=0.5)
            bounces = 6
        else:
            sc, view, pos, _ = scenes.config_sponza_class(luts, 64, 36)       # ~100 k triangles: tree in global memory, overflow stacks
            bounces = 3
        _CACHE[key] = (sc, view, pos, bounces)
    return _CACHE[key]


def _rays_of(cb, w, h):
    """The primary rays of every pixel for `cb` as S.Ray records, row-major."""
    o, d, seed = G.primary_rays(cb, w, h)
    rays = np.zeros(w * h, S.Ray)
    rays["origin"] = o; rays["direction"] = d.reshape(-1, 3); rays["tmin"] = 0.0; rays["tmax"] = np.float32(1e10); rays["rng"] = seed.reshape(-1)
    return rays


def _oracle_index(luts, name, index):
    """(rays, Accumulation of the oracle's or_render of `index` alone on a cleared image, flattened) for the scene's camera."""
    key = ("index", name, index)
    if key not in _CACHE:
        from oracle.binding import Oracle
        sc, view, pos, bounces = _scene(luts, name)
        cb = scenes.fill_constants(view, pos, sc, index, bounces)
        acc, out = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
        o = Oracle(sc)
        try:
            o.render(cb, acc, out)
        finally:
            o.close()
        _CACHE[key] = (_rays_of(cb, W, H), acc.reshape(-1, 4), cb)
    return _CACHE[key]


def _context(sc, structure=None):
    from hobbyrenderer_amd.native import PathTracerContext
    ctx = PathTracerContext(0)
    try:
        if structure is not None:
            ctx.set_acceleration_structure(structure)
        ctx.upload_scene(sc)
    except Exception:
        ctx.close()
        raise
    return ctx


def _assert_bits(got, want, what):
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = (a != b).any(-1)
    if bad.any():
        i = int(np.argwhere(bad)[0][0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} rays differ, first at {i}: {got[i]} != {want[i]}")


def _random_rays(rng, n, extent=2.5):
    """tests/test_ray_queries_gpu.py _rays: origins in a cube, unit directions, tmin in {0, 1e-4}, random RNG states."""
    r = np.zeros(n, S.Ray)
    r["origin"] = (rng.random((n, 3)).astype(np.float32) - np.float32(0.5)) * np.float32(2 * extent)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.sqrt((d.astype(np.float64) ** 2).sum(1, keepdims=True)).astype(np.float32)
    r["direction"] = d
    r["tmin"] = np.where(rng.random(n) < 0.5, 0.0, 1e-4).astype(np.float32)
    r["tmax"] = np.where(rng.random(n) < 0.7, 1e10, rng.random(n) * 4).astype(np.float32)      # ignored by the call
    r["rng"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    return r


# ---------------------------------------------------------------- 1. camera rays reproduce the render
@pytest.mark.parametrize("index", [0, 5])
@pytest.mark.parametrize("name", SCENES)
def test_camera_rays_reproduce_the_render(luts, name, index):
    rays, want, cb = _oracle_index(luts, name, index)
    assert (want[:, 3] == 1.0).all() and (want[:, :3] > 0).any()
    ctx = _context(_scene(luts, name)[0])
    try:
        for label, tpr in PATHS:
            got = ctx.trace_radiance(rays, cb, thread_per_ray=tpr)
            _assert_bits(got, want, f"{name}, index {index}, {label} vs the oracle's Accumulation")
    finally:
        ctx.close()


# ---------------------------------------------------------------- 2. rays that are not the camera's
FACES = [(math.pi / 2, 0.0), (-math.pi / 2, 0.0), (0.0, -math.pi / 2), (0.0, math.pi / 2), (0.0, 0.0), (math.pi, 0.0)]      # (yaw, pitch): +x -x +y -y +z -z


@pytest.mark.parametrize("name,position", [("cornell", (0.1, 1.0, -1.2)), ("soup", (0.05, 0.1, -0.05))])
def test_six_face_probe_in_shuffled_order(luts, name, position):
    from oracle.binding import Oracle
    sc, _, _, bounces = _scene(luts, name)
    n, index = 8, 2
    rays, want, cb = [], [], None
    o = Oracle(sc)
    try:
        for yaw, pitch in FACES:
            view, pos = scenes.planar_view(n, n, position=position, yaw=yaw, pitch=pitch, fov_y=math.pi / 2, aspect=1.0)
            cb = scenes.fill_constants(view, pos, sc, index, bounces)
            acc, out = np.zeros((n, n, 4), np.float32), np.zeros((n, n, 4), np.float32)
            o.render(cb, acc, out)
            rays.append(_rays_of(cb, n, n)); want.append(acc.reshape(-1, 4))
    finally:
        o.close()
    rays, want = np.concatenate(rays), np.concatenate(want)
    assert len(rays) == 384
    d = rays["direction"].reshape(6, 64, 3).mean(1)
    assert sorted(int(np.argmax(np.abs(v))) * 2 + int(v[np.argmax(np.abs(v))] < 0) for v in d) == [0, 1, 2, 3, 4, 5]      # the six faces look along +-x, +-y, +-z
    perm = np.random.default_rng(3).permutation(len(rays))
    ctx = _context(sc)
    try:
        for label, tpr in PATHS:
            got = ctx.trace_radiance(rays[perm], cb, thread_per_ray=tpr)        # (view and camera of cb are those of the last face: not read)
            _assert_bits(got, want[perm], f"{name} probe, {label} vs six oracle renders")
    finally:
        ctx.close()


# ---------------------------------------------------------------- 3. accumulate
def test_accumulate_equals_progressive_accumulation(luts):
    from oracle.binding import Oracle
    sc, view, pos, bounces = _scene(luts, "cornell")
    constants = lambda i: scenes.fill_constants(view, pos, sc, i, bounces)       # noqa: E731
    o = Oracle(sc)
    try:
        want, _ = o.render_accumulated(constants, W, H, spp=3)
    finally:
        o.close()
    ctx = _context(sc)
    try:
        for label, tpr in PATHS:
            out = ctx.trace_radiance(_rays_of(constants(0), W, H), constants(0), thread_per_ray=tpr)
            for i in (1, 2):
                back = ctx.trace_radiance(_rays_of(constants(i), W, H), constants(i), accumulate=True, thread_per_ray=tpr, out=out)
                assert back is out
            assert (out[:, 3] == 3.0).all()
            _assert_bits(out, want.reshape(-1, 4), f"three indices accumulated, {label}")
    finally:
        ctx.close()


# ---------------------------------------------------------------- 4. two schedules agree
@pytest.mark.parametrize("schedule", ["one-batch", "batches-of-1024", "two-level"])
@pytest.mark.parametrize("name", SCENES + ["sponza"])
def test_wavefront_and_thread_per_ray_agree(luts, monkeypatch, name, schedule):
    """20 011 random rays: 20 segments of 1 024 with a ragged last one; with HRPT_RADIANCE_BATCH=1024 twenty batches, the last of 555 rays."""
    sc, view, pos, bounces = _scene(luts, name)
    cb = scenes.fill_constants(view, pos, sc, 0, bounces)
    rays = _random_rays(np.random.default_rng(17), 20011, extent=3.0)
    if schedule == "batches-of-1024":
        monkeypatch.setenv("HRPT_RADIANCE_BATCH", "1024")
    ctx = _context(sc, S.ACCEL_TWO_LEVEL if schedule == "two-level" else None)
    try:
        assert schedule != "two-level" or ctx.build_info().structure == S.ACCEL_TWO_LEVEL
        a = ctx.trace_radiance(rays, cb)
        b = ctx.trace_radiance(rays, cb, thread_per_ray=True)
    finally:
        ctx.close()
    assert (a[:, 3] == 1.0).all() and (a[:, :3] > 0).any(1).sum() > 1000       # every ray traced, light arrives along many
    _assert_bits(a, b, f"{name}, {schedule}: wavefront vs thread per ray")
    key = ("random", name)              # ... and every schedule and structure gives the same bytes
    _assert_bits(a, _CACHE.setdefault(key, a), f"{name}, {schedule} vs the first schedule run")


# ---------------------------------------------------------------- 5. non-finite rays
@pytest.mark.parametrize("label,tpr", PATHS)
def test_non_finite_rays(luts, label, tpr):
    sc, view, pos, bounces = _scene(luts, "cornell")
    cb = scenes.fill_constants(view, pos, sc, 0, bounces)
    rays = _random_rays(np.random.default_rng(9), 1500)
    bad = [0, 63, 64, len(rays) - 1]
    rays["origin"][0] = (np.nan, 0, 0); rays["direction"][63] = (0, np.inf, 0); rays["tmin"][64] = np.nan
    rays["origin"][-1] = (0, -np.inf, 0); rays["direction"][-1] = (np.nan, np.nan, np.nan); rays["tmin"][-1] = np.inf
    good = np.ones(len(rays), bool); good[bad] = False
    ctx = _context(sc)
    try:
        without = ctx.trace_radiance(rays[good], cb, thread_per_ray=tpr)
        got = ctx.trace_radiance(rays, cb, thread_per_ray=tpr)
        assert not got[bad].view(np.uint32).any()                                # (0, 0, 0, 0), positive zeros
        _assert_bits(got[good], without, f"{label}: the finite rays next to non-finite ones")
        # ACCUMULATE: the slots of non-finite rays keep their bits, the others take prev + (L, 1)
        prev = (np.arange(len(rays) * 4, dtype=np.float32).reshape(-1, 4) * np.float32(0.125)) + np.float32(0.5)
        prev[bad[1]] = np.array([0x7FC01234, 0xFFFFFFFF, 0x80000000, 0x00000001], np.uint32).view(np.float32)      # payloads a float addition would not keep
        out = prev.copy()
        ctx.trace_radiance(rays, cb, accumulate=True, thread_per_ray=tpr, out=out)
        assert np.array_equal(out[bad].view(np.uint32), prev[bad].view(np.uint32))
        want = prev[good].copy(); want[:, :3] = without[:, :3] + prev[good][:, :3]; want[:, 3] = np.float32(1.0) + prev[good][:, 3]
        _assert_bits(out[good], want, f"{label}: accumulated next to non-finite rays")
    finally:
        ctx.close()


# ---------------------------------------------------------------- 6. tmin below the first hit
def test_tmin_below_the_first_hit_changes_nothing(luts):
    sc, view, pos, bounces = _scene(luts, "cornell")
    cb = scenes.fill_constants(view, pos, sc, 0, bounces)
    rng = np.random.default_rng(4)
    rays = _random_rays(rng, 1000)
    rays["origin"] = rng.uniform((-0.9, 1.3, -3.5), (0.9, 1.9, 0.9), (1000, 3)).astype(np.float32)      # free space above the boxes: every surface is >= 0.08 away
    a, b = rays.copy(), rays.copy()
    a["tmin"] = 0.0; b["tmin"] = np.float32(1e-4)
    ctx = _context(sc)
    try:
        for label, tpr in PATHS:
            _assert_bits(ctx.trace_radiance(a, cb, thread_per_ray=tpr), ctx.trace_radiance(b, cb, thread_per_ray=tpr), f"tmin 0 vs 1e-4, {label}")
    finally:
        ctx.close()


# ---------------------------------------------------------------- 7. isolation
@pytest.mark.parametrize("label,tpr", PATHS)
def test_renders_do_not_notice_the_call(luts, label, tpr):
    w, h = 64, 36
    sc, view, pos, cfg = scenes.config_cornell(luts, w, h, extra_lights=True)
    constants = lambda i: scenes.fill_constants(view, pos, sc, i, cfg["max_bounces"])       # noqa: E731
    rays = _random_rays(np.random.default_rng(2), 5000)

    def state(c):
        return (c.read_accumulation(), c.read_output(), c.read_gbuffer(S.GB_DEPTH), c.exposure(), c.stats(), c.build_info())

    ctx, plain = _context(sc), _context(sc)
    try:
        for c in (ctx, plain):
            c.resize(w, h)
            c.render(constants(0), accum_count=2)
            c.render_gbuffer(constants(0), planes=1 << S.GB_DEPTH)
            c.post_process(S.PostParams(1, 1.0, 0.016, 5.0, -7.0, 23.0, 0.0, 0, 80.0))      # an adapted exposure and a histogram to leave alone
        before = state(ctx)
        got = ctx.trace_radiance(rays, constants(3), thread_per_ray=tpr)
        assert (got[:, :3] > 0).any()
        after = state(ctx)
        for k in range(3):
            assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k
        assert before[3][0] == after[3][0] and np.array_equal(before[3][1], after[3][1])
        for k, struct in ((4, S.Stats), (5, S.BuildInfo)):
            for field, _ in struct._fields_:
                assert getattr(before[k], field) == getattr(after[k], field), field
        for c in (ctx, plain):
            c.render(constants(2), accum_count=2)
        _assert_bits(ctx.read_accumulation().reshape(-1, 4), plain.read_accumulation().reshape(-1, 4), f"the next render, {label}")
        a, b = ctx.stats(), plain.stats()
        for field in ("closestRays", "shadowRays", "paths", "megakernelFallbacks", "queuePoolBytes"):
            assert getattr(a, field) == getattr(b, field), field
    finally:
        ctx.close(); plain.close()


# ---------------------------------------------------------------- 8. device pointers
def test_device_pointers(luts):
    import torch
    rays, want, cb = _oracle_index(luts, "cornell", 0)
    ctx = _context(_scene(luts, "cornell")[0])
    try:
        host = ctx.trace_radiance(rays, cb)
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda:0")
        for flags in (0, S.RADIANCE_THREAD_PER_RAY):
            d_out = torch.full((len(rays), 4), -7.0, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            ctx.trace_radiance_device(d_rays.data_ptr(), d_out.data_ptr(), len(rays), cb, flags)
            ctx.trace_radiance_device(d_rays.data_ptr(), d_out.data_ptr(), len(rays), cb, flags | S.RADIANCE_ACCUMULATE)     # ordered on the context stream
            ctx.synchronize()
            got = d_out.cpu().numpy()
            assert (got[:, 3] == 2.0).all()
            twice = host.copy(); twice[:, :3] = host[:, :3] + host[:, :3]; twice[:, 3] = 2.0
            _assert_bits(got, twice, f"device pointers, flags {flags:#x}")
    finally:
        ctx.close()
    _assert_bits(host, want, "host form vs the oracle")


# ---------------------------------------------------------------- 9. argument checks
def test_argument_checks(luts):
    from hobbyrenderer_amd.native import PathTracerContext, lib
    sc, view, pos, bounces = _scene(luts, "cornell")
    cb = np.ascontiguousarray(scenes.fill_constants(view, pos, sc, 0, bounces))
    rays = _random_rays(np.random.default_rng(1), 100)
    sentinel = np.full((len(rays), 4), -3.0, np.float32)
    out = sentinel.copy()

    def call(c, r=rays, o=out, n=len(rays), constants=cb, flags=0):
        return lib.hrpt_trace_radiance(c._h if c else None, None if r is None else r.ctypes.data, None if o is None else o.ctypes.data, n,
                                       None if constants is None else constants.ctypes.data, flags)

    def refused(c, code, **kw):
        assert call(c, **kw) == code, kw
        assert b"hrpt_trace_radiance" in lib.hrpt_last_error(c._h), kw
        assert np.array_equal(out, sentinel), kw

    assert call(None) == -1                                                      # null context
    ctx = PathTracerContext(0)
    try:
        refused(ctx, -4)                                                         # no scene: HRPT_ERR_NO_SCENE
        ctx.upload_scene(sc)
        ctx.resize(32, 18)
        ctx.render(scenes.fill_constants(scenes.planar_view(32, 18)[0], pos, sc, 0, 2))
        before = (ctx.read_accumulation(), ctx.stats())
        too_deep, too_many = cb.copy(), cb.copy()
        too_deep["m_MaxBounces"] = 65; too_many["m_LightCount"] = len(sc.lights) + 1
        refused(ctx, -1, constants=too_deep)
        refused(ctx, -1, constants=too_many)
        for flags in (1, 0x800, 0x80000000, S.RADIANCE_ACCUMULATE | 0x10):
            refused(ctx, -1, flags=flags)
        refused(ctx, -1, r=None)
        refused(ctx, -1, o=None)
        refused(ctx, -1, constants=None)
        assert call(ctx, n=0) == 0 and call(ctx, r=None, o=None, n=0) == 0      # count == 0 succeeds and does nothing
        assert np.array_equal(out, sentinel)
        after = (ctx.read_accumulation(), ctx.stats())
        assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32))
        for field, _ in S.Stats._fields_:
            assert getattr(before[1], field) == getattr(after[1], field), field
        full = cb.copy(); full["m_MaxBounces"] = 64                              # the largest count that is accepted
        assert call(ctx, n=4, constants=full) == 0 and (out[:4, 3] == 1.0).all() and np.array_equal(out[4:], sentinel[4:])
    finally:
        ctx.close()
