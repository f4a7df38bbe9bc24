"""Traced indirect lighting on the GPU. The three kernels equal the host executors and the NumPy statement on the
synthetic cases; the context call equals, as bytes, hrpt_indirect_rays_host -> hrpt_trace_radiance(HRPT_RADIANCE_SECONDARY) ->
hrpt_indirect_resolve_host through the public calls on a second context; a closed emissive box gives its emission back in the diffuse plane;
nothing of the lighting call leaves a trace in what renders see; errors leave the planes and Output as they were; the chain through
hrpt_temporal_device into hrpt_indirect_compose_device equals the host chain; and deferred direct light plus this stage agrees with the path
tracer's image in the mean.

Every comparison of two implementations is of bits and covers every pixel.

test_deferred_plus_indirect_agrees_with_the_path_tracer, measured on one MI355X (K = 256, Cornell 33 x 25, m_MaxBounces 3): path tracer mean
(0.54105, 0.39146, 0.23350), deferred + indirect (0.54155, 0.39248, 0.23323); the difference (-0.00050, -0.00103, 0.00027) is 0.1 to 0.3
standard errors of the difference, against a bar of five (0.0271, 0.0184, 0.0066). No bias from the bounce-0 cut-off shows at this K."""
import ctypes as C
import math

import numpy as np
import pytest

from hobbyrenderer_amd import native, scenes, structs as S
import indirect_cases as IC
import indirect_reference as R
from test_deferred_gpu import _camera, _context, _moved, _scene, same_bytes
from test_temporal_cpu import u32

pytestmark = pytest.mark.gpu

FOUR = (S.GB_ALBEDO, S.GB_NORMAL, S.GB_GEO_NORMAL, S.GB_DEPTH)
FOUR_MASK = sum(1 << p for p in FOUR)
FIVE_MASK = FOUR_MASK | (1 << S.GB_EMISSIVE)
DIFFUSE, SPECULAR, TPR = S.INDIRECT_DIFFUSE, S.INDIRECT_SPECULAR, S.INDIRECT_THREAD_PER_RAY
SEED = 77


def _constants(sc, name, w, h, bounces=3, index=3):
    view, pos = _camera(name, w, h)
    cb = scenes.fill_constants(view, pos, sc, index, bounces)
    cb["m_Jitter"] = (0.25, -0.125)
    return cb


def _planes(ctx):
    return [ctx.read_gbuffer(p) for p in FOUR]


def _lobes(flags):
    return int(bool(flags & DIFFUSE)) + int(bool(flags & SPECULAR))


# ---------------------------------------------------------------- 1. the kernels == the host executors == the statement, synthetic cases
@pytest.mark.parametrize("size", IC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernels_equal_host_and_statement_on_the_synthetic_cases(size):
    import torch
    c = IC.case(*size)
    W, H = size
    A, _, G, D = c["planes"]
    ctx = native.PathTracerContext(0)                                                # no scene: the three kernels need none
    try:
        dev = [torch.from_numpy(np.array(p)).to("cuda:0") for p in c["planes"]]      # copies: the cases are read-only
        stream = torch.cuda.current_stream()
        for flags in IC.LOBES:
            p = S.IndirectParams(flags, SEED, 0.35)
            n = _lobes(flags)
            # rays
            d_rays = torch.full((n * H * W * 12,), float("nan"), device="cuda:0")
            im = S.IndirectImages(*[t.data_ptr() for t in dev], None, None, None)
            ctx.indirect_rays_device(im, W, H, c["cb"], d_rays.data_ptr(), p, stream.cuda_stream)
            stream.synchronize()
            got = d_rays.cpu().numpy().view(S.Ray).reshape(n, H, W)
            host = native.indirect_rays_host(*c["planes"], c["cb"], p)
            assert got.tobytes() == host.tobytes(), f"rays, flags {flags}: device against host"
            assert host.tobytes() == R.rays(*c["planes"], c["cb"], flags, SEED).tobytes(), f"rays, flags {flags}: host against the statement"
            # resolve, with and without the plane of a lobe that is not flagged
            rad = IC.radiance_for(c, flags)
            d_rad = torch.from_numpy(rad).to("cuda:0")
            d_dif, d_spec = (torch.full((H, W, 4), float("nan"), device="cuda:0") for _ in range(2))
            im = S.IndirectImages(*[t.data_ptr() for t in dev], d_dif.data_ptr(), d_spec.data_ptr(), None)
            ctx.indirect_resolve_device(im, W, H, c["cb"], d_rad.data_ptr(), p, stream.cuda_stream)
            stream.synchronize()
            dif, spec = d_dif.cpu().numpy(), d_spec.cpu().numpy()
            hdif, hspec = native.indirect_resolve_host(*c["planes"], c["cb"], rad, p)
            same_bytes(dif, hdif, f"diffuse, flags {flags}: device against host")
            same_bytes(spec, hspec, f"specular, flags {flags}: device against host")
            rdif, rspec = R.resolve(*c["planes"], c["cb"], rad, flags, SEED)
            same_bytes(hdif, rdif, "diffuse: host against the statement"); same_bytes(hspec, rspec, "specular: host against the statement")
            if n == 1:
                mine, other = (d_dif, d_spec) if flags & DIFFUSE else (d_spec, d_dif)
                mine.fill_(float("nan")); other.fill_(5.0)
                one = S.IndirectImages(*[t.data_ptr() for t in dev], d_dif.data_ptr() if flags & DIFFUSE else None, d_spec.data_ptr() if flags & SPECULAR else None, None)
                ctx.indirect_resolve_device(one, W, H, c["cb"], d_rad.data_ptr(), p, stream.cuda_stream)
                stream.synchronize()
                same_bytes(mine.cpu().numpy(), hdif if flags & DIFFUSE else hspec, "one plane only")
                assert (other == 5.0).all()                                          # the absent plane's memory is not written
                other.copy_(torch.from_numpy(hspec if flags & DIFFUSE else hdif))
            # compose
            d_color = torch.from_numpy(np.array(c["color"])).to("cuda:0")
            im = S.IndirectImages(dev[0].data_ptr(), None, dev[2].data_ptr(), dev[3].data_ptr(), d_dif.data_ptr(), d_spec.data_ptr(), d_color.data_ptr())
            ctx.indirect_compose_device(im, W, H, p, stream.cuda_stream)
            stream.synchronize()
            host = native.indirect_compose_host(c["color"], A, G, D, hdif, hspec, p)
            same_bytes(d_color.cpu().numpy(), host, f"compose, flags {flags}: device against host")
            same_bytes(host, R.compose(c["color"], A, G, D, hdif, hspec, 0.35), "compose: host against the statement")
    finally:
        ctx.close()


# ---------------------------------------------------------------- 2. the context call == the composition of the public calls
@pytest.mark.parametrize("name,size,structure,move", [("cube", (61, 37), None, False), ("cornell", (61, 37), None, False), ("soup", (33, 9), None, False),
                                                      ("cornell", (33, 9), S.ACCEL_TWO_LEVEL, False), ("soup", (33, 9), S.ACCEL_TWO_LEVEL, True)],
                         ids=["cube", "cornell", "soup", "cornell-two-level", "soup-two-level-moved"])
def test_context_call_equals_the_composition_of_the_public_calls(luts, name, size, structure, move):
    sc = _scene(luts, name)
    W, H = size
    cb = _constants(sc, name, W, H)
    ctx, other = _context(sc, structure, W, H), _context(sc, structure)
    try:
        assert structure is None or ctx.build_info().structure == S.ACCEL_TWO_LEVEL
        if move:                                                              # hrpt_update_instances before the frame
            sc = _moved(sc, len(sc.instances) - 1)
            for c in (ctx, other):
                c.update_instances(sc.instances[-1:], len(sc.instances) - 1)
        ctx.render_gbuffer(cb, planes=FOUR_MASK)
        planes = _planes(ctx)
        hit = planes[3][..., 0] != R.MISS
        assert hit.any()
        results = {}
        for flags in (DIFFUSE | SPECULAR, DIFFUSE, SPECULAR, DIFFUSE | SPECULAR | TPR):
            p = S.IndirectParams(flags, SEED)
            ctx.indirect_lighting(cb, p)
            got = (ctx.read_indirect(0), ctx.read_indirect(1))
            rays = native.indirect_rays_host(*planes, cb, p)
            assert rays.tobytes() == R.rays(*planes, cb, flags & 3, SEED).tobytes(), "host executor against the statement"
            rad = other.trace_radiance(rays.reshape(-1), cb, thread_per_ray=bool(flags & TPR), secondary=True).reshape(rays.shape + (4,))
            want = native.indirect_resolve_host(*planes, cb, rad, p)
            for k, what in enumerate(("diffuse", "specular")):
                same_bytes(got[k], want[k], f"{name} flags {flags:#x} {what}")
                assert np.isfinite(got[k]).all() and (got[k][~hit] == 0).all()
            results[flags] = got
        both = results[DIFFUSE | SPECULAR]
        same_bytes(results[DIFFUSE | SPECULAR | TPR][0], both[0], "thread per ray, diffuse"); same_bytes(results[DIFFUSE | SPECULAR | TPR][1], both[1], "thread per ray, specular")
        same_bytes(results[DIFFUSE][0], both[0], "the diffuse lobe alone"); same_bytes(results[SPECULAR][1], both[1], "the specular lobe alone")
        assert (results[DIFFUSE][1] == 0).all() and (results[SPECULAR][0] == 0).all()      # the plane of a lobe that is not flagged is zeroed
        assert (both[0][hit][:, :3] > 0).any() and (both[1][hit][:, :3] > 0).any()
        # compose adds into Output and nowhere else
        ctx.render(cb, accum_count=1)
        before = ctx.read_output()
        p = S.IndirectParams(DIFFUSE | SPECULAR, SEED, 0.6)
        ctx.indirect_compose(p)
        same_bytes(ctx.read_output(), native.indirect_compose_host(before, planes[0], planes[2], planes[3], both[0], both[1], p), f"{name} compose")
    finally:
        ctx.close(); other.close()


# ---------------------------------------------------------------- 3. a closed emissive box gives its emission back
def test_closed_emissive_box_with_black_walls(luts):
    LE = (2.0, 1.5, 0.5)
    b = scenes.SceneBuilder()
    quad = b.add_mesh(*scenes.generate_floor_quad())
    wall = b.add_material(m_BaseColor=(0, 0, 0, 1), m_EmissiveFactor=LE + (1,))
    # x in [-1, 1], y in [0, 2], z in [-4, 1]; the quads overlap at the edges so that no ray leaves through a seam
    for rot, at, scale in (("+y", (0, 0, -1.5), (3, 1, 6)), ("-y", (0, 2, -1.5), (3, 1, 6)), ("+x", (-1, 1, -1.5), (3, 1, 6)), ("-x", (1, 1, -1.5), (3, 1, 6)),
                           ("-z", (0, 1, 1), (3, 1, 3)), ("+z", (0, 1, -4), (3, 1, 3))):
        b.add_instance(quad, wall, scenes._mat(scale, scenes._ROT_TO[rot], at))
    sc = b.finalize(luts)
    W, H = 61, 37
    view, pos = scenes.planar_view(W, H, position=(0.1, 0.9, -3.0), yaw=0.3, pitch=0.1, fov_y=math.radians(70.0))
    # m_MaxBounces = 2: the traced segment is the path's last, so what comes back is the emission of the wall it lands on and nothing else (a
    # third segment would add the dielectric walls' specular reflection of each other, which albedo 0 does not remove)
    cb = scenes.fill_constants(view, pos, sc, 0, 2)
    ctx = _context(sc, None, W, H)
    try:
        ctx.render_gbuffer(cb, planes=FOUR_MASK)
        assert (ctx.read_gbuffer(S.GB_DEPTH)[..., 0] != R.MISS).all()
        for flags in (DIFFUSE | SPECULAR, DIFFUSE | SPECULAR | TPR):
            ctx.indirect_lighting(cb, S.IndirectParams(flags, SEED))
            dif = ctx.read_indirect(0)
            want = np.broadcast_to(np.float32(LE + (1.0,)), dif.shape)
            same_bytes(dif, want, f"the diffuse plane, flags {flags:#x}")
    finally:
        ctx.close()


# ---------------------------------------------------------------- 4. isolation
def test_renders_do_not_notice_the_lighting_call(luts):
    w, h = 64, 36
    sc, view, pos, cfg = scenes.config_cornell(luts, w, h, extra_lights=True)
    constants = lambda i: scenes.fill_constants(view, pos, sc, i, cfg["max_bounces"])       # noqa: E731
    full = view.copy()
    full["m_CameraDirectionOrPosition"] = (pos[0], pos[1], pos[2], 1.0)

    def state(c):
        return ([c.read_accumulation(), c.read_output(), c.read_motion_vectors(), c.read_temporal_history()] + [c.read_gbuffer(p) for p in FOUR], c.exposure(), c.stats(),
                c.build_info())

    ctx, plain = _context(sc, None, w, h), _context(sc, None, w, h)
    try:
        for c in (ctx, plain):
            c.render(constants(0), accum_count=2)
            c.render_motion_vectors(constants(0), full, planes=FOUR_MASK)
            c.temporal_accumulate(full, full)
            c.post_process(S.PostParams(1, 1.0, 0.016, 5.0, -7.0, 23.0, 0.0, 0, 80.0))      # an adapted exposure and a histogram to leave alone
        before = state(ctx)
        ctx.indirect_lighting(constants(0))
        ctx.indirect_lighting(constants(0), S.IndirectParams(DIFFUSE | TPR, 5))
        assert (ctx.read_indirect(0)[..., :3] > 0).any()
        after = state(ctx)
        for k, (a, b) in enumerate(zip(before[0], after[0])):
            assert np.array_equal(u32(a), u32(b)), k
        assert before[1][0] == after[1][0] and np.array_equal(before[1][1], after[1][1])
        for k, struct in ((2, S.Stats), (3, S.BuildInfo)):
            for field, _ in struct._fields_:
                assert getattr(before[k], field) == getattr(after[k], field), field
        for c in (ctx, plain):
            c.render(constants(2), accum_count=2)
        same_bytes(ctx.read_accumulation(), plain.read_accumulation(), "the next render")
        same_bytes(ctx.read_output(), plain.read_output(), "the next render's Output")
        a, b = ctx.stats(), plain.stats()
        for field in ("closestRays", "shadowRays", "paths", "megakernelFallbacks", "queuePoolBytes"):
            assert getattr(a, field) == getattr(b, field), field
    finally:
        ctx.close(); plain.close()


# ---------------------------------------------------------------- 5. errors leave the planes and Output as they were
def test_errors_leave_the_planes_and_output_as_they_were(luts):
    lib = native.lib
    sc = _scene(luts, "cornell")
    W, H = 33, 9
    cb = np.ascontiguousarray(_constants(sc, "cornell", W, H))
    ok = S.IndirectParams(DIFFUSE | SPECULAR, SEED)
    ctx = native.PathTracerContext(0)
    try:
        err = lambda: lib.hrpt_last_error(ctx._h).decode()                                  # noqa: E731
        call = lambda constants=cb, p=ok: lib.hrpt_indirect_lighting(ctx._h, None if constants is None else constants.ctypes.data, None if p is None else C.byref(p))   # noqa: E731
        compose = lambda p=ok: lib.hrpt_indirect_compose(ctx._h, None if p is None else C.byref(p))   # noqa: E731
        assert call() == -4 and "no scene" in err()                                         # HRPT_ERR_NO_SCENE
        ctx.upload_scene(sc)
        assert call() == -1 and "hrpt_resize not called" in err()
        assert compose() == -1 and "hrpt_resize not called" in err()
        ctx.resize(W, H)
        assert call() == -1 and "HRPT_GB_ALBEDO" in err()
        ctx.render_gbuffer(cb, planes=FOUR_MASK & ~(1 << S.GB_GEO_NORMAL))
        assert call() == -1 and "HRPT_GB_GEO_NORMAL" in err()
        ctx.render_gbuffer(cb, planes=FOUR_MASK)
        assert compose() == -1 and "hrpt_indirect_lighting writes them" in err()            # compose before lighting
        assert lib.hrpt_read_indirect(ctx._h, 0, None, 0) == -1 and ctx.indirect_device(0) is None
        ctx.render(cb, accum_count=1)
        assert call() == 0
        before = (ctx.read_indirect(0), ctx.read_indirect(1), ctx.read_output())
        too_many, too_deep = cb.copy(), cb.copy()
        too_many["m_LightCount"] = len(sc.lights) + 1; too_deep["m_MaxBounces"] = 65
        assert call(constants=too_many) == -1 and "m_LightCount" in err()
        assert call(constants=too_deep) == -1 and "m_MaxBounces" in err()
        assert call(constants=None) == -1 and call(p=None) == -1 and compose(p=None) == -1
        bad = [S.IndirectParams(0, 0), S.IndirectParams(TPR, 0), S.IndirectParams(3 | 4, 0), S.IndirectParams(3 | 0x100, 0), S.IndirectParams(3, 0, math.nan),
               S.IndirectParams(3, 0, math.inf)]
        p = S.IndirectParams(3, 0); p.reserved = 3
        for p in bad + [p]:
            assert call(p=p) == -1 and "no lobe flag" in err()
            assert compose(p=p) == -1 and "no lobe flag" in err()
        four = [ctx.gbuffer_device(q) for q in FOUR]
        im = S.IndirectImages(*four, None, None, None)
        dev = lambda images: lib.hrpt_indirect_lighting_device(ctx._h, None if images is None else C.byref(images), W, H, cb.ctypes.data, C.byref(ok), None)   # noqa: E731
        assert dev(im) == -1 and "null image" in err()
        assert dev(S.IndirectImages(*four, ctx.indirect_device(0), four[3], None)) == -1 and "must differ" in err()
        assert dev(S.IndirectImages(*four, ctx.indirect_device(0), ctx.indirect_device(0), None)) == -1 and "must differ" in err()
        assert dev(None) == -1
        cim = S.IndirectImages(four[0], None, four[2], four[3], ctx.indirect_device(0), ctx.indirect_device(1), None)
        assert lib.hrpt_indirect_compose_device(ctx._h, C.byref(cim), W, H, C.byref(ok), None) == -1 and "null image" in err()
        cim.colorInOut = ctx.indirect_device(1)
        assert lib.hrpt_indirect_compose_device(ctx._h, C.byref(cim), W, H, C.byref(ok), None) == -1 and "must differ" in err()
        assert lib.hrpt_read_indirect(ctx._h, 2, before[0].ctypes.data, before[0].nbytes) == -1
        after = (ctx.read_indirect(0), ctx.read_indirect(1), ctx.read_output())
        for a, b, what in zip(before, after, ("diffuse", "specular", "Output")):
            same_bytes(b, a, f"{what} after refused calls")
        assert compose() == 0 and not np.array_equal(ctx.read_output(), before[2])
        ctx.resize(W + 1, H)                                                                # the indirect planes and the ray buffers are dropped
        assert ctx.indirect_device(0) is None and compose() == -1 and "hrpt_indirect_lighting writes them" in err()
        assert call() == 0 and ctx.read_indirect(1).shape == (H, W + 1, 4)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 6. lighting -> temporal on the diffuse plane -> compose
def test_the_chain_through_temporal_into_compose_equals_the_host_chain(luts):
    import torch
    sc = _scene(luts, "cornell")
    W, H = 33, 25
    view, pos = _camera("cornell", W, H)
    full = view.copy()
    full["m_CameraDirectionOrPosition"] = (pos[0], pos[1], pos[2], 1.0)
    cb = scenes.fill_constants(view, pos, sc, 5, 3)
    p = S.IndirectParams(DIFFUSE | SPECULAR, SEED, 0.8)
    tp = S.TemporalParams(0.9, S.TEMPORAL_LINEAR)
    ctx = _context(sc, None, W, H)
    try:
        ctx.render_motion_vectors(cb, full, planes=FIVE_MASK)
        ctx.deferred_lighting(cb)
        ctx.indirect_lighting(cb, p)
        stream = torch.cuda.current_stream()
        ctx.synchronize()
        lit, planes, motion = ctx.read_output(), _planes(ctx), ctx.read_motion_vectors()
        dif, spec = ctx.read_indirect(0), ctx.read_indirect(1)
        history, smooth = (torch.full((H, W, 4), float("nan"), device="cuda:0") for _ in range(2))
        tim = S.TemporalImages(ctx.indirect_device(0), ctx.motion_vectors_device(), ctx.gbuffer_device(S.GB_DEPTH), ctx.gbuffer_device(S.GB_NORMAL), None,
                               history.data_ptr(), smooth.data_ptr())
        ctx.temporal_device(tim, W, H, full, full, tp, stream.cuda_stream)
        color = torch.from_numpy(lit).to("cuda:0")
        cim = S.IndirectImages(ctx.gbuffer_device(S.GB_ALBEDO), None, ctx.gbuffer_device(S.GB_GEO_NORMAL), ctx.gbuffer_device(S.GB_DEPTH), smooth.data_ptr(),
                               ctx.indirect_device(1), color.data_ptr())
        ctx.indirect_compose_device(cim, W, H, p, stream.cuda_stream)
        stream.synchronize()
        want_smooth, _ = native.temporal_host(dif, motion, planes[3], planes[1], None, full, full, tp)
        same_bytes(smooth.cpu().numpy(), want_smooth, "the diffuse plane through the temporal stage")
        want = native.indirect_compose_host(lit, planes[0], planes[2], planes[3], want_smooth, spec, p)
        got = color.cpu().numpy()
        same_bytes(got, want, "composed")
        assert np.isfinite(got).all() and not np.array_equal(got, lit)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 7. against the path tracer
def test_deferred_plus_indirect_agrees_with_the_path_tracer(luts):
    """Cornell with the point and spot light at radius 0 and the right wall metallic, 33 x 25, m_MaxBounces = 3, K = 256 indices. (a) hrpt_render,
    one sample per index on a cleared Accumulation; (b) per index, with the jitter hrpt_render derives from the index: render_gbuffer ->
    deferred_lighting(SHADOWS) -> indirect_lighting(frameSeed = index) -> indirect_compose. The whole-image mean per channel of the two K-averages
    differs by at most five standard errors of the difference, the standard errors estimated from the K per-index image means of each side:
    a false-failure chance below 1e-6 per channel for unbiased estimators, and with fixed seeds the test is deterministic."""
    W, H, K, BOUNCES = 33, 25, 256, 3
    sc = scenes.cornell_scene(luts, extra_lights=True)
    sc.lights["m_Radius"] = 0.0
    green = int(np.argmin(np.abs(sc.materials["m_BaseColor"][:, :3] - np.float32([0.12, 0.45, 0.15])).sum(-1)))
    sc.materials["m_RoughnessMetallic"][green] = (0.3, 1.0)                             # the right wall: a rough mirror
    view, pos = _camera("cornell", W, H)
    constants = lambda i: scenes.fill_constants(view, pos, sc, i, BOUNCES)               # noqa: E731  (m_Jitter = the Halton point of index i, as hrpt_render forms it)
    ctx = _context(sc, None, W, H)
    try:
        a, b = np.zeros((K, 3)), np.zeros((K, 3))
        for i in range(K):
            ctx.clear_accumulation()
            ctx.render(constants(i), accum_count=1)
            acc = ctx.read_accumulation()
            assert (acc[..., 3] == 1).all()
            a[i] = acc[..., :3].astype(np.float64).mean((0, 1))
        spec_sum, deferred_first = np.zeros((H, W, 3)), None
        for i in range(K):
            cb = constants(i)
            ctx.render_gbuffer(cb, planes=FIVE_MASK)
            ctx.deferred_lighting(cb, S.DeferredParams(S.DEFERRED_SHADOWS))
            if i == 0:
                deferred_first, geo = ctx.read_output(), ctx.read_gbuffer(S.GB_GEO_NORMAL)
            p = S.IndirectParams(DIFFUSE | SPECULAR, i, 1.0)
            ctx.indirect_lighting(cb, p)
            ctx.indirect_compose(p)
            b[i] = ctx.read_output()[..., :3].astype(np.float64).mean((0, 1))
            spec_sum += ctx.read_indirect(1)[..., :3]
    finally:
        ctx.close()
    mean_a, mean_b = a.mean(0), b.mean(0)
    se_a, se_b = a.std(0, ddof=1) / math.sqrt(K), b.std(0, ddof=1) / math.sqrt(K)
    bar = 5.0 * np.sqrt(se_a ** 2 + se_b ** 2)
    print(f"path tracer mean {mean_a} (SE {se_a}); deferred + indirect mean {mean_b} (SE {se_b}); difference {mean_a - mean_b}, bar {bar}")
    # the specular plane lights the metallic wall where deferred alone gives only highlights
    metal = geo[..., 3] == 1
    assert metal.sum() > 20
    lit = (spec_sum[metal] > 0).any(-1)
    dark = (deferred_first[metal][:, :3] < 1e-3).all(-1)
    print(f"metallic wall: {int(metal.sum())} pixels, {int(dark.sum())} dark under deferred alone at index 0, {int(lit.sum())} lit by the specular plane")
    assert lit.all() and (spec_sum[metal].mean() > 10 * K * 1e-3)
    assert (np.abs(mean_a - mean_b) <= bar).all(), (mean_a, mean_b, bar)
