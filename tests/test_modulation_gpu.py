"""The demodulate and compose stages on the device (hrpt_demodulate_device / hrpt_compose_device, hrpt_demodulate / hrpt_compose; DESIGN.md
section 20): the gfx950 kernels against the host executors and the NumPy restatement (tests/modulation_reference.py), bit for bit on
uint32 views with no pixel left out; the context path over a real scene in the documented frame order, every stage against the chained
host calls over the read-backs; the errors of the context calls; and what the stages must leave alone."""
import ctypes as C

import numpy as np
import pytest

from hobbyrenderer_amd import native, scenes, structs as S
import denoise_cases as DC
import modulation_cases as MC
import modulation_reference as R
import temporal_cases as TC
from test_modulation_cpu import KEYS, assert_same, case, u32
from test_temporal_gpu import H, SPP, W, _view

pytestmark = pytest.mark.gpu

NEEDED = (S.GB_ALBEDO, S.GB_NORMAL, S.GB_GEO_NORMAL, S.GB_EMISSIVE, S.GB_DEPTH)
PLANES = sum(1 << k for k in NEEDED)
PLANE_NAMES = {S.GB_ALBEDO: "HRPT_GB_ALBEDO", S.GB_NORMAL: "HRPT_GB_NORMAL", S.GB_GEO_NORMAL: "HRPT_GB_GEO_NORMAL", S.GB_EMISSIVE: "HRPT_GB_EMISSIVE",
               S.GB_DEPTH: "HRPT_GB_DEPTH"}


@pytest.fixture(scope="module")
def ctx0():
    ctx = native.PathTracerContext(0)
    yield ctx
    ctx.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")


def device_demodulate(ctx, c, floor, emissive, in_place):
    """hrpt_demodulate_device over torch tensors on the current torch stream; (colorOut, modulation) as host arrays."""
    import torch
    h, w = c["color"].shape[:2]
    dev = [_dev(c[k]) for k in KEYS]
    em = _dev(c["emissive"]) if emissive else None
    out = dev[0] if in_place else torch.full((h, w, 4), float("nan"), device="cuda:0")
    mod = torch.full((h, w, 4), float("nan"), device="cuda:0")
    im = S.DemodulateImages(*[t.data_ptr() for t in dev], None if em is None else em.data_ptr(), out.data_ptr(), mod.data_ptr())
    stream = torch.cuda.current_stream()
    ctx.demodulate_device(im, w, h, c["view"], S.ModulationParams(floor), stream.cuda_stream)
    stream.synchronize()
    return out.cpu().numpy(), mod.cpu().numpy()


def device_compose(ctx, color, mod, emissive, in_place):
    import torch
    h, w = color.shape[:2]
    col, m = _dev(color), _dev(mod)
    em = None if emissive is None else _dev(emissive)
    out = col if in_place else torch.full((h, w, 4), float("nan"), device="cuda:0")
    im = S.ComposeImages(col.data_ptr(), m.data_ptr(), None if em is None else em.data_ptr(), out.data_ptr())
    stream = torch.cuda.current_stream()
    ctx.compose_device(im, w, h, stream.cuda_stream)
    stream.synchronize()
    return out.cpu().numpy()


def check_case(ctx, c, floors, what):
    other = DC.TC.radiance(c["color"].shape[1], c["color"].shape[0], 77)
    for floor in floors:
        for k, emissive in enumerate((True, False)):
            for in_place in (False, True):
                label = f"{what} floor={floor} emissive={emissive} in_place={in_place}"
                e = c["emissive"] if emissive else None
                ref_col, ref_mod = R.demodulate(*[c[k2] for k2 in KEYS], c["view"], floor=floor, emissive=e)
                host_col, host_mod = native.demodulate_host(*[c[k2] for k2 in KEYS], c["view"], S.ModulationParams(floor), emissive=e)
                dev_col, dev_mod = device_demodulate(ctx, c, floor, emissive, in_place)
                assert_same(dev_mod, host_mod, label + ": device vs host, modulation")
                assert_same(dev_mod, ref_mod, label + ": device vs reference, modulation")
                assert_same(dev_col, host_col, label + ": device vs host, colour")
                assert_same(dev_col, ref_col, label + ": device vs reference, colour")
                for colour, name in ((dev_col, "demodulated"), (other, "other")):
                    got = device_compose(ctx, colour, dev_mod, e, in_place)
                    assert_same(got, native.compose_host(colour, host_mod, e), label + f": device vs host, composed {name} colour")
                    assert_same(got, R.compose(colour, ref_mod, e), label + f": device vs reference, composed {name} colour")


# ---------------------------------------------------------------- 1. device == host == NumPy on the synthetic cases
@pytest.mark.parametrize("size", MC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_host_and_reference(ctx0, size):
    w, h = size
    check_case(ctx0, case(w, h), MC.FLOORS, f"{w}x{h}")


def test_many_tiles_and_partial_tiles(ctx0):
    """200 x 120: 7 x 15 tiles of 32 x 8, partial on the right edge."""
    check_case(ctx0, MC.case(200, 120), (0.04,), "200x120")


# ---------------------------------------------------------------- 2. the context path over a scene
def _scene_context(luts):
    """The cube scene with its material tinted: the default one is a white non-metal, whose factor is (1, 1, 1) at every hit."""
    sc = scenes.cube_scene(luts)
    sc.materials["m_BaseColor"] = (0.8, 0.3, 0.1, 1.0)
    sc.materials["m_RoughnessMetallic"] = (0.4, 0.5)
    sc.materials["m_EmissiveFactor"] = (0.05, 0.1, 0.2, 1.0)
    ctx = native.PathTracerContext(0)
    ctx.upload_scene(sc)
    ctx.resize(W, H)
    records = sc.instances.copy()
    records["m_PrevWorld"] = records["m_World"]
    ctx.update_instances(records, 0)
    return sc, ctx


def _render(ctx, sc, view, pos, full, frame, planes=PLANES):
    cb = scenes.fill_constants(view, pos, sc, frame * SPP, 2)
    ctx.clear_accumulation()
    ctx.render(cb, accum_count=SPP)
    cbm = cb.copy()
    cbm["m_Jitter"] = (0.0, 0.0)
    ctx.render_motion_vectors(cbm, full, planes=planes)


def _planes(ctx):
    return {k: ctx.read_gbuffer(k) for k in NEEDED}


def test_context_path_every_stage_equals_the_chained_host_calls(luts):
    """Three frames of render -> motion vectors -> demodulate -> temporal -> denoise (2 iterations) -> compose: after each stage Output, the
    modulation image and the history equal the host calls chained over the read-backs; the history holds the DEMODULATED signal."""
    sc, ctx = _scene_context(luts)
    view, pos, full = _view()
    tparams = TC.params(0.9, False)
    iterations = 2
    try:
        history = None
        for frame in range(3):
            _render(ctx, sc, view, pos, full, frame)
            g, motion, color = _planes(ctx), ctx.read_motion_vectors(), ctx.read_output()
            hit = g[S.GB_DEPTH][..., 0] != np.float32(1e10)
            assert 0 < hit.sum() < hit.size

            ctx.demodulate(full, S.ModulationParams(0.04))
            want_col, want_mod = native.demodulate_host(color, g[S.GB_ALBEDO], g[S.GB_NORMAL], g[S.GB_GEO_NORMAL], g[S.GB_DEPTH], full,
                                                        S.ModulationParams(0.04), emissive=g[S.GB_EMISSIVE])
            mod = ctx.read_modulation()
            assert_same(mod, want_mod, f"frame {frame}: modulation")
            assert_same(ctx.read_output(), want_col, f"frame {frame}: demodulated Output")
            assert_same(mod, R.modulation(g[S.GB_ALBEDO], g[S.GB_NORMAL], g[S.GB_GEO_NORMAL], g[S.GB_DEPTH], full), f"frame {frame}: modulation vs reference")
            assert (mod[hit][:, 3] == 1).all() and (mod[~hit] == np.float32([1, 1, 1, 0])).all() and (mod[hit][:, :3] != 1).any()
            assert ctx.modulation_device()

            ctx.temporal_accumulate(full, full, tparams)
            t_out, t_hist = native.temporal_host(want_col, motion, g[S.GB_DEPTH], g[S.GB_NORMAL], history, full, full, tparams)
            assert_same(ctx.read_output(), t_out, f"frame {frame}: temporal Output")
            assert_same(ctx.read_temporal_history(), t_hist, f"frame {frame}: temporal history")

            ctx.denoise(full, DC.params(3.0, frame, iterations))
            x = t_hist
            for i in range(iterations):
                last = i + 1 == iterations
                r = native.denoise_host(x, g[S.GB_DEPTH], g[S.GB_NORMAL], g[S.GB_GEO_NORMAL], full, DC.params(3.0 * (1 << i), frame * iterations + i),
                                        color=t_out if last else None)
                x, d_out = r if last else (r, None)
            assert_same(ctx.read_temporal_history(), x, f"frame {frame}: denoised history")
            assert_same(ctx.read_output(), d_out, f"frame {frame}: denoised Output")

            ctx.compose()
            assert_same(ctx.read_output(), native.compose_host(d_out, want_mod, g[S.GB_EMISSIVE]), f"frame {frame}: composed Output")
            assert_same(ctx.read_modulation(), want_mod, f"frame {frame}: modulation after compose")
            assert_same(ctx.read_temporal_history(), x, f"frame {frame}: history after compose")
            history = x
    finally:
        ctx.close()


def test_errors_isolation_and_caller_stream(luts):
    import torch
    view, pos, full = _view()
    # a plane that was never requested is named
    for missing in NEEDED:
        sc, ctx = _scene_context(luts)
        try:
            _render(ctx, sc, view, pos, full, 0, planes=PLANES & ~(1 << missing))
            with pytest.raises(native.HrptError) as e:
                ctx.demodulate(full)
            assert e.value.code == -1 and PLANE_NAMES[missing] + " " in str(e.value) and "never requested" in str(e.value)
            with pytest.raises(native.HrptError) as e:               # compose before demodulate
                ctx.compose()
            assert e.value.code == -1 and "hrpt_demodulate" in str(e.value)
            assert ctx.modulation_device() is None
            with pytest.raises(native.HrptError):
                ctx.read_modulation()
        finally:
            ctx.close()

    sc, ctx = _scene_context(luts)
    try:
        _render(ctx, sc, view, pos, full, 0)
        color = ctx.read_output()
        wrong = full.copy(); wrong["m_ViewportSize"] = (W, H + 1)
        with pytest.raises(native.HrptError) as e:
            ctx.demodulate(wrong)
        assert "m_ViewportSize" in str(e.value)
        for bad in (S.ModulationParams(0.0), S.ModulationParams(float("nan")), S.ModulationParams(float("inf")), S.ModulationParams(-1.0),
                    S.ModulationParams(0.04, 1)):
            with pytest.raises(native.HrptError):
                ctx.demodulate(full, bad)
        assert native.lib.hrpt_demodulate(ctx._h, None, C.byref(S.ModulationParams())) == -1
        assert native.lib.hrpt_demodulate(ctx._h, full.ctypes.data, None) == -1
        assert_same(ctx.read_output(), color, "refused calls leave Output alone")
        assert ctx.modulation_device() is None                    # ... and allocate nothing

        # the calls leave Accumulation, the planes, the motion plane, the temporal history, exposure and the statistics as they were
        ctx.temporal_accumulate(full, full, TC.params(0.9, False))
        ctx.post_process(S.PostParams(1, 1.0, 0.016, 5.0, -7.0, 23.0, 0.0, 0, 80.0))

        def state():
            images = [ctx.read_accumulation(), ctx.read_motion_vectors(), ctx.read_temporal_history()] + [ctx.read_gbuffer(k) for k in NEEDED]
            return images, ctx.exposure(), ctx.stats()
        g = _planes(ctx)
        before_out = ctx.read_output()
        images_before, exposure_before, stats_before = state()
        ctx.demodulate(full, S.ModulationParams(0.5))
        want_col, want_mod = native.demodulate_host(before_out, g[S.GB_ALBEDO], g[S.GB_NORMAL], g[S.GB_GEO_NORMAL], g[S.GB_DEPTH], full,
                                                    S.ModulationParams(0.5), emissive=g[S.GB_EMISSIVE])
        assert_same(ctx.read_output(), want_col, "floor 0.5: demodulated Output")
        ctx.compose()
        images_after, exposure_after, stats_after = state()
        for a, b in zip(images_before, images_after):
            assert np.array_equal(u32(a), u32(b))
        assert exposure_before[0] == exposure_after[0] and np.array_equal(exposure_before[1], exposure_after[1])
        for field, _ in S.Stats._fields_:
            assert getattr(stats_before, field) == getattr(stats_after, field), field
        assert_same(ctx.read_output(), native.compose_host(want_col, want_mod, g[S.GB_EMISSIVE]), "floor 0.5: composed Output")
        # stateless: a second demodulate without a render divides again
        ctx.demodulate(full, S.ModulationParams(0.5))
        once = ctx.read_output()
        ctx.demodulate(full, S.ModulationParams(0.5))
        assert_same(ctx.read_output(), native.demodulate_host(once, g[S.GB_ALBEDO], g[S.GB_NORMAL], g[S.GB_GEO_NORMAL], g[S.GB_DEPTH], full,
                                                               S.ModulationParams(0.5), emissive=g[S.GB_EMISSIVE])[0], "two demodulates divide twice")

        # on a caller stream
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        _render(ctx, sc, view, pos, full, 1)
        g, color = _planes(ctx), ctx.read_output()
        ctx.demodulate(full)
        stream.synchronize()
        got_col, got_mod = ctx.read_output(), ctx.read_modulation()
        ctx.compose()
        stream.synchronize()
        got_back = ctx.read_output()
        ctx.set_stream(None)
        want_col, want_mod = native.demodulate_host(color, g[S.GB_ALBEDO], g[S.GB_NORMAL], g[S.GB_GEO_NORMAL], g[S.GB_DEPTH], full, emissive=g[S.GB_EMISSIVE])
        assert_same(got_col, want_col, "caller stream: demodulated Output")
        assert_same(got_mod, want_mod, "caller stream: modulation")
        assert_same(got_back, native.compose_host(want_col, want_mod, g[S.GB_EMISSIVE]), "caller stream: composed Output")

        # hrpt_resize drops the modulation image: compose is an error until demodulate has run again
        ctx.resize(W, H)
        with pytest.raises(native.HrptError) as e:
            ctx.compose()
        assert e.value.code == -1 and "hrpt_demodulate" in str(e.value)
        assert ctx.modulation_device() is None
        _render(ctx, sc, view, pos, full, 2)
        g, color = _planes(ctx), ctx.read_output()
        ctx.demodulate(full)
        ctx.compose()
        want_col, want_mod = native.demodulate_host(color, g[S.GB_ALBEDO], g[S.GB_NORMAL], g[S.GB_GEO_NORMAL], g[S.GB_DEPTH], full, emissive=g[S.GB_EMISSIVE])
        assert_same(ctx.read_output(), native.compose_host(want_col, want_mod, g[S.GB_EMISSIVE]), "after hrpt_resize: composed Output")
    finally:
        ctx.close()
