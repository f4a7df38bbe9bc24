"""The upscale stage on the device (hrpt_upscale_device / hrpt_upscale / hrpt_post_process_device): the gfx950 kernel
against the host executor and the NumPy restatement (tests/upscale_reference.py), bit for bit on uint32 views with no pixel left out; the
context path over a real scene in the documented frame order; what the stage must leave alone; and the post chain over a caller's image."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from hobbyrenderer_amd import native, scenes, structs as S
import upscale_cases as UC
from test_temporal_cpu import assert_same, u32
from test_upscale_cpu import MOTIONS, SIZES, host

pytestmark = pytest.mark.gpu


def make_context(staged):
    """A context whose upscale kernel gathers its current-frame taps from global memory (the default) or serves them from the LDS-staged
    window: HRPT_UPSCALE_STAGED is read at hrpt_create."""
    before = os.environ.get("HRPT_UPSCALE_STAGED")
    os.environ["HRPT_UPSCALE_STAGED"] = "1" if staged else "0"
    try:
        return native.PathTracerContext(0)
    finally:
        if before is None:
            del os.environ["HRPT_UPSCALE_STAGED"]
        else:
            os.environ["HRPT_UPSCALE_STAGED"] = before


@pytest.fixture(scope="module", params=[False, True], ids=["gather", "staged"])
def ctx0(request):
    ctx = make_context(request.param)
    yield ctx
    ctx.close()


def device_call(ctx, c, history, clamp):
    """hrpt_upscale_device over torch tensors on the current torch stream; the outputs start as NaN, so that an unwritten pixel shows.
    Returns (colorOut, historyOut) as host arrays."""
    import torch
    (w, h), (W, H) = c["size"], c["display"]
    dev = [torch.from_numpy(np.array(c[k], np.float32)).to("cuda:0") for k in ("color", "depth", "motion")]      # a copy: the cases are read-only
    hist = None if history is None else torch.from_numpy(np.array(history, np.float32)).to("cuda:0")
    hout = torch.full((H, W, 4), float("nan"), device="cuda:0")
    cout = torch.full((H, W, 4), float("nan"), device="cuda:0")
    im = S.UpscaleImages(*[t.data_ptr() for t in dev], None if hist is None else hist.data_ptr(), hout.data_ptr(), cout.data_ptr())
    stream = torch.cuda.current_stream()
    ctx.upscale_device(im, w, h, W, H, c["view"], c["prev"], UC.params(c, clamp), stream.cuda_stream)
    stream.synchronize()
    return cout.cpu().numpy(), hout.cpu().numpy()


# ---------------------------------------------------------------- 1. device == host == NumPy on the synthetic cases
@SIZES
@MOTIONS
def test_device_equals_host_and_reference(ctx0, name, pair):
    """100x60 -> 200x120 is 7 x 15 tiles of 32 x 8, partial on the right edge; 37x23 -> 55x34 has windows that start between texels."""
    for jitter in (False, True):
        c = UC.case(name, pair, jitter)
        for with_history in (False, True):
            for clamp in (True, False):
                what = f"{name} {UC.pair_id(pair)} jitter={jitter} history={with_history} clamp={clamp}"
                hist = c["history"] if with_history else None
                dev = device_call(ctx0, c, hist, clamp)
                lib = host(c, hist, clamp)
                ref = UC.reference(name, pair, jitter, with_history, clamp)
                for k, plane in enumerate(("colorOut", "historyOut")):
                    assert_same(dev[k], lib[k], f"{what}: device vs host, {plane}")
                    assert_same(dev[k], ref[k], f"{what}: device vs reference, {plane}")


@pytest.mark.parametrize("pair", [((1, 1), (4, 4)), ((40, 9), (160, 36)), ((33, 9), (33, 9))], ids=UC.pair_id)
def test_ratio_limits_on_the_device(ctx0, pair):
    """4x: the smallest window of render texels under a tile; 1x with the jitter at both of its limits: the widest (35 x 11 texels of the
    staged kernel's 36 x 12)."""
    for jitter in ((0.5, 0.5), (-0.5, -0.5), UC.JITTER):
        c = dict(UC.case("random", pair, True), jitter=jitter)
        dev = device_call(ctx0, c, c["history"], True)
        lib = host(c, c["history"], True)
        assert_same(dev[0], lib[0], f"{UC.pair_id(pair)} jitter={jitter}: colorOut")
        assert_same(dev[1], lib[1], f"{UC.pair_id(pair)} jitter={jitter}: historyOut")


# ---------------------------------------------------------------- 2. the context path over a scene
W, H, DW, DH = 32, 18, 64, 36
PLANES = 1 << S.GB_DEPTH


def _view(yaw=0.0):
    view, pos = scenes.planar_view(W, H, position=(0.0, 1.0, -3.4), yaw=yaw, fov_y=math.radians(40.0), aspect=16.0 / 9.0)
    full = view.copy()
    full["m_CameraDirectionOrPosition"] = (pos[0], pos[1], pos[2], 1.0)
    return view, pos, full


def _frame(ctx, sc, view, pos, prev_full, index):
    """render + planes of one frame in the documented order: accumCount 1 at accumulation index `index`, the planes with the same jitter.
    Returns the read-backs the host executor needs and the jitter to pass on."""
    cb = scenes.fill_constants(view, pos, sc, index, 2)       # m_Jitter = (halton(index + 1, 2) - 0.5, halton(index + 1, 3) - 0.5)
    jitter = (float(native.lib.hrpt_halton(index + 1, 2)) - 0.5, float(native.lib.hrpt_halton(index + 1, 3)) - 0.5)
    assert tuple(np.float32(j) for j in jitter) == tuple(cb["m_Jitter"])
    ctx.clear_accumulation()
    ctx.render(cb, accum_count=1)
    ctx.render_motion_vectors(cb, prev_full, planes=PLANES)
    return dict(color=ctx.read_output(), depth=ctx.read_gbuffer(S.GB_DEPTH), motion=ctx.read_motion_vectors()), jitter


def _state(ctx):
    return [ctx.read_output(), ctx.read_accumulation(), ctx.read_motion_vectors(), ctx.read_gbuffer(S.GB_DEPTH), ctx.read_temporal_history()], ctx.stats()


@pytest.mark.parametrize("staged", [False, True], ids=["gather", "staged"])
def test_context_path_four_frames_reset_and_display_size(luts, staged):
    sc = scenes.cornell_scene(luts)
    ctx = make_context(staged)
    try:
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        view, pos, full = _view()
        prev_full = full
        history = None
        for frame in range(4):
            if frame == 2:                                    # the camera yaws; last frame's view becomes prevView
                view, pos, full = _view(0.04)
            inp, jitter = _frame(ctx, sc, view, pos, prev_full, 5 + frame)
            p = S.UpscaleParams(jitter=jitter)
            ctx.upscale(DW, DH, full, prev_full, p)
            want = native.upscale_host(inp["color"], inp["depth"], inp["motion"], history, (DW, DH), full, prev_full, p)
            assert_same(ctx.read_upscaled(), want[0], f"frame {frame}: upscaled")
            assert_same(ctx.read_upscale_history(), want[1], f"frame {frame}: history")
            assert np.array_equal(u32(ctx.read_output()), u32(inp["color"]))
            if frame == 2:
                assert np.hypot(inp["motion"][..., 0], inp["motion"][..., 1]).max() > 0.5
            if frame:                                         # the history was used: more sample weight than this frame alone gives
                alone = native.upscale_host(inp["color"], inp["depth"], inp["motion"], None, (DW, DH), full, prev_full, p)
                assert (want[1][..., 3] > alone[1][..., 3]).mean() > 0.5
            history, prev_full = want[1], full
        assert ctx.upscaled_device()

        # HRPT_UPSCALE_RESET runs without the history, on the same inputs
        p = S.UpscaleParams(jitter=jitter, flags=S.UPSCALE_RESET)
        ctx.upscale(DW, DH, full, full, p)
        want = native.upscale_host(inp["color"], inp["depth"], inp["motion"], None, (DW, DH), full, full, p)
        assert_same(ctx.read_upscale_history(), want[1], "HRPT_UPSCALE_RESET")
        # ... and the next call uses what the reset call wrote
        p = S.UpscaleParams(jitter=jitter)
        ctx.upscale(DW, DH, full, full, p)
        want2 = native.upscale_host(inp["color"], inp["depth"], inp["motion"], want[1], (DW, DH), full, full, p)
        assert_same(ctx.read_upscale_history(), want2[1], "after the reset call")
        # a changed display size drops the history
        ctx.upscale(48, 27, full, full, p)
        want3 = native.upscale_host(inp["color"], inp["depth"], inp["motion"], None, (48, 27), full, full, p)
        assert ctx.read_upscaled().shape == (27, 48, 4)
        assert_same(ctx.read_upscaled(), want3[0], "48 x 27: upscaled")
        assert_same(ctx.read_upscale_history(), want3[1], "48 x 27: history")
        # hrpt_resize drops the images; the next call runs without history
        ctx.resize(W, H)
        assert ctx.upscaled_device() is None
        with pytest.raises(native.HrptError) as e:
            ctx.read_upscaled()
        assert e.value.code == -1 and "hrpt_upscale writes it" in str(e.value)
        inp, jitter = _frame(ctx, sc, view, pos, full, 11)
        p = S.UpscaleParams(jitter=jitter)
        ctx.upscale(48, 27, full, full, p)
        want4 = native.upscale_host(inp["color"], inp["depth"], inp["motion"], None, (48, 27), full, full, p)
        assert_same(ctx.read_upscale_history(), want4[1], "after hrpt_resize")
    finally:
        ctx.close()


def test_isolation_errors_and_caller_stream(luts):
    import torch
    sc = scenes.cornell_scene(luts)
    view, pos, full = _view()
    ctx = native.PathTracerContext(0)
    try:
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        p = S.UpscaleParams()
        # before the first call: no image; planes missing is an error
        assert ctx.upscaled_device() is None
        cb = scenes.fill_constants(view, pos, sc, 0, 2)
        ctx.render(cb, accum_count=1)
        with pytest.raises(native.HrptError) as e:
            ctx.upscale(DW, DH, full, full, p)
        assert e.value.code == -1 and "never requested" in str(e.value)
        ctx.render_motion_vectors(cb, full)                                  # motion only: depth still missing
        with pytest.raises(native.HrptError) as e:
            ctx.upscale(DW, DH, full, full, p)
        assert "never requested" in str(e.value) and ctx.upscaled_device() is None
        ctx.render_motion_vectors(cb, full, planes=PLANES | (1 << S.GB_NORMAL))
        ctx.temporal_accumulate(full, full, S.TemporalParams(0.9, S.TEMPORAL_LINEAR))       # a temporal history to leave alone
        wrong = full.copy(); wrong["m_ViewportSize"] = (DW, DH)
        bad_calls = [(DW, DH, wrong, p, "m_ViewportSize"), (W - 1, DH, full, p, "display size"), (4 * W + 1, DH, full, p, "display size"),
                     (DW, 0, full, p, "1..65535"), (DW, DH, full, S.UpscaleParams(jitter=(0.6, 0.0)), "jitter"), (DW, DH, full, S.UpscaleParams(kernel=0.0), "kernel"),
                     (DW, DH, full, S.UpscaleParams(maxHistory=-1.0), "maxHistory"), (DW, DH, full, S.UpscaleParams(flags=8), "flags")]
        for dw, dh, v, params, word in bad_calls:
            with pytest.raises(native.HrptError) as e:
                ctx.upscale(dw, dh, v, full, params)
            assert e.value.code == -1 and word in str(e.value), word
        assert ctx.upscaled_device() is None                                 # bad input allocates nothing
        assert native.lib.hrpt_upscale(ctx._h, DW, DH, None, full.ctypes.data, C.byref(p)) == -1
        assert native.lib.hrpt_get_upscaled_device(ctx._h, None) == -1

        # a call leaves Output, Accumulation, the planes, the temporal history and the statistics as they were
        before, stats_before = _state(ctx)
        ctx.post_process(S.PostParams(1, 1.0, 0.016, 5.0, -7.0, 23.0, 0.0, 0, 80.0))
        exposure_before = ctx.exposure()
        ctx.upscale(DW, DH, full, full, p)
        ctx.upscale(DW, DH, full, full, p)
        after, stats_after = _state(ctx)
        for a, b in zip(before, after):
            assert np.array_equal(u32(a), u32(b))
        for field, _ in S.Stats._fields_:
            assert getattr(stats_before, field) == getattr(stats_after, field), field
        e0, e1 = exposure_before, ctx.exposure()
        assert e0[0] == e1[0] and np.array_equal(e0[1], e1[1])
        buf = np.zeros(4, np.float32)
        assert native.lib.hrpt_read_upscaled(ctx._h, buf.ctypes.data, buf.nbytes) == -1          # bytes != DW * DH * 16
        assert native.lib.hrpt_read_upscale_history(ctx._h, buf.ctypes.data, buf.nbytes) == -1

        # on a caller stream: the second call of the pair above repeated there gives the same image
        want = ctx.read_upscale_history()
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        ctx.upscale(DW, DH, full, full, S.UpscaleParams(flags=S.UPSCALE_RESET))
        ctx.upscale(DW, DH, full, full, p)
        stream.synchronize()
        on_stream = ctx.read_upscale_history()
        ctx.set_stream(None)
        assert_same(on_stream, want, "caller stream")

        # argument errors of the device call on a live context
        cpair = UC.SIZE_PAIRS[1]
        c = UC.case("zero", cpair, False)
        dev = [torch.from_numpy(np.array(c[k], np.float32)).to("cuda:0") for k in ("color", "depth", "motion")]      # a copy: the cases are read-only
        hout, cout = torch.zeros((24, 40, 4), device="cuda:0"), torch.zeros((24, 40, 4), device="cuda:0")
        ptrs = [t.data_ptr() for t in dev]
        for im, word in ((S.UpscaleImages(*ptrs, None, hout.data_ptr(), None), "null image"),
                         (S.UpscaleImages(*ptrs, hout.data_ptr(), hout.data_ptr(), cout.data_ptr()), "historyOut must differ"),
                         (S.UpscaleImages(*ptrs, None, hout.data_ptr(), hout.data_ptr()), "colorOut must differ")):
            with pytest.raises(native.HrptError) as e:
                ctx.upscale_device(im, 20, 12, 40, 24, c["view"], c["prev"])
            assert e.value.code == -1 and word in str(e.value), word
        with pytest.raises(native.HrptError) as e:
            ctx.upscale_device(S.UpscaleImages(*ptrs, None, hout.data_ptr(), cout.data_ptr()), 20, 12, 81, 24, c["view"], c["prev"])
        assert "display size" in str(e.value)
        torch.cuda.synchronize()
        assert not hout.any().item() and not cout.any().item()               # bad input changes nothing
    finally:
        ctx.close()


# ---------------------------------------------------------------- 3. hrpt_post_process_device
@pytest.mark.parametrize("auto", [1, 0], ids=["auto-exposure", "manual"])
def test_post_process_device_equals_post_process(luts, auto):
    import torch
    sc = scenes.cornell_scene(luts)
    view, pos, _ = _view()
    pp = S.PostParams(auto, 0.75, 0.016, 5.0, -7.0, 23.0, 0.0, 0, 80.0)
    results = []
    for device_call_ in (False, True):                        # two fresh contexts: the exposure history starts at 1 in both
        ctx = native.PathTracerContext(0)
        try:
            ctx.upload_scene(sc)
            ctx.resize(W, H)
            ctx.render(scenes.fill_constants(view, pos, sc, 0, 2), accum_count=2)
            if device_call_:
                hdr = torch.from_numpy(ctx.read_output()).to("cuda:0")
                display = torch.full((H, W, 4), float("nan"), device="cuda:0")
                stream = torch.cuda.current_stream()
                for _ in range(2):                            # twice: the second pass adapts from the first one's exposure
                    ctx.post_process_device(hdr.data_ptr(), display.data_ptr(), W * H, pp, stream.cuda_stream)
                stream.synchronize()
                results.append((display.cpu().numpy(), ctx.exposure()))
                with pytest.raises(native.HrptError) as e:
                    ctx.post_process_device(hdr.data_ptr(), hdr.data_ptr(), W * H, pp)
                assert "must differ" in str(e.value)
                with pytest.raises(native.HrptError):
                    ctx.post_process_device(hdr.data_ptr(), display.data_ptr(), 0, pp)
                assert native.lib.hrpt_post_process_device(ctx._h, None, display.data_ptr(), W * H, C.byref(pp), None) == -1
                assert native.lib.hrpt_post_process_device(ctx._h, hdr.data_ptr(), display.data_ptr(), W * H, None, None) == -1
            else:
                for _ in range(2):
                    ctx.post_process(pp)
                results.append((ctx.read_display(), ctx.exposure()))
        finally:
            ctx.close()
    (d0, e0), (d1, e1) = results
    assert_same(d1, d0, "display image")
    assert np.float32(e0[0]).view(np.uint32) == np.float32(e1[0]).view(np.uint32) and np.array_equal(e0[1], e1[1])
