"""The temporal stage on the device (hrpt_temporal_device / hrpt_temporal_accumulate / hrpt_clear_accumulation):
the gfx950 kernel against the host executor and the NumPy restatement (tests/temporal_reference.py), bit for bit on uint32 views with no
pixel left out; the context path over a real scene through static frames, a camera move and an instance move; the cleared accumulation on
both kernel paths; and what the stage must leave alone."""
import ctypes as C
import math

import numpy as np
import pytest

from hobbyrenderer_amd import native, scenes, structs as S
import temporal_cases as TC
import temporal_reference as R
from test_temporal_cpu import assert_same, u32

pytestmark = pytest.mark.gpu

PATHS = [("wavefront", S.FRAME_WAVEFRONT), ("megakernel", S.FRAME_MEGAKERNEL)]
PLANES = (1 << S.GB_DEPTH) | (1 << S.GB_NORMAL)


@pytest.fixture(scope="module")
def ctx0():
    ctx = native.PathTracerContext(0)
    yield ctx
    ctx.close()


def device_call(ctx, c, history, linear, in_place=False):
    """hrpt_temporal_device over torch tensors on the current torch stream; returns (colorOut, historyOut) as host arrays."""
    import torch
    h, w = c["color"].shape[:2]
    dev = [torch.from_numpy(np.ascontiguousarray(c[k], np.float32)).to("cuda:0") for k in ("color", "motion", "depth", "normal")]
    hist = None if history is None else torch.from_numpy(np.ascontiguousarray(history, np.float32)).to("cuda:0")
    hout = torch.full((h, w, 4), float("nan"), device="cuda:0")
    cout = dev[0] if in_place else torch.full((h, w, 4), float("nan"), device="cuda:0")
    im = S.TemporalImages(*[t.data_ptr() for t in dev], None if hist is None else hist.data_ptr(), hout.data_ptr(), cout.data_ptr())
    stream = torch.cuda.current_stream()
    ctx.temporal_device(im, w, h, c["view"], c["prev"], TC.params(c["blend"], linear), stream.cuda_stream)
    stream.synchronize()
    return cout.cpu().numpy(), hout.cpu().numpy()


# ---------------------------------------------------------------- 1. device == host == NumPy on the synthetic cases
@pytest.mark.parametrize("size", TC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", TC.MOTIONS)
def test_device_equals_host_and_reference(ctx0, name, size):
    w, h = size
    for jitter in (False, True):
        c = TC.case(name, w, h, jitter)
        for linear in (False, True):
            for hist in (None, c["history"]):
                what = f"{name} {w}x{h} jitter={jitter} linear={linear} history={hist is not None}"
                dev = device_call(ctx0, c, hist, linear, in_place=jitter)
                host = native.temporal_host(c["color"], c["motion"], c["depth"], c["normal"], hist, c["view"], c["prev"], TC.params(c["blend"], linear))
                ref = R.temporal(c["color"], c["motion"], c["depth"], c["normal"], hist, c["view"], c["prev"], blend=c["blend"], linear=linear)
                for k, plane in enumerate(("colorOut", "historyOut")):
                    assert_same(dev[k], host[k], f"{what}: device vs host, {plane}")
                    assert_same(dev[k], ref[k], f"{what}: device vs reference, {plane}")


def test_many_tiles_and_partial_tiles(ctx0):
    """200 x 120 with the random motion field: 7 x 15 tiles of 32 x 8, partial on the right edge."""
    w, h = 200, 120
    c = TC.case("random", w, h, True)
    for linear in (False, True):
        dev = device_call(ctx0, c, c["history"], linear)
        host = native.temporal_host(c["color"], c["motion"], c["depth"], c["normal"], c["history"], c["view"], c["prev"], TC.params(c["blend"], linear))
        ref = R.temporal(c["color"], c["motion"], c["depth"], c["normal"], c["history"], c["view"], c["prev"], blend=c["blend"], linear=linear)
        for k, plane in enumerate(("colorOut", "historyOut")):
            assert_same(dev[k], host[k], f"200x120 linear={linear}: device vs host, {plane}")
            assert_same(dev[k], ref[k], f"200x120 linear={linear}: device vs reference, {plane}")


# ---------------------------------------------------------------- 2. the context path over a scene
W, H, SPP = 64, 36, 2
YAW, PITCH = math.atan2(-2.0, 3.0), math.asin(1.5 / math.sqrt(15.25))


def _view(yaw_offset=0.0):
    view, pos = scenes.planar_view(W, H, position=(2.0, 1.5, -3.0), yaw=YAW + yaw_offset, pitch=PITCH)
    full = view.copy()
    full["m_CameraDirectionOrPosition"] = (pos[0], pos[1], pos[2], 1.0)       # planar_view leaves it zero; the temporal stage reads it
    return view, pos, full


def _frame(ctx, sc, view, pos, full, prev_full, frame, params):
    """One frame of the documented order; returns the read-backs the reference needs and what the stage left behind."""
    cb = scenes.fill_constants(view, pos, sc, frame * SPP, 2)
    ctx.clear_accumulation()
    ctx.render(cb, accum_count=SPP)
    cbm = cb.copy()
    cbm["m_Jitter"] = (0.0, 0.0)            # the planes' primary rays without the per-index jitter: the same hit mask every static frame
    ctx.render_motion_vectors(cbm, prev_full, planes=PLANES)
    color = ctx.read_output()
    inputs = dict(color=color, motion=ctx.read_motion_vectors(), depth=ctx.read_gbuffer(S.GB_DEPTH), normal=ctx.read_gbuffer(S.GB_NORMAL))
    ctx.temporal_accumulate(full, prev_full, params)
    return inputs, ctx.read_output(), ctx.read_temporal_history()


@pytest.mark.parametrize("linear", [True, False], ids=["linear", "reference-space"])
def test_context_path_static_camera_move_instance_move(luts, linear):
    sc = scenes.cube_scene(luts)
    params = TC.params(0.9, linear)
    view, pos, full = _view()
    ctx = native.PathTracerContext(0)
    try:
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        records = sc.instances.copy()
        records["m_PrevWorld"] = records["m_World"]
        ctx.update_instances(records, 0)
        history = None
        prev_full = full
        outputs = []
        for frame in range(6):
            if frame == 4:                                    # the camera yaws; last frame's view becomes prevView
                prev_full = full
                view, pos, full = _view(0.05)
            if frame == 5:                                    # an instance moves, by the m_PrevWorld protocol of section 16
                prev_full = full
                records = records.copy()
                records["m_PrevWorld"] = records["m_World"]
                moved = records["m_World"][0].astype(np.float64); moved[3, :3] += (0.12, 0.05, -0.08)
                records["m_World"][0] = moved.astype(np.float32)
                ctx.update_instances(records, 0)
            inp, out, hist = _frame(ctx, sc, view, pos, full, prev_full, frame, params)
            ref_out, ref_hist, d = R.temporal(inp["color"], inp["motion"], inp["depth"], inp["normal"], history, full, prev_full, linear=linear, details=True)
            assert_same(out, ref_out, f"frame {frame}: Output")
            assert_same(hist, ref_hist, f"frame {frame}: history")
            hit = ~d["miss"]
            assert 0 < hit.sum() < hit.size
            if frame < 4:
                outputs.append(inp["color"])
                assert not u32(inp["motion"][..., :3]).any()
                np.testing.assert_allclose(hist[..., 3][hit], float(frame), rtol=1e-3)
                if linear and frame:
                    mean = np.mean([o[..., :3].astype(np.float64) for o in outputs], 0)
                    np.testing.assert_allclose(out[..., :3][hit], mean[hit], rtol=1e-4)
            else:                                             # something moved: pixels that reproject with confidence and pixels that do not
                assert np.hypot(inp["motion"][..., 0], inp["motion"][..., 1])[hit].max() > 0.5
                assert (d["confidence"][hit] > 0.5).any() and (hist[..., 3][hit] > 1.0).any()
            prev_full = full
            history = hist
    finally:
        ctx.close()


# ---------------------------------------------------------------- 3. hrpt_clear_accumulation
@pytest.mark.parametrize("label,flags", PATHS)
def test_clear_accumulation_starts_a_frame_at_a_nonzero_index(luts, label, flags):
    sc = scenes.cube_scene(luts)
    view, pos, _ = _view()
    constants = lambda i: scenes.fill_constants(view, pos, sc, i, 2)       # noqa: E731
    ctx = native.PathTracerContext(0)
    try:
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        ctx.render(constants(0), accum_count=4, flags=flags)                # something to clear
        singles = []
        for k in (7, 8, 9):
            ctx.clear_accumulation()
            ctx.render(constants(k), accum_count=1, flags=flags)
            a = ctx.read_accumulation()
            assert (a[..., 3] == 1).all()
            singles.append(a[..., :3])
        ctx.clear_accumulation()
        assert not u32(ctx.read_accumulation()).any()
        ctx.render(constants(7), accum_count=3, flags=flags)
        acc, out = ctx.read_accumulation(), ctx.read_output()
        assert (acc[..., 3] == 3).all()
        assert np.array_equal(u32(acc[..., :3]), u32((singles[0] + singles[1]) + singles[2])), label     # exactly the indices 7, 8, 9
        assert np.array_equal(u32(out[..., :3]), u32(acc[..., :3] / np.float32(3))) and (out[..., 3] == 1).all()
        ctx.render(constants(7), accum_count=3, flags=flags)                # without the clear the alpha keeps growing
        assert (ctx.read_accumulation()[..., 3] == 6).all()
    finally:
        ctx.close()


# ---------------------------------------------------------------- 4. isolation and protocol
def test_isolation_reset_resize_errors_and_caller_stream(luts):
    import torch
    sc = scenes.cube_scene(luts)
    view, pos, full = _view()
    linear = TC.params(0.9, True)
    ctx = native.PathTracerContext(0)
    try:
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        # before the first call: no history image; planes missing is an error
        assert ctx.temporal_history_device() is None
        with pytest.raises(native.HrptError) as e:
            ctx.read_temporal_history()
        assert e.value.code == -1 and "never requested" in str(e.value)
        cb = scenes.fill_constants(view, pos, sc, 0, 2)
        ctx.render(cb, accum_count=SPP)
        with pytest.raises(native.HrptError) as e:
            ctx.temporal_accumulate(full, full, linear)
        assert e.value.code == -1 and "never requested" in str(e.value)
        ctx.render_motion_vectors(cb, full)                                  # motion only: depth and normal still missing
        with pytest.raises(native.HrptError):
            ctx.temporal_accumulate(full, full, linear)
        assert ctx.temporal_history_device() is None
        ctx.render_motion_vectors(cb, full, planes=PLANES | (1 << S.GB_ALBEDO))
        wrong = full.copy(); wrong["m_ViewportSize"] = (W, H + 1)
        with pytest.raises(native.HrptError) as e:
            ctx.temporal_accumulate(wrong, full, linear)
        assert "m_ViewportSize" in str(e.value) and ctx.temporal_history_device() is None
        for bad in (S.TemporalParams(1.5), S.TemporalParams(0.9, 8)):
            with pytest.raises(native.HrptError):
                ctx.temporal_accumulate(full, full, bad)
        assert native.lib.hrpt_temporal_accumulate(ctx._h, None, full.ctypes.data, C.byref(linear)) == -1
        assert native.lib.hrpt_get_temporal_history_device(ctx._h, None) == -1

        # a call leaves Accumulation, the planes, the motion plane and the statistics as they were
        def state():
            return [ctx.read_accumulation(), ctx.read_motion_vectors()] + [ctx.read_gbuffer(k) for k in (S.GB_DEPTH, S.GB_NORMAL, S.GB_ALBEDO)], ctx.stats()
        before, stats_before = state()
        color = ctx.read_output()
        ctx.temporal_accumulate(full, full, linear)
        first = ctx.read_temporal_history()
        after, stats_after = state()
        for a, b in zip(before, after):
            assert np.array_equal(u32(a), u32(b))
        for field, _ in S.Stats._fields_:
            assert getattr(stats_before, field) == getattr(stats_after, field), field
        assert ctx.temporal_history_device()
        ref0 = R.temporal(color, before[1], before[2], before[3], None, full, full, linear=True)
        assert_same(ctx.read_output(), ref0[0], "first call: no history")
        assert_same(first, ref0[1], "first call: history")
        buf = np.zeros(4, np.float32)
        assert native.lib.hrpt_read_temporal_history(ctx._h, buf.ctypes.data, buf.nbytes) == -1          # bytes != W * H * 16

        # a render after it re-resolves Output from the accumulation
        cb2 = scenes.fill_constants(view, pos, sc, SPP, 2)
        ctx.render(cb2, accum_count=SPP)
        acc = ctx.read_accumulation()
        color2 = ctx.read_output()
        assert np.array_equal(u32(color2[..., :3]), u32(acc[..., :3] / acc[..., 3:4]))

        # second call uses the history; HRPT_TEMPORAL_RESET ignores it
        ctx.temporal_accumulate(full, full, linear)
        ref1 = R.temporal(color2, before[1], before[2], before[3], first, full, full, linear=True)
        assert_same(ctx.read_temporal_history(), ref1[1], "second call: with history")
        assert (ref1[1][..., 3] > 0.5).any()
        ctx.render(cb2, accum_count=SPP)                                     # same indices onto the kept accumulation: another Output
        color3 = ctx.read_output()
        ctx.temporal_accumulate(full, full, TC.params(0.9, True, S.TEMPORAL_RESET))
        ref_reset = R.temporal(color3, before[1], before[2], before[3], None, full, full, linear=True)
        assert_same(ctx.read_temporal_history(), ref_reset[1], "HRPT_TEMPORAL_RESET")
        assert not u32(ctx.read_temporal_history()[..., 3]).any()

        # on a caller stream
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        ctx.render(cb2, accum_count=SPP)
        ctx.render_motion_vectors(cb2, full, planes=PLANES)
        ctx.temporal_accumulate(full, full, linear)
        stream.synchronize()
        on_stream = ctx.read_temporal_history()
        ctx.set_stream(None)
        assert (on_stream[..., 3] > 0.5).any()                               # the reset call's history was used

        # hrpt_resize drops the history: zeroed images of the new size, and the next call runs without history
        ctx.resize(W, H)
        assert not u32(ctx.read_temporal_history()).any()
        ctx.render(cb, accum_count=SPP)
        ctx.render_motion_vectors(cb, full, planes=PLANES)
        color4 = ctx.read_output()
        ctx.temporal_accumulate(full, full, linear)
        ref4 = R.temporal(color4, ctx.read_motion_vectors(), ctx.read_gbuffer(S.GB_DEPTH), ctx.read_gbuffer(S.GB_NORMAL), None, full, full, linear=True)
        assert_same(ctx.read_temporal_history(), ref4[1], "after hrpt_resize")
    finally:
        ctx.close()
