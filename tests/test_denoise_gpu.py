"""The denoise stage on the device (hrpt_denoise_device / hrpt_denoise): the gfx950 kernel against the host executor
and the NumPy restatement (tests/denoise_reference.py), bit for bit on uint32 views with no pixel left out; the context path over a real
scene in the documented frame order -- iterated passes, the denoised image as the next frame's history, HRPT_DENOISE_OUTPUT_ONLY -- and
what the stage must leave alone."""
import ctypes as C

import numpy as np
import pytest

from hobbyrenderer_amd import native, scenes, structs as S
import denoise_cases as DC
import denoise_reference as R
import temporal_cases as TC
from test_denoise_cpu import KEYS, assert_same, u32
from test_temporal_gpu import H, SPP, W, _view

pytestmark = pytest.mark.gpu

PLANES = (1 << S.GB_DEPTH) | (1 << S.GB_NORMAL) | (1 << S.GB_GEO_NORMAL)


@pytest.fixture(scope="module")
def ctx0():
    ctx = native.PathTracerContext(0)
    yield ctx
    ctx.close()


def device_call(ctx, c, radius, frame, noise=None, color=False, in_place=False):
    """hrpt_denoise_device over torch tensors on the current torch stream; returns output, or (output, colorOut), as host arrays."""
    import torch
    h, w = c["input"].shape[:2]
    dev = [torch.from_numpy(np.ascontiguousarray(c[k], np.float32)).to("cuda:0") for k in KEYS]
    tile = None if noise is None else torch.from_numpy(np.ascontiguousarray(noise, np.float32)).to("cuda:0")
    out = torch.full((h, w, 4), float("nan"), device="cuda:0")
    col = cout = None
    if color:
        col = torch.from_numpy(np.ascontiguousarray(c["color"], np.float32)).to("cuda:0")
        cout = col if in_place else torch.full((h, w, 4), float("nan"), device="cuda:0")
    im = S.DenoiseImages(*[t.data_ptr() for t in dev], None if tile is None else tile.data_ptr(), out.data_ptr(),
                         None if col is None else col.data_ptr(), None if cout is None else cout.data_ptr())
    stream = torch.cuda.current_stream()
    ctx.denoise_device(im, w, h, c["view"], DC.params(radius, frame), stream.cuda_stream)
    stream.synchronize()
    return (out.cpu().numpy(), cout.cpu().numpy()) if color else out.cpu().numpy()


def host_call(c, radius, frame, noise=None, color=None):
    return native.denoise_host(*[c[k] for k in KEYS], c["view"], DC.params(radius, frame), noise=noise, color=color)


def check_case(ctx, c, radius, frames, what):
    tile = DC.caller_tile()
    for k, frame in enumerate(frames):
        for noise in (None, tile):
            label = f"{what} radius={radius} frame={frame} tile={'caller' if noise is not None else 'default'}"
            ref, ref_col = R.denoise(*[c[k2] for k2 in KEYS], c["view"], radius=radius, frame=frame, noise=noise, color=c["color"])
            host, host_col = host_call(c, radius, frame, noise, c["color"])
            dev, dev_col = device_call(ctx, c, radius, frame, noise, color=True, in_place=(k % 2 == 1))
            assert_same(dev, host, label + ": device vs host, output")
            assert_same(dev, ref, label + ": device vs reference, output")
            assert_same(dev_col, host_col, label + ": device vs host, colorOut")
            assert_same(dev_col, ref_col, label + ": device vs reference, colorOut")
            assert_same(device_call(ctx, c, radius, frame, noise), ref, label + ": device without the colour pair")


# ---------------------------------------------------------------- 1. device == host == NumPy on the synthetic cases
@pytest.mark.parametrize("size", DC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("radius", DC.RADII)
def test_device_equals_host_and_reference(ctx0, radius, size):
    w, h = size
    check_case(ctx0, DC.case(w, h), radius, DC.FRAMES, f"{w}x{h}")


@pytest.mark.parametrize("size", [(1, 1), (2, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiny_images(ctx0, size):
    w, h = size
    for radius in DC.RADII:
        check_case(ctx0, DC.case(w, h), radius, (0, 4097), f"{w}x{h}")


def test_many_tiles_and_partial_tiles(ctx0):
    """200 x 120: 7 x 15 tiles of 32 x 8, partial on the right edge; radius 12 reaches 48 texels, across several tiles."""
    w, h = 200, 120
    check_case(ctx0, DC.case(w, h), 12.0, (4096,), "200x120")


# ---------------------------------------------------------------- 2. the context path over a scene
RADIUS = 3.0


def _frame(ctx, sc, view, pos, full, prev_full, frame, tparams):
    """One frame of the documented order up to and including hrpt_temporal_accumulate; returns the read-backs the host chain needs."""
    cb = scenes.fill_constants(view, pos, sc, frame * SPP, 2)
    ctx.clear_accumulation()
    ctx.render(cb, accum_count=SPP)
    cbm = cb.copy()
    cbm["m_Jitter"] = (0.0, 0.0)
    ctx.render_motion_vectors(cbm, prev_full, planes=PLANES)
    inputs = dict(color=ctx.read_output(), motion=ctx.read_motion_vectors(), depth=ctx.read_gbuffer(S.GB_DEPTH), normal=ctx.read_gbuffer(S.GB_NORMAL),
                  geo=ctx.read_gbuffer(S.GB_GEO_NORMAL))
    ctx.temporal_accumulate(full, prev_full, tparams)
    inputs["output"], inputs["history"] = ctx.read_output(), ctx.read_temporal_history()
    return inputs


def _host_chain(f, full, iterations, frame, radius=RADIUS):
    """What hrpt_denoise computes from a frame's read-backs: `iterations` chained host passes; pass i uses radius * 2^i and
    frame * iterations + i (uint32), the last one also gives Output."""
    x = f["history"]
    for i in range(iterations):
        p = DC.params(radius * float(1 << i), (frame * iterations + i) & 0xFFFFFFFF)
        last = i + 1 == iterations
        r = native.denoise_host(x, f["depth"], f["normal"], f["geo"], full, p, color=f["output"] if last else None)
        x, out = r if last else (r, None)
    return x, out


def _scene_context(luts):
    sc = scenes.cube_scene(luts)
    ctx = native.PathTracerContext(0)
    ctx.upload_scene(sc)
    ctx.resize(W, H)
    records = sc.instances.copy()
    records["m_PrevWorld"] = records["m_World"]
    ctx.update_instances(records, 0)
    return sc, ctx


@pytest.mark.parametrize("iterations", [3, 1, 2])
def test_context_path_denoised_history_feeds_the_next_frame(luts, iterations):
    """Three frames: temporal -> denoise every frame. Output and the history equal the chained host passes over the read-backs, and the next
    temporal call reprojects the DENOISED history. iterations 1 and 2 flip the ping-pong pair an odd and an even number of times."""
    sc, ctx = _scene_context(luts)
    view, pos, full = _view()
    tparams = TC.params(0.9, False)
    try:
        history = None
        for frame, number in enumerate((7, 0xFFFFFFFF, 8)):      # the middle frame number makes frame * iterations + i wrap
            f = _frame(ctx, sc, view, pos, full, full, frame, tparams)
            want_out, want_hist = native.temporal_host(f["color"], f["motion"], f["depth"], f["normal"], history, full, full, tparams)
            assert_same(f["output"], want_out, f"frame {frame}: temporal Output")
            assert_same(f["history"], want_hist, f"frame {frame}: temporal history (fed with the denoised one)")
            if frame:
                assert (f["history"][..., 3] > 0.5).any()
            ctx.denoise(full, DC.params(RADIUS, number, iterations))
            hist, out = _host_chain(f, full, iterations, number)
            assert_same(ctx.read_temporal_history(), hist, f"frame {frame}: denoised history")
            assert_same(ctx.read_output(), out, f"frame {frame}: denoised Output")
            hit = f["depth"][..., 0] != np.float32(1e10)
            assert 0 < hit.sum() < hit.size and (u32(hist[hit]) != u32(f["history"][hit])).any()
            assert np.array_equal(u32(out[..., 3]), u32(f["output"][..., 3]))
            ptr = ctx.temporal_history_device()
            assert ptr
            history = hist
    finally:
        ctx.close()


def test_output_only_leaves_the_history_alone(luts):
    sc, ctx = _scene_context(luts)
    view, pos, full = _view()
    tparams = TC.params(0.9, True)
    try:
        history = None
        for frame, iterations in enumerate((2, 1, 3)):
            f = _frame(ctx, sc, view, pos, full, full, frame, tparams)
            want_out, want_hist = native.temporal_host(f["color"], f["motion"], f["depth"], f["normal"], history, full, full, tparams)
            assert_same(f["history"], want_hist, f"frame {frame}: temporal history (fed with the unfiltered one)")
            ptr = ctx.temporal_history_device()
            ctx.denoise(full, DC.params(RADIUS, frame, iterations, S.DENOISE_OUTPUT_ONLY))
            _, out = _host_chain(f, full, iterations, frame)
            assert_same(ctx.read_output(), out, f"frame {frame}: denoised Output")
            assert (u32(out) != u32(f["output"])).any()
            assert_same(ctx.read_temporal_history(), f["history"], f"frame {frame}: history after HRPT_DENOISE_OUTPUT_ONLY")
            assert ctx.temporal_history_device() == ptr
            history = f["history"]
        # hrpt_resize drops the history and the scratch pair: an error until the temporal stage has run again, then the same results
        ctx.resize(W, H)
        with pytest.raises(native.HrptError) as e:
            ctx.denoise(full, DC.params(RADIUS, 0, 2, S.DENOISE_OUTPUT_ONLY))
        assert e.value.code == -1 and "hrpt_temporal_accumulate" in str(e.value)
        f = _frame(ctx, sc, view, pos, full, full, 5, tparams)
        ctx.denoise(full, DC.params(RADIUS, 5, 2, S.DENOISE_OUTPUT_ONLY))
        assert_same(ctx.read_output(), _host_chain(f, full, 2, 5)[1], "after hrpt_resize: denoised Output")
        assert_same(ctx.read_temporal_history(), f["history"], "after hrpt_resize: history")
    finally:
        ctx.close()


def test_isolation_errors_and_caller_stream(luts):
    import torch
    sc, ctx = _scene_context(luts)
    view, pos, full = _view()
    tparams = TC.params(0.9, False)
    try:
        cb = scenes.fill_constants(view, pos, sc, 0, 2)
        ctx.render(cb, accum_count=SPP)
        ctx.render_motion_vectors(cb, full, planes=PLANES)
        with pytest.raises(native.HrptError) as e:               # no temporal history yet
            ctx.denoise(full)
        assert e.value.code == -1 and "hrpt_temporal_accumulate" in str(e.value)
        assert ctx.temporal_history_device() is None
    finally:
        ctx.close()

    sc, ctx = _scene_context(luts)
    try:
        cb = scenes.fill_constants(view, pos, sc, 0, 2)
        ctx.render(cb, accum_count=SPP)
        ctx.render_motion_vectors(cb, full, planes=(1 << S.GB_DEPTH) | (1 << S.GB_NORMAL))
        ctx.temporal_accumulate(full, full, tparams)
        before = ctx.read_temporal_history()
        with pytest.raises(native.HrptError) as e:               # the geo-normal plane (metallic) was never requested
            ctx.denoise(full)
        assert e.value.code == -1 and "never requested" in str(e.value)
        f = _frame(ctx, sc, view, pos, full, full, 1, tparams)
        wrong = full.copy(); wrong["m_ViewportSize"] = (W, H + 1)
        with pytest.raises(native.HrptError) as e:
            ctx.denoise(wrong)
        assert "m_ViewportSize" in str(e.value)
        for bad in (S.DenoiseParams(radius=0.0), S.DenoiseParams(iterations=6), S.DenoiseParams(iterations=0), S.DenoiseParams(flags=2),
                    S.DenoiseParams(phi=float("nan")), S.DenoiseParams(radius=3e38, iterations=2)):
            with pytest.raises(native.HrptError):
                ctx.denoise(full, bad)
        assert native.lib.hrpt_denoise(ctx._h, None, C.byref(S.DenoiseParams())) == -1
        assert native.lib.hrpt_denoise(ctx._h, full.ctypes.data, None) == -1
        assert_same(ctx.read_temporal_history(), f["history"], "refused calls leave the history alone")
        assert (u32(before) != u32(f["history"])).any()

        # a call leaves Accumulation, the planes, the motion plane, exposure and the statistics as they were
        ctx.post_process(S.PostParams(1, 1.0, 0.016, 5.0, -7.0, 23.0, 0.0, 0, 80.0))

        def state():
            images = [ctx.read_accumulation(), ctx.read_motion_vectors()] + [ctx.read_gbuffer(k) for k in (S.GB_DEPTH, S.GB_NORMAL, S.GB_GEO_NORMAL)]
            return images, ctx.exposure(), ctx.stats()
        images_before, exposure_before, stats_before = state()
        ctx.denoise(full, DC.params(RADIUS, 3, 2))
        images_after, exposure_after, stats_after = state()
        for a, b in zip(images_before, images_after):
            assert np.array_equal(u32(a), u32(b))
        assert exposure_before[0] == exposure_after[0] and np.array_equal(exposure_before[1], exposure_after[1])
        for field, _ in S.Stats._fields_:
            assert getattr(stats_before, field) == getattr(stats_after, field), field
        hist, out = _host_chain(f, full, 2, 3)
        assert_same(ctx.read_temporal_history(), hist, "default call: history")
        assert_same(ctx.read_output(), out, "default call: Output")

        # on a caller stream
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        f = _frame(ctx, sc, view, pos, full, full, 2, tparams)
        ctx.denoise(full, DC.params(RADIUS, 4, 3))
        stream.synchronize()
        got_hist, got_out = ctx.read_temporal_history(), ctx.read_output()
        ctx.set_stream(None)
        hist, out = _host_chain(f, full, 3, 4)
        assert_same(got_hist, hist, "caller stream: history")
        assert_same(got_out, out, "caller stream: Output")
    finally:
        ctx.close()
