"""Lifetime of a context's device buffers (csrc/pt_device_buffer.h: DeviceBuffer; csrc/pt_capi_internal.h: the per-scene / per-size /
per-context groups of HrptContext). One context goes twice through resize -> upload -> every call that allocates a buffer lazily -> resize to another size and
back -> upload again; every image read back in the second pass equals the first pass bit for bit, a released animation is unknown to the
context afterwards, and a second context that lives and dies between the passes changes nothing. Cornell-class scene at 16 x 8, the
gentle 4-joint pose of tests/skin_cases.py on its 28 vertices, the 5-joint skeleton of tests/anim_cases.py. No memory is measured."""
import numpy as np
import pytest

from hobbyrenderer_amd import native, scenes, structs as S
import anim_cases as AK
import deform_cases as D
import denoise_cases as DC
import skin_cases as SK
import temporal_cases as TC
from test_deform_gpu import _on_device
from test_skin_gpu import OnDevice

pytestmark = pytest.mark.gpu
W, H = 16, 8
MANUAL_EXPOSURE = S.PostParams(0, 1.0, 0.016, 5.0, -7.0, 23.0, 0.0, 0, 80.0)      # nothing adapts from one frame to the next


def _one_pass(ctx, luts, anim, tile):
    """The sequence of the module docstring, once; name -> the bytes read back at that point."""
    sc, view, pos, cfg = scenes.config_cornell(luts, W, H)
    full = view.copy()
    full["m_CameraDirectionOrPosition"] = (pos[0], pos[1], pos[2], 1.0)
    cb = scenes.fill_constants(view, pos, sc, 0, cfg["max_bounces"])
    cbm = cb.copy()
    cbm["m_Jitter"] = (0.0, 0.0)
    got = {}

    def keep(name, image):
        assert name not in got
        got[name] = np.ascontiguousarray(image).tobytes()

    ctx.resize(W, H)
    ctx.upload_scene(sc)
    ctx.set_denoise_noise(None)                          # the default tile, whatever the pass before left
    # the frame: render, G-buffer with all planes, motion vectors, demodulate, temporal, denoise (both ways), compose, bloom, post
    ctx.clear_accumulation()
    ctx.render(cb, accum_count=2)
    keep("accumulation", ctx.read_accumulation())
    keep("output", ctx.read_output())
    ctx.render_gbuffer(cbm, planes=S.GB_ALL_PLANES)
    ctx.render_motion_vectors(cbm, full, planes=S.GB_ALL_PLANES)
    for plane in range(S.GB_PLANES):
        keep(f"gbuffer {plane}", ctx.read_gbuffer(plane))
    keep("motion", ctx.read_motion_vectors())
    ctx.demodulate(full)
    keep("modulation", ctx.read_modulation())
    ctx.temporal_accumulate(full, full, TC.params(0.9, False))
    keep("temporal history", ctx.read_temporal_history())
    ctx.denoise(full, DC.params(3.0, 0, iterations=2))
    keep("denoised history", ctx.read_temporal_history())
    keep("denoised output", ctx.read_output())
    ctx.denoise(full, DC.params(3.0, 1, iterations=2, flags=S.DENOISE_OUTPUT_ONLY))
    keep("history after output-only", ctx.read_temporal_history())
    keep("output-only output", ctx.read_output())
    ctx.compose()
    ctx.bloom()
    keep("bloomed output", ctx.read_output())
    ctx.post_process(MANUAL_EXPOSURE)
    keep("display", ctx.read_display())
    # geometry: floats quantised on the device, the skinned update, the animation
    _, floats = D.deformed(sc, 0, 28, 1, 0.02)
    ctx.update_vertices_device(_on_device(floats).data_ptr(), 0, 28)
    pose = OnDevice(SK.gentle_pose(floats, 4, 3, amplitude=0.02))
    ctx.update_vertices_skinned(*pose.args, 0)
    anim.set_times(AK.cases()["skin5"]["times"][0])
    ctx.animate(anim)
    for name, array in zip(("palette", "morph weights", "node worlds"), ctx.read_animation(anim)):
        keep(name, array)
    ctx.clear_accumulation()
    ctx.render(cb, accum_count=1)
    keep("posed accumulation", ctx.read_accumulation())
    ctx.render_motion_vectors(cbm, full, planes=1 << S.GB_DEPTH)      # the previous positions of both updates reach the device here
    keep("posed motion", ctx.read_motion_vectors())
    ctx.set_denoise_noise(tile)
    ctx.denoise(full, DC.params(3.0, 2, flags=S.DENOISE_OUTPUT_ONLY))
    keep("caller-tile output", ctx.read_output())
    # another size and back, then the scene again: what depends on the size or on the scene is gone, the rest stays usable
    ctx.resize(H, W)
    ctx.resize(W, H)
    ctx.upload_scene(sc)
    ctx.render(cb, accum_count=1)
    keep("accumulation after the second upload", ctx.read_accumulation())
    ctx.release_animation(anim)
    with pytest.raises(native.HrptError) as e:
        ctx.animation_device(anim)
    assert e.value.code == -1 and "hrpt_animate has not run for this animation" in str(e.value)
    return got


def test_two_passes_over_one_context_give_the_same_bits(luts):
    anim = native.Animation(**AK.cases()["skin5"]["tables"])
    tile = DC.caller_tile()
    ctx = native.PathTracerContext(0)
    try:
        first = _one_pass(ctx, luts, anim, tile)
        other = native.PathTracerContext(0)              # lives and dies between the passes, with buffers of every lifetime
        try:
            _one_pass(other, luts, anim, tile)
        finally:
            other.close()
        second = _one_pass(ctx, luts, anim, tile)
    finally:
        ctx.close(); anim.close()
    assert list(first) == list(second)
    differing = [name for name in first if first[name] != second[name]]
    assert not differing, differing
    # the passes did something: the pose moved the image and left motion behind, the stages wrote what they own
    assert first["posed accumulation"] != first["accumulation after the second upload"]
    assert any(first["posed motion"]) and any(first["modulation"]) and any(first["display"])
