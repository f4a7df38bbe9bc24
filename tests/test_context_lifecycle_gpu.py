"""Lifetime of a context's device buffers (csrc/pt_device_buffer.h: DeviceBuffer; csrc/pt_capi_internal.h: the per-scene / per-size /
per-context groups of HrptContext). One context goes twice through resize -> upload -> every call that allocates a buffer lazily -> resize to another size and
back -> upload again; every image read back in the second pass equals the first pass bit for bit, a released animation is unknown to the
context afterwards, and a second context that lives and dies between the passes changes nothing. Cornell-class scene at 16 x 8, the
gentle 4-joint pose of tests/skin_cases.py on its 28 vertices, the 5-joint skeleton of tests/anim_cases.py. No memory is measured.

The stages whose images or scratch a resize drops are in the sequence too: temporal upscaling at two display sizes, the probe irradiance
plane, deferred lighting with one and then three lights (its ray and hit records grow), traced indirect lighting with one and then both
lobes (its records grow). After the resize there and back their read-backs fail until the stage has run again, the two calls on grown
scratch equal the same call on a fresh context bit for bit, and HrptStats::queuePoolBytes ends where a fresh context's does."""
import numpy as np
import pytest

from hobbyrenderer_amd import native, scenes, structs as S
import anim_cases as AK
import deferred_cases as DFC
import deform_cases as D
import denoise_cases as DC
import skin_cases as SK
import temporal_cases as TC
from test_deform_gpu import _on_device
from test_skin_gpu import OnDevice

pytestmark = pytest.mark.gpu
W, H = 16, 8
MANUAL_EXPOSURE = S.PostParams(0, 1.0, 0.016, 5.0, -7.0, 23.0, 0.0, 0, 80.0)      # nothing adapts from one frame to the next
UPSCALE_SIZES = ((24, 12), (32, 16))
PROBE_VOLUME = dict(origin=(-0.5, 0.5, -1.5), spacing=(1.0, 1.0, 1.5), counts=(2, 2, 2), rays_per_probe=8, max_ray_distance=4.0)
THREE_LIGHTS = DFC.case(33, 9)["lights"][:3]             # a spot, a point and a directional light
INDIRECT_SEED = 3
DROPPED_BY_RESIZE = (("read_upscaled", (), "no upscaled image"), ("read_probe_irradiance", (), "at the current size"), ("read_indirect", (0,), "at the current size"))


BOTH_LOBES = S.INDIRECT_DIFFUSE | S.INDIRECT_SPECULAR


def _deferred(ctx, cbm, lights):
    """Deferred lighting with traced shadows under `lights` (min(lights, 4) per batch: ray and hit records for pixels x lights); Output."""
    ctx.update_lights(lights)
    ctx.deferred_lighting(DFC.with_lights(cbm, len(lights)), S.DeferredParams(S.DEFERRED_SHADOWS))
    return ctx.read_output()


def _indirect(ctx, cbm, flags):
    """Traced indirect lighting with the lobes of `flags` (ray and radiance records for pixels x lobes); the diffuse and the specular plane."""
    ctx.indirect_lighting(cbm, S.IndirectParams(flags, INDIRECT_SEED, 0.5))
    return ctx.read_indirect(0), ctx.read_indirect(1)


def _lighting(ctx, sc, cbm, keep):
    """One light and then THREE_LIGHTS (three times the ray and hit records), the diffuse lobe and then both (twice the records), compose.
    The G-buffer planes of `cbm` are in place; the scene's own lights are back afterwards."""
    keep("deferred, one light", _deferred(ctx, cbm, sc.lights))
    keep("deferred, three lights", _deferred(ctx, cbm, THREE_LIGHTS))
    ctx.update_lights(sc.lights)
    keep("indirect diffuse, one lobe", _indirect(ctx, cbm, S.INDIRECT_DIFFUSE)[0])
    diffuse, specular = _indirect(ctx, cbm, BOTH_LOBES)
    keep("indirect diffuse, both lobes", diffuse)
    keep("indirect specular, both lobes", specular)
    ctx.indirect_compose(S.IndirectParams(BOTH_LOBES, INDIRECT_SEED, 0.5))
    keep("output with indirect", ctx.read_output())


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
    # the stages a resize leaves nothing of: upscale at two display sizes, the probe plane, deferred and indirect lighting on growing scratch
    for dw, dh in UPSCALE_SIZES:
        ctx.upscale(dw, dh, full, full)
        keep(f"upscaled {dw} x {dh}", ctx.read_upscaled())
        keep(f"upscale history {dw} x {dh}", ctx.read_upscale_history())
    probes = native.ProbeVolume(ctx, native.probe_volume(**PROBE_VOLUME))
    try:
        probes.update(cb, 1)
        probes.shade_gbuffer(full, 1.0)
        keep("probe irradiance", ctx.read_probe_irradiance())
    finally:
        probes.close()
    _lighting(ctx, sc, cbm, keep)
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
    for read, args, words in DROPPED_BY_RESIZE:          # nothing of the old size is left to read
        with pytest.raises(native.HrptError) as e:
            getattr(ctx, read)(*args)
        assert e.value.code == -1 and words in str(e.value), read
    ctx.upload_scene(sc)
    ctx.render(cb, accum_count=1)
    keep("accumulation after the second upload", ctx.read_accumulation())
    ctx.release_animation(anim)
    with pytest.raises(native.HrptError) as e:
        ctx.animation_device(anim)
    assert e.value.code == -1 and "hrpt_animate has not run for this animation" in str(e.value)
    got["queue pool bytes"] = int(ctx.stats().queuePoolBytes)
    return got


@pytest.fixture(scope="module")
def fresh(luts):
    """What contexts that have done nothing else return, one context per entry: the three-light call and the two-lobe call each made alone
    on the planes of the same constants, so that their scratch is allocated at its final size in one step, and the queue pool after a
    pass's renders."""
    sc, view, pos, cfg = scenes.config_cornell(luts, W, H)
    assert len(sc.lights) == 1
    cb = scenes.fill_constants(view, pos, sc, 0, cfg["max_bounces"])
    cbm = cb.copy()
    cbm["m_Jitter"] = (0.0, 0.0)
    got = {}

    def alone(call):
        ctx = native.PathTracerContext(0)
        try:
            ctx.resize(W, H)
            ctx.upload_scene(sc)
            call(ctx)
        finally:
            ctx.close()

    def three_lights(ctx):
        ctx.render_gbuffer(cbm, planes=S.GB_ALL_PLANES)
        got["deferred, three lights"] = _deferred(ctx, cbm, THREE_LIGHTS).tobytes()

    def both_lobes(ctx):
        ctx.render_gbuffer(cbm, planes=S.GB_ALL_PLANES)
        diffuse, specular = _indirect(ctx, cbm, BOTH_LOBES)
        got["indirect diffuse, both lobes"], got["indirect specular, both lobes"] = diffuse.tobytes(), specular.tobytes()

    def renders(ctx):
        # hrpt_render alone sizes the render's queue pool (csrc/pt_wavefront.hip: G-buffer, motion, ray and radiance calls use it or a pool of
        # their own and never grow it; geometry updates and hrpt_resize leave it alone), so the three renders of a pass stand for the pass
        for accum_count in (2, 1, 1):
            ctx.render(cb, accum_count=accum_count)
        got["queue pool bytes"] = int(ctx.stats().queuePoolBytes)

    for call in (three_lights, both_lobes, renders):
        alone(call)
    return got


def test_two_passes_over_one_context_give_the_same_bits(luts, fresh):
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
    assert all(any(first[name]) for name in first if name.startswith(("upscale", "probe", "deferred", "indirect")))
    assert first["deferred, three lights"] != first["deferred, one light"] and first["output with indirect"] != first["deferred, three lights"]
    # scratch that grew within a pass, and scratch left over from the pass before, give what a fresh context gives
    for name in ("deferred, three lights", "indirect diffuse, both lobes", "indirect specular, both lobes", "queue pool bytes"):
        assert first[name] == fresh[name] and second[name] == fresh[name], name
    assert fresh["queue pool bytes"] > 0
