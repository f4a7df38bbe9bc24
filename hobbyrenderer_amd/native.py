"""ctypes binding of libhobbyrt_pt.so (include/hobbyrt_pt.h). There is no fallback: if the in-tree HIP
library is missing this module raises at import, and if no GPU is present hrpt_create fails."""
import ctypes as C
import os

import numpy as np

from . import structs as S

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HRPT_LIBRARY") or os.path.join(_HERE, "libhobbyrt_pt.so")   # HRPT_LIBRARY: A/B another build of the same ABI

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build it with `make -C hobbyrenderer_amd/csrc` (or __graft_entry__.build()). "
        "The HIP library is the only backend of this package.")

# One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 / libhsa-runtime64 (soname libamdhip64.so.7)
# and RCCL is linked against it. If libhobbyrt_pt.so were loaded first it would pull /opt/rocm's copy in as a SECOND
# runtime, and whichever initialises the GPU second then finds no device. Importing torch first makes the dynamic
# loader satisfy our DT_NEEDED libamdhip64.so.7 with the already loaded copy. Without torch the ROCm copy is used.
try:
    import torch  # noqa: F401
except ImportError:  # pure-ctypes use (no multi-GPU): /opt/rocm's runtime through the library's RUNPATH
    torch = None

lib = C.CDLL(LIB_PATH)

EXPORTS = [
    "hrpt_create", "hrpt_destroy", "hrpt_last_error", "hrpt_upload_scene", "hrpt_resize", "hrpt_render",
    "hrpt_synchronize", "hrpt_set_stream", "hrpt_get_device_images", "hrpt_read_accumulation", "hrpt_read_output",
    "hrpt_write_accumulation", "hrpt_resolve_output", "hrpt_resolve_device", "hrpt_resolve_columns_device", "hrpt_get_stats", "hrpt_reset_stats", "hrpt_set_bvh_builder", "hrpt_set_acceleration_structure", "hrpt_set_shadow_overlap", "hrpt_get_build_info", "hrpt_update_instances", "hrpt_refit_instances", "hrpt_update_lights", "hrpt_update_materials", "hrpt_update_vertices", "hrpt_update_vertices_device", "hrpt_quantize_vertices_host", "hrpt_quantize_vertices_device", "hrpt_skin_vertices_host", "hrpt_skin_vertices_device", "hrpt_update_vertices_skinned", "hrpt_trace_rays", "hrpt_trace_radiance", "hrpt_allgather", "hrpt_selftest_f16_decode", "hrpt_selftest_unorm8", "hrpt_selftest_sample_textures", "hrpt_selftest_atmosphere", "hrpt_selftest_bvh", "hrpt_selftest_read_bvh", "hrpt_selftest_host_build", "hrpt_post_process", "hrpt_read_display", "hrpt_get_exposure", "hrpt_set_exposure", "hrpt_halton",
    "hrpt_bloom", "hrpt_bloom_device", "hrpt_bloom_host", "hrpt_bloom_pack_probe",
    "hrpt_render_gbuffer", "hrpt_read_gbuffer", "hrpt_get_gbuffer_device",
    "hrpt_render_motion_vectors", "hrpt_read_motion_vectors", "hrpt_get_motion_vectors_device",
    "hrpt_temporal_host", "hrpt_temporal_device", "hrpt_temporal_accumulate", "hrpt_read_temporal_history", "hrpt_get_temporal_history_device",
    "hrpt_clear_accumulation",
    "hrpt_upscale_host", "hrpt_upscale_device", "hrpt_upscale", "hrpt_read_upscaled", "hrpt_read_upscale_history", "hrpt_get_upscaled_device",
    "hrpt_post_process_device",
    "hrpt_denoise_host", "hrpt_denoise_device", "hrpt_denoise", "hrpt_set_denoise_noise",
    "hrpt_demodulate_host", "hrpt_compose_host", "hrpt_demodulate_device", "hrpt_compose_device", "hrpt_demodulate", "hrpt_compose",
    "hrpt_read_modulation", "hrpt_get_modulation_device", "hrpt_modulation_probe",
    "hrpt_precompute_atmosphere", "hrpt_precompute_atmosphere_ex", "hrpt_atmosphere_pass",
    "hrpt_animation_create", "hrpt_animation_destroy", "hrpt_animation_advance", "hrpt_animation_set_times", "hrpt_animation_get_times",
    "hrpt_animate_host", "hrpt_animate", "hrpt_get_animation_device", "hrpt_read_animation", "hrpt_animation_release",
    "hrpt_probes_create", "hrpt_probes_destroy", "hrpt_probes_update", "hrpt_probes_query", "hrpt_probes_shade_gbuffer",
    "hrpt_read_probe_irradiance", "hrpt_get_probe_irradiance_device", "hrpt_probes_read", "hrpt_probes_get_device", "hrpt_probes_write",
    "hrpt_probes_rays_host", "hrpt_probes_blend_host", "hrpt_probes_blend_device", "hrpt_probes_query_host",
    "hrpt_deferred_lighting", "hrpt_deferred_lighting_device", "hrpt_deferred_rays_host", "hrpt_deferred_shade_host",
    "hrpt_indirect_lighting", "hrpt_indirect_compose", "hrpt_read_indirect", "hrpt_get_indirect_device", "hrpt_indirect_lighting_device",
    "hrpt_indirect_compose_device", "hrpt_indirect_rays_device", "hrpt_indirect_resolve_device", "hrpt_indirect_rays_host", "hrpt_indirect_resolve_host", "hrpt_indirect_compose_host",
]

lib.hrpt_create.argtypes = [C.POINTER(S.DeviceDesc), C.POINTER(C.c_void_p)]
lib.hrpt_destroy.argtypes = [C.c_void_p]
lib.hrpt_destroy.restype = None
lib.hrpt_last_error.argtypes = [C.c_void_p]
lib.hrpt_last_error.restype = C.c_char_p
lib.hrpt_upload_scene.argtypes = [C.c_void_p, C.POINTER(S.SceneDesc)]
lib.hrpt_resize.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
lib.hrpt_render.argtypes = [C.c_void_p, C.c_void_p]
lib.hrpt_synchronize.argtypes = [C.c_void_p]
lib.hrpt_set_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
lib.hrpt_get_device_images.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
lib.hrpt_read_accumulation.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.hrpt_read_output.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.hrpt_write_accumulation.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.hrpt_resolve_output.argtypes = [C.c_void_p]
lib.hrpt_resolve_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
lib.hrpt_resolve_columns_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
lib.hrpt_get_stats.argtypes = [C.c_void_p, C.POINTER(S.Stats)]
lib.hrpt_set_bvh_builder.argtypes = [C.c_void_p, C.c_int]
lib.hrpt_set_shadow_overlap.argtypes = [C.c_void_p, C.c_int]
lib.hrpt_set_acceleration_structure.argtypes = [C.c_void_p, C.c_int]
lib.hrpt_allgather.argtypes = [C.POINTER(C.c_void_p), C.c_int]
lib.hrpt_trace_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
lib.hrpt_trace_radiance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]
lib.hrpt_get_build_info.argtypes = [C.c_void_p, C.POINTER(S.BuildInfo)]
lib.hrpt_update_instances.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
lib.hrpt_refit_instances.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
lib.hrpt_update_lights.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
lib.hrpt_update_materials.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
lib.hrpt_update_vertices.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
lib.hrpt_update_vertices_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
lib.hrpt_quantize_vertices_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int]
lib.hrpt_quantize_vertices_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
lib.hrpt_skin_vertices_host.argtypes = [C.POINTER(S.SkinArgs), C.c_void_p, C.c_int]
lib.hrpt_skin_vertices_device.argtypes = [C.c_void_p, C.POINTER(S.SkinArgs), C.c_void_p, C.c_void_p, C.c_void_p]
lib.hrpt_update_vertices_skinned.argtypes = [C.c_void_p, C.POINTER(S.SkinArgs), C.c_uint32, C.c_uint32, C.c_void_p]
lib.hrpt_animation_create.argtypes = [C.POINTER(S.AnimationDesc), C.POINTER(C.c_void_p)]
lib.hrpt_animation_destroy.argtypes = [C.c_void_p]
lib.hrpt_animation_destroy.restype = None
lib.hrpt_animation_advance.argtypes = [C.c_void_p, C.c_float]
lib.hrpt_animation_set_times.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
lib.hrpt_animation_get_times.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
lib.hrpt_animate_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
lib.hrpt_animate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
lib.hrpt_get_animation_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
lib.hrpt_read_animation.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.hrpt_animation_release.argtypes = [C.c_void_p, C.c_void_p]
lib.hrpt_reset_stats.argtypes = [C.c_void_p]
lib.hrpt_selftest_f16_decode.argtypes = [C.c_void_p, C.c_void_p]
lib.hrpt_selftest_unorm8.argtypes = [C.c_void_p, C.c_void_p]
lib.hrpt_selftest_sample_textures.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
lib.hrpt_selftest_atmosphere.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
lib.hrpt_selftest_bvh.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
lib.hrpt_selftest_read_bvh.argtypes = [C.c_void_p, C.POINTER(S.BvhDump)]
lib.hrpt_selftest_host_build.argtypes = [C.POINTER(S.SceneDesc), C.c_uint32, C.c_uint32, C.POINTER(S.BvhDump)]
lib.hrpt_post_process.argtypes = [C.c_void_p, C.POINTER(S.PostParams)]
lib.hrpt_read_display.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.hrpt_get_exposure.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_void_p]
lib.hrpt_set_exposure.argtypes = [C.c_void_p, C.c_float]
lib.hrpt_bloom.argtypes = [C.c_void_p, C.POINTER(S.BloomParams)]
lib.hrpt_bloom_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(S.BloomParams), C.c_void_p]
lib.hrpt_bloom_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(S.BloomParams), C.c_int]
lib.hrpt_bloom_pack_probe.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
lib.hrpt_render_gbuffer.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
lib.hrpt_read_gbuffer.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
lib.hrpt_get_gbuffer_device.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
lib.hrpt_render_motion_vectors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
lib.hrpt_read_motion_vectors.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.hrpt_get_motion_vectors_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
lib.hrpt_temporal_host.argtypes = [C.POINTER(S.TemporalImages), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(S.TemporalParams), C.c_int]
lib.hrpt_temporal_device.argtypes = [C.c_void_p, C.POINTER(S.TemporalImages), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(S.TemporalParams), C.c_void_p]
lib.hrpt_temporal_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(S.TemporalParams)]
lib.hrpt_read_temporal_history.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.hrpt_get_temporal_history_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
lib.hrpt_clear_accumulation.argtypes = [C.c_void_p]
lib.hrpt_upscale_host.argtypes = [C.POINTER(S.UpscaleImages), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(S.UpscaleParams), C.c_int]
lib.hrpt_upscale_device.argtypes = [C.c_void_p, C.POINTER(S.UpscaleImages), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(S.UpscaleParams), C.c_void_p]
lib.hrpt_upscale.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(S.UpscaleParams)]
lib.hrpt_read_upscaled.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.hrpt_read_upscale_history.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.hrpt_get_upscaled_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
lib.hrpt_post_process_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(S.PostParams), C.c_void_p]
lib.hrpt_denoise_host.argtypes = [C.POINTER(S.DenoiseImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.DenoiseParams), C.c_int]
lib.hrpt_denoise_device.argtypes = [C.c_void_p, C.POINTER(S.DenoiseImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.DenoiseParams), C.c_void_p]
lib.hrpt_denoise.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(S.DenoiseParams)]
lib.hrpt_set_denoise_noise.argtypes = [C.c_void_p, C.c_void_p]
lib.hrpt_demodulate_host.argtypes = [C.POINTER(S.DemodulateImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.ModulationParams), C.c_int]
lib.hrpt_compose_host.argtypes = [C.POINTER(S.ComposeImages), C.c_uint32, C.c_uint32, C.c_int]
lib.hrpt_demodulate_device.argtypes = [C.c_void_p, C.POINTER(S.DemodulateImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.ModulationParams), C.c_void_p]
lib.hrpt_compose_device.argtypes = [C.c_void_p, C.POINTER(S.ComposeImages), C.c_uint32, C.c_uint32, C.c_void_p]
lib.hrpt_demodulate.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(S.ModulationParams)]
lib.hrpt_compose.argtypes = [C.c_void_p]
lib.hrpt_read_modulation.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.hrpt_get_modulation_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
lib.hrpt_modulation_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p]
lib.hrpt_probes_create.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
lib.hrpt_probes_destroy.argtypes = [C.c_void_p]
lib.hrpt_probes_destroy.restype = None
lib.hrpt_probes_update.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
lib.hrpt_probes_query.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
lib.hrpt_probes_shade_gbuffer.argtypes = [C.c_void_p, C.c_void_p, C.c_float]
lib.hrpt_read_probe_irradiance.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.hrpt_get_probe_irradiance_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
lib.hrpt_probes_read.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
lib.hrpt_probes_get_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
lib.hrpt_probes_write.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
lib.hrpt_probes_rays_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
lib.hrpt_probes_blend_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]
lib.hrpt_probes_blend_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
lib.hrpt_probes_query_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
lib.hrpt_deferred_lighting.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(S.DeferredParams)]
lib.hrpt_deferred_lighting_device.argtypes = [C.c_void_p, C.POINTER(S.DeferredImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.DeferredParams), C.c_void_p]
lib.hrpt_deferred_rays_host.argtypes = [C.POINTER(S.DeferredImages), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
lib.hrpt_deferred_shade_host.argtypes = [C.POINTER(S.DeferredImages), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(S.DeferredParams), C.c_int]
lib.hrpt_indirect_lighting.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(S.IndirectParams)]
lib.hrpt_indirect_compose.argtypes = [C.c_void_p, C.POINTER(S.IndirectParams)]
lib.hrpt_read_indirect.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
lib.hrpt_get_indirect_device.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
lib.hrpt_indirect_lighting_device.argtypes = [C.c_void_p, C.POINTER(S.IndirectImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.IndirectParams), C.c_void_p]
lib.hrpt_indirect_compose_device.argtypes = [C.c_void_p, C.POINTER(S.IndirectImages), C.c_uint32, C.c_uint32, C.POINTER(S.IndirectParams), C.c_void_p]
lib.hrpt_indirect_rays_device.argtypes = [C.c_void_p, C.POINTER(S.IndirectImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.IndirectParams), C.c_void_p, C.c_void_p]
lib.hrpt_indirect_resolve_device.argtypes = [C.c_void_p, C.POINTER(S.IndirectImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.IndirectParams), C.c_void_p, C.c_void_p]
lib.hrpt_indirect_rays_host.argtypes = [C.POINTER(S.IndirectImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.IndirectParams), C.c_void_p, C.c_int]
lib.hrpt_indirect_resolve_host.argtypes = [C.POINTER(S.IndirectImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.IndirectParams), C.c_void_p, C.c_int]
lib.hrpt_indirect_compose_host.argtypes = [C.POINTER(S.IndirectImages), C.c_uint32, C.c_uint32, C.POINTER(S.IndirectParams), C.c_int]
lib.hrpt_halton.argtypes = [C.c_uint32, C.c_uint32]
lib.hrpt_halton.restype = C.c_float
lib.hrpt_precompute_atmosphere.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
lib.hrpt_precompute_atmosphere_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
lib.hrpt_atmosphere_pass.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32] + [C.c_void_p] * 8 + [C.c_int, C.c_int]


class HrptError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"hrpt error {code}: {message}")
        self.code = code


def _check_rc(rc):
    """A call without a context: its message is the library's process-wide one."""
    if rc != 0:
        raise HrptError(rc, lib.hrpt_last_error(None).decode())


def _ptr(a):
    return None if a is None else a.ctypes.data


_COUNT_WORDS = {2: "two", 4: "four", 5: "five"}


def _same_shape_images(name, required, **optional):
    """The image arguments of a host wrapper as contiguous float32 arrays: `required` all [H, W, 4] of one shape, each optional one None or
    of that shape. Returns (required, optional in the order given, shape)."""
    imgs = [np.ascontiguousarray(a, np.float32) for a in required]
    shape = imgs[0].shape
    if len(shape) != 3 or shape[2] != 4 or any(a.shape != shape for a in imgs):
        raise ValueError(f"{name}: {_COUNT_WORDS[len(imgs)]} float32 [H, W, 4] images of one size expected")
    opt = []
    for key, a in optional.items():
        a = None if a is None else np.ascontiguousarray(a, np.float32)
        if a is not None and a.shape != shape:
            raise ValueError(f"{name}: {key} must have the images' shape")
        opt.append(a)
    return imgs, opt, shape


def _frame_params(constants, accum_count, tile, flags, stripes):
    p = np.zeros((), S.FrameParams)
    p["stripeCount"], p["stripeIndex"] = stripes
    p["constants"] = constants
    p["accumCount"] = accum_count
    p["tileX0"], p["tileY0"], p["tileX1"], p["tileY1"] = tile
    p["flags"] = flags
    return p


ATMOSPHERE_ORDERS = 4        # scattering orders of the default tables (Bruneton's demo value; the reference's own count is unknown)


def _atmosphere_cache_path(orders):
    """Cache file of the tables for this producer source: hobbyrenderer_amd/.cache/ (git-ignored; it travels to the GPU box like the built
    libraries do). The key covers the producer and the arithmetic header, so an edit of either invalidates it."""
    import hashlib
    h = hashlib.sha1()
    for rel in (("csrc", "atmosphere_precompute.cpp"), ("..", "include", "hobbyrt", "detmath.h")):
        with open(os.path.join(_HERE, *rel), "rb") as f:
            h.update(f.read())
    return os.path.join(_HERE, ".cache", f"atmosphere_o{orders}_{h.hexdigest()[:12]}.npz")


def precompute_atmosphere(nthreads=0, orders=ATMOSPHERE_ORDERS, device=-2, cache=True):
    """Stand-ins for bin/bruneton/*.dat (src/CommonResources.cpp:519-569): float32 RGBA tables (transmittance 64 x 256, scattering
    32 x 128 x 256, irradiance 16 x 64) with `orders` scattering orders (csrc/atmosphere_precompute.cpp). device: -1 host threads, >= 0 that
    GPU, -2 the current GPU when there is one. The result does not depend on the executor (bit-identical; tests/test_atmosphere.py), so it
    is cached on disk: four orders take ~40 s on 8 host threads and ~0.1 s on the GPU."""
    path = _atmosphere_cache_path(orders) if cache else None
    if path and os.path.exists(path):
        try:
            with np.load(path) as z:
                t, s, i = z["transmittance"], z["scattering"], z["irradiance"]
            if t.shape == S.LUT_TRANSMITTANCE_SHAPE and s.shape == S.LUT_SCATTERING_SHAPE and i.shape == S.LUT_IRRADIANCE_SHAPE:
                return t, s, i
        except (OSError, ValueError, KeyError):
            pass
    t = np.zeros(S.LUT_TRANSMITTANCE_SHAPE, np.float32)
    s = np.zeros(S.LUT_SCATTERING_SHAPE, np.float32)
    i = np.zeros(S.LUT_IRRADIANCE_SHAPE, np.float32)
    rc = lib.hrpt_precompute_atmosphere_ex(t.ctypes.data, s.ctypes.data, i.ctypes.data, orders, nthreads, device)
    if rc != 0:
        raise HrptError(rc, "hrpt_precompute_atmosphere_ex")
    if path:
        try:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            tmp = f"{path}.{os.getpid()}.tmp.npz"
            np.savez(tmp, transmittance=t, scattering=s, irradiance=i)
            os.replace(tmp, path)
        except OSError:
            pass
    return t, s, i


ATM_PASS_TRANSMITTANCE, ATM_PASS_DIRECT_IRRADIANCE, ATM_PASS_SINGLE, ATM_PASS_DENSITY, ATM_PASS_INDIRECT, ATM_PASS_MULTIPLE = range(6)
_ATM_NS, _ATM_NI, _ATM_NT = 32 * 128 * 256, 16 * 64, 64 * 256


def atmosphere_pass(pass_id, order, first, count, tables, device=-1, nthreads=0):
    """hrpt_atmosphere_pass: texels [first, first + count) of one producer pass (ATM_PASS_*) from the full-size float32 tables in `tables`
    (keys T [64 * 256, 4], dIrr [16 * 64, 3], dR / dM / dDens / dMulti [32 * 128 * 256, 3], scat [32 * 128 * 256, 4]; none is modified), by
    host threads (device < 0) or on that GPU. Returns a dict of the tables the pass writes, zero outside the texels asked for unless the
    table was an input: "out" (pass 0: [64 * 256, 4]; passes 1, 4: [16 * 64, 3]; passes 3, 5: [32 * 128 * 256, 3]), "scat" (passes 2 and
    5: a copy of tables["scat"] with the texels written / accumulated), "dR" and "dM" (pass 2)."""
    shapes = {"T": (_ATM_NT, 4), "dIrr": (_ATM_NI, 3), "dR": (_ATM_NS, 3), "dM": (_ATM_NS, 3), "dDens": (_ATM_NS, 3), "dMulti": (_ATM_NS, 3), "scat": (_ATM_NS, 4)}
    written = ("scat", "dR", "dM") if pass_id == ATM_PASS_SINGLE else (("scat",) if pass_id == ATM_PASS_MULTIPLE else ())
    t = {k: (np.array(tables[k], np.float32) if k in written else np.ascontiguousarray(tables[k], np.float32)).reshape(shape) for k, shape in shapes.items()}
    out = np.zeros((_ATM_NT, 4) if pass_id == ATM_PASS_TRANSMITTANCE else ((_ATM_NI, 3) if pass_id in (ATM_PASS_DIRECT_IRRADIANCE, ATM_PASS_INDIRECT) else (_ATM_NS, 3)), np.float32)
    _check_rc(lib.hrpt_atmosphere_pass(int(pass_id), int(order), int(first), int(count), t["T"].ctypes.data, t["dIrr"].ctypes.data, t["dR"].ctypes.data, t["dM"].ctypes.data,
                                       t["dDens"].ctypes.data, t["dMulti"].ctypes.data, t["scat"].ctypes.data, out.ctypes.data, int(nthreads), int(device)))
    res = {"out": out, "scat": t["scat"]}
    if pass_id == ATM_PASS_SINGLE:
        res["dR"], res["dM"] = t["dR"], t["dM"]
    return res


def bloom_host(img, params=None, nthreads=0):
    """hrpt_bloom_host: the bloom stage (csrc/pt_bloom.h) on host threads over a float32 [H, W, 4] image; returns the composited image.
    Needs no GPU; bit-identical to PathTracerContext.bloom."""
    img = np.ascontiguousarray(img, np.float32)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError("bloom_host: float32 [H, W, 4] image expected")
    params = params if params is not None else S.BloomParams()
    out = np.empty_like(img)
    _check_rc(lib.hrpt_bloom_host(img.ctypes.data, out.ctypes.data, img.shape[1], img.shape[0], C.byref(params), int(nthreads)))
    return out


def bloom_pack_probe(rgb):
    """Test hook: (packed R11G11B10_FLOAT words, the values read back from them) for float32 [..., 3] colours."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    packed = np.empty(rgb.shape[:-1], np.uint32)
    unpacked = np.empty_like(rgb)
    _check_rc(lib.hrpt_bloom_pack_probe(rgb.ctypes.data, packed.size, packed.ctypes.data, unpacked.ctypes.data))
    return packed, unpacked


def _view_record(view):
    return np.ascontiguousarray(np.asarray(view, S.PlanarViewConstants))


def temporal_host(color, motion, depth, normal, history, view, prev_view, params=None, nthreads=0):
    """hrpt_temporal_host: the temporal stage (csrc/pt_temporal.h) on host threads over float32 [H, W, 4] images; needs no GPU and is
    bit-identical to PathTracerContext.temporal_accumulate / temporal_device. color: Output of a render; motion: read_motion_vectors();
    depth / normal: the planes S.GB_DEPTH / S.GB_NORMAL of the same frame; history: what the previous call returned, or None.
    view / prev_view: S.PlanarViewConstants of this and of last frame. view["m_ViewportSize"] must be (W, H), and
    view["m_CameraDirectionOrPosition"] must hold (camera position, 1): scenes.planar_view leaves it zero, the caller fills it.
    Returns (colour out, history out): rgb = blended radiance in both, alpha = color's alpha / the age."""
    imgs, (hist,), shape = _same_shape_images("temporal_host", (color, motion, depth, normal), history=history)
    params = params if params is not None else S.TemporalParams()
    out, hout = np.empty(shape, np.float32), np.empty(shape, np.float32)
    im = S.TemporalImages(*[a.ctypes.data for a in imgs], _ptr(hist), hout.ctypes.data, out.ctypes.data)
    v, pv = _view_record(view), _view_record(prev_view)
    _check_rc(lib.hrpt_temporal_host(C.byref(im), shape[1], shape[0], v.ctypes.data, pv.ctypes.data, C.byref(params), int(nthreads)))
    return out, hout


def upscale_host(color, depth, motion, history, display_size, view, prev_view, params=None, nthreads=0):
    """hrpt_upscale_host: the upscale stage (csrc/pt_upscale.h) on host threads; needs no GPU and is bit-identical to
    PathTracerContext.upscale / upscale_device. color / depth / motion: float32 [h, w, 4] images of one render-size frame (Output, the plane
    S.GB_DEPTH, read_motion_vectors()); history: what the previous call returned, float32 [H, W, 4], or None; display_size = (W, H) with
    w <= W <= 4 w and h <= H <= 4 h. view / prev_view: the render-size S.PlanarViewConstants of this and of last frame. params.jitter is the
    sample offset the frame was rendered with. Returns (colour out, history out) at the display size: rgb = the resolved radiance in both,
    alpha = the nearest render texel's alpha / the accumulated sample weight."""
    imgs, _, shape = _same_shape_images("upscale_host", (color, depth, motion))
    W, H = int(display_size[0]), int(display_size[1])
    hist = None if history is None else np.ascontiguousarray(history, np.float32)
    if hist is not None and hist.shape != (H, W, 4):
        raise ValueError("upscale_host: history must be a float32 [H, W, 4] image of the display size")
    params = params if params is not None else S.UpscaleParams()
    out, hout = np.empty((H, W, 4), np.float32), np.empty((H, W, 4), np.float32)
    im = S.UpscaleImages(*[a.ctypes.data for a in imgs], _ptr(hist), hout.ctypes.data, out.ctypes.data)
    v, pv = _view_record(view), _view_record(prev_view)
    _check_rc(lib.hrpt_upscale_host(C.byref(im), shape[1], shape[0], W, H, v.ctypes.data, pv.ctypes.data, C.byref(params), int(nthreads)))
    return out, hout


def denoise_host(input, depth, normal, geo_normal, view, params=None, noise=None, color=None, nthreads=0):
    """hrpt_denoise_host: ONE pass of the denoise stage (csrc/pt_denoise.h) on host threads over float32 [H, W, 4] images; needs no GPU and
    is bit-identical to PathTracerContext.denoise_device and to one pass of PathTracerContext.denoise. input: rgb = radiance, a = age (the
    history of the temporal stage); depth / normal / geo_normal: the planes S.GB_DEPTH / S.GB_NORMAL / S.GB_GEO_NORMAL of the same frame;
    noise: a float32 [64, 64, 2] tile, or None for the library's default tile (white noise); color: an image whose alpha the second
    result keeps. view: as for temporal_host. params.iterations must be 1; params.radius and params.frame are used as given.
    Returns output = (filtered rgb, age), or (output, colorOut) when color is given."""
    imgs, _, shape = _same_shape_images("denoise_host", (input, depth, normal, geo_normal))
    tile = None if noise is None else np.ascontiguousarray(noise, np.float32)
    if tile is not None and tile.shape != (64, 64, 2):
        raise ValueError("denoise_host: noise must be a float32 [64, 64, 2] tile")
    _, (col,), _ = _same_shape_images("denoise_host", imgs, color=color)      # checked after the tile, as before the helper existed
    params = params if params is not None else S.DenoiseParams()
    out = np.empty(shape, np.float32)
    cout = None if col is None else np.empty(shape, np.float32)
    im = S.DenoiseImages(*[a.ctypes.data for a in imgs], _ptr(tile), out.ctypes.data, _ptr(col), _ptr(cout))
    v = _view_record(view)
    _check_rc(lib.hrpt_denoise_host(C.byref(im), shape[1], shape[0], v.ctypes.data, C.byref(params), int(nthreads)))
    return out if cout is None else (out, cout)


def noise_tile_from_png(path):
    """A float32 [64, 64, 2] noise tile for denoise_host / PathTracerContext.set_denoise_noise from a 64 x 64 PNG, decoded through the
    library's own PNG decoder: tile[y][x] = (R / 255, G / 255), one correctly rounded binary32 division each. The reference's blue-noise
    tile is its data file external/LDR_RG01_0.png (tests/golden/blue_noise_rg_64.png is a copy)."""
    from . import scene_io
    with open(path, "rb") as f:
        rgba = scene_io.decode_image(f.read())
    if rgba.shape != (64, 64, 4):
        raise ValueError(f"noise_tile_from_png: a 64 x 64 image expected, got {rgba.shape[1]} x {rgba.shape[0]}")
    return np.ascontiguousarray(rgba[..., :2].astype(np.float32) / np.float32(255.0))


def demodulate_host(color, albedo, normal, geo_normal, depth, view, params=None, emissive=None, nthreads=0):
    """hrpt_demodulate_host: the demodulate stage (csrc/pt_modulation.h) on host threads over float32 [H, W, 4]
    images; needs no GPU and is bit-identical to PathTracerContext.demodulate / demodulate_device. color: Output of a render; albedo /
    normal / geo_normal / depth / emissive: the planes S.GB_ALBEDO / S.GB_NORMAL / S.GB_GEO_NORMAL / S.GB_DEPTH / S.GB_EMISSIVE of the same
    frame (emissive None = 0). view: as for temporal_host. Returns (colour out, modulation): colour out = (max(rgb - E, 0) / Mf, alpha),
    modulation = (Mf, 1) at a hit and (1, 1, 1, 0) at a miss."""
    imgs, (em,), shape = _same_shape_images("demodulate_host", (color, albedo, normal, geo_normal, depth), emissive=emissive)
    params = params if params is not None else S.ModulationParams()
    out, mod = np.empty(shape, np.float32), np.empty(shape, np.float32)
    im = S.DemodulateImages(*[a.ctypes.data for a in imgs], _ptr(em), out.ctypes.data, mod.ctypes.data)
    v = _view_record(view)
    _check_rc(lib.hrpt_demodulate_host(C.byref(im), shape[1], shape[0], v.ctypes.data, C.byref(params), int(nthreads)))
    return out, mod


def compose_host(color, modulation, emissive=None, nthreads=0):
    """hrpt_compose_host: the compose stage on host threads: (rgb * Mf + E, alpha) with Mf from `modulation` (what demodulate_host
    returned); a texel whose modulation alpha is 0 (a miss) passes through. Bit-identical to PathTracerContext.compose / compose_device."""
    imgs, (em,), shape = _same_shape_images("compose_host", (color, modulation), emissive=emissive)
    out = np.empty(shape, np.float32)
    im = S.ComposeImages(imgs[0].ctypes.data, imgs[1].ctypes.data, _ptr(em), out.ctypes.data)
    _check_rc(lib.hrpt_compose_host(C.byref(im), shape[1], shape[0], int(nthreads)))
    return out


def modulation_probe(albedo, normal, view_dir, rough, metal, floor=0.04):
    """Test hook (hrpt_modulation_probe): the factor Mf of one hit, float32 [3], for an albedo, a unit normal and a unit vector towards the
    camera given directly instead of reconstructed from a depth."""
    a, n, v = [np.ascontiguousarray(x, np.float32).reshape(3) for x in (albedo, normal, view_dir)]
    out = np.empty(3, np.float32)
    _check_rc(lib.hrpt_modulation_probe(a.ctypes.data, n.ctypes.data, v.ctypes.data, float(rough), float(metal), float(floor), out.ctypes.data))
    return out


def probe_volume(origin, spacing, counts, rays_per_probe, hysteresis=0.97, max_ray_distance=1e4, distance_exponent=50.0, normal_bias=0.0, view_bias=0.0):
    """An S.ProbeVolume record (HrptProbeVolume). Probe (x, y, z) sits at origin + (x, y, z) * spacing."""
    v = np.zeros((), S.ProbeVolume)
    v["origin"], v["spacing"], v["counts"], v["raysPerProbe"] = origin, spacing, counts, rays_per_probe
    v["hysteresis"], v["maxRayDistance"], v["distanceExponent"], v["normalBias"], v["viewBias"] = hysteresis, max_ray_distance, distance_exponent, normal_bias, view_bias
    return v


def _volume_record(volume):
    v = np.ascontiguousarray(np.asarray(volume, S.ProbeVolume))
    return v, int(np.prod(v["counts"], dtype=np.uint64)), int(v["raysPerProbe"].reshape(-1)[0])


def probe_points(position, normal, view):
    """S.ProbePoint records from [n, 3] positions, unit normals and unit directions to the viewer."""
    position = np.asarray(position, np.float32)
    pts = np.zeros(len(position), S.ProbePoint)
    pts["position"], pts["normal"], pts["view"] = position, normal, view
    return pts


def probes_rays_host(volume, frame_seed):
    """hrpt_probes_rays_host: the ray records (S.Ray [P * N]) and the N shared directions (float32 [N, 4]) of one update. Needs no GPU."""
    v, P, N = _volume_record(volume)
    if not (0 < P <= 1 << 20 and 0 < N <= 1024):      # the library refuses it too; this keeps the arrays below from being sized by a bad record
        raise HrptError(-1, "probes_rays_host: counts or raysPerProbe out of range")
    rays, dirs = np.zeros(P * N, S.Ray), np.zeros((N, 4), np.float32)
    _check_rc(lib.hrpt_probes_rays_host(v.ctypes.data, int(frame_seed) & 0xFFFFFFFF, rays.ctypes.data, dirs.ctypes.data))
    return rays, dirs


def probes_blend_host(volume, directions, radiance, hits, irradiance, distance, has_history, nthreads=0):
    """hrpt_probes_blend_host: the blend (csrc/pt_probes.h) on host threads; needs no GPU and is bit-identical to the kernel. directions:
    float32 [N, 4]; radiance: float32 [P * N, 4] and hits: S.RayHit [P * N] as trace_radiance / trace_rays returned them; irradiance
    [P, 8, 8, 4] and distance [P, 16, 16, 2]: the atlases before. Returns the atlases after (new arrays)."""
    v, P, N = _volume_record(volume)
    directions, radiance = np.ascontiguousarray(directions, np.float32), np.ascontiguousarray(radiance, np.float32)
    hits = np.ascontiguousarray(hits, S.RayHit)
    irr, dist = np.array(irradiance, np.float32, order="C"), np.array(distance, np.float32, order="C")
    if directions.shape != (N, 4) or radiance.shape != (P * N, 4) or hits.shape != (P * N,) or irr.shape != (P,) + S.PROBE_IRRADIANCE_SHAPE or dist.shape != (P,) + S.PROBE_DISTANCE_SHAPE:
        raise ValueError("probes_blend_host: array shapes do not match the volume")
    _check_rc(lib.hrpt_probes_blend_host(v.ctypes.data, directions.ctypes.data, radiance.ctypes.data, hits.ctypes.data, irr.ctypes.data, dist.ctypes.data,
                                         1 if has_history else 0, int(nthreads)))
    return irr, dist


def probes_query_host(volume, irradiance, distance, points, nthreads=0):
    """hrpt_probes_query_host: float32 [n, 4] = (irradiance rgb, inside) at the S.ProbePoint records `points`. Needs no GPU."""
    v, P, _ = _volume_record(volume)
    irr, dist = np.ascontiguousarray(irradiance, np.float32), np.ascontiguousarray(distance, np.float32)
    if irr.shape != (P,) + S.PROBE_IRRADIANCE_SHAPE or dist.shape != (P,) + S.PROBE_DISTANCE_SHAPE:
        raise ValueError("probes_query_host: atlas shapes do not match the volume")
    points = np.ascontiguousarray(points, S.ProbePoint)
    out = np.zeros((len(points), 4), np.float32)
    _check_rc(lib.hrpt_probes_query_host(v.ctypes.data, irr.ctypes.data, dist.ctypes.data, points.ctypes.data, out.ctypes.data, len(points), int(nthreads)))
    return out


def _indirect_lobes(params):
    return int(bool(params.flags & S.INDIRECT_DIFFUSE)) + int(bool(params.flags & S.INDIRECT_SPECULAR))


def indirect_rays_host(albedo, normal, geo_normal, depth, constants, params=None, nthreads=0):
    """hrpt_indirect_rays_host: the ray records (S.Ray [lobes, H, W], diffuse first) of every pixel of the four float32 [H, W, 4] planes
    rendered with `constants` (csrc/pt_indirect.h). An untraced record has a NaN origin and zeros elsewhere. Needs no
    GPU; bit-identical to the kernel."""
    imgs, _, shape = _same_shape_images("indirect_rays_host", (albedo, normal, geo_normal, depth))
    params = params if params is not None else S.IndirectParams()
    cb = np.ascontiguousarray(constants, S.PathTracerConstants)
    out = np.zeros((max(_indirect_lobes(params), 1), shape[0], shape[1]), S.Ray)
    im = S.IndirectImages(*[a.ctypes.data for a in imgs], None, None, None)
    _check_rc(lib.hrpt_indirect_rays_host(C.byref(im), shape[1], shape[0], cb.ctypes.data, C.byref(params), out.ctypes.data, int(nthreads)))
    return out


def indirect_resolve_host(albedo, normal, geo_normal, depth, constants, radiance, params=None, nthreads=0):
    """hrpt_indirect_resolve_host: (diffuse, specular) float32 [H, W, 4] from the radiance of the records (float32 [lobes, H, W, 4], the layout
    of indirect_rays_host); the plane of a lobe that is not flagged comes back as zeros."""
    imgs, _, shape = _same_shape_images("indirect_resolve_host", (albedo, normal, geo_normal, depth))
    params = params if params is not None else S.IndirectParams()
    rad = np.ascontiguousarray(radiance, np.float32)
    if rad.shape != (max(_indirect_lobes(params), 1),) + shape:
        raise ValueError("indirect_resolve_host: radiance must be [lobes, H, W, 4]")
    cb = np.ascontiguousarray(constants, S.PathTracerConstants)
    dif, spec = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    im = S.IndirectImages(*[a.ctypes.data for a in imgs], dif.ctypes.data, spec.ctypes.data, None)
    _check_rc(lib.hrpt_indirect_resolve_host(C.byref(im), shape[1], shape[0], cb.ctypes.data, C.byref(params), rad.ctypes.data, int(nthreads)))
    return dif, spec


def indirect_compose_host(color, albedo, geo_normal, depth, diffuse, specular, params=None, nthreads=0):
    """hrpt_indirect_compose_host: color + (diffuse * albedo * (1 - metallic) + specular) * intensity at hits, float32 [H, W, 4] (a new array)."""
    imgs, _, shape = _same_shape_images("indirect_compose_host", (color, albedo, geo_normal, depth, diffuse))
    (spec,), _, sshape = _same_shape_images("indirect_compose_host", (specular,))
    if sshape != shape:
        raise ValueError("indirect_compose_host: specular must have the images' shape")
    params = params if params is not None else S.IndirectParams()
    out = imgs[0].copy()
    im = S.IndirectImages(imgs[1].ctypes.data, None, imgs[2].ctypes.data, imgs[3].ctypes.data, imgs[4].ctypes.data, spec.ctypes.data, out.ctypes.data)
    _check_rc(lib.hrpt_indirect_compose_host(C.byref(im), shape[1], shape[0], C.byref(params), int(nthreads)))
    return out


def deferred_rays_host(depth, normal, constants, lights, first_light=0, light_count=None):
    """hrpt_deferred_rays_host: the shadow-ray records (S.Ray [light_count, H, W]) of lights[first_light : first_light + light_count] at every
    pixel of the float32 [H, W, 4] planes S.GB_DEPTH / S.GB_NORMAL rendered with `constants` (csrc/pt_deferred.h). A lit
    pair: origin X, direction L, tmax = the distance to the light; an unlit pair or a miss: origin NaN, the rest 0. Needs no GPU."""
    (depth, normal), _, shape = _same_shape_images("deferred_rays_host", (depth, normal))
    lights = np.ascontiguousarray(lights, S.GPULight).reshape(-1)
    light_count = len(lights) - first_light if light_count is None else int(light_count)
    if first_light < 0 or light_count < 0 or first_light + light_count > len(lights):
        raise ValueError("deferred_rays_host: light range outside the list")
    rays = np.zeros((light_count, shape[0], shape[1]), S.Ray)
    im = S.DeferredImages(None, normal.ctypes.data, None, None, depth.ctypes.data, None, None)
    cb = np.ascontiguousarray(constants)
    _check_rc(lib.hrpt_deferred_rays_host(C.byref(im), shape[1], shape[0], cb.ctypes.data, lights.ctypes.data if len(lights) else None, int(first_light), light_count,
                                          rays.ctypes.data if light_count else None))
    return rays


def deferred_shade_host(albedo, normal, geo_normal, emissive, depth, constants, lights, visibility=None, sun_radiance=None, sky=None, indirect=None,
                        params=None, nthreads=0):
    """hrpt_deferred_shade_host: the lit image, float32 [H, W, 4], of all `lights` over the five float32 [H, W, 4] planes; needs no GPU and is
    bit-identical to PathTracerContext.deferred_lighting / deferred_lighting_device given the same visibilities and atmosphere terms.
    visibility: float32 [len(lights), H, W] (None = 1); sun_radiance: [H, W, 4], the radiance of a directional light at each first hit (None =
    colour x intensity); sky: [H, W, 4] stored at misses (None = zeros); indirect: [H, W, 4], read with S.DEFERRED_INDIRECT in params.flags."""
    imgs, (sun, sk, ind), shape = _same_shape_images("deferred_shade_host", (albedo, normal, geo_normal, emissive, depth), sun_radiance=sun_radiance, sky=sky, indirect=indirect)
    lights = np.ascontiguousarray(lights, S.GPULight).reshape(-1)
    vis = None if visibility is None else np.ascontiguousarray(visibility, np.float32)
    if vis is not None and vis.shape != (len(lights), shape[0], shape[1]):
        raise ValueError("deferred_shade_host: visibility must be [lights, H, W]")
    params = params if params is not None else S.DeferredParams()
    out = np.empty(shape, np.float32)
    im = S.DeferredImages(*[a.ctypes.data for a in imgs], _ptr(ind), out.ctypes.data)
    cb = np.ascontiguousarray(constants)
    _check_rc(lib.hrpt_deferred_shade_host(C.byref(im), shape[1], shape[0], cb.ctypes.data, lights.ctypes.data if len(lights) else None, len(lights), _ptr(vis), _ptr(sun),
                                           _ptr(sk), C.byref(params), int(nthreads)))
    return out


class ProbeVolume:
    """HrptProbes: an irradiance probe volume on one PathTracerContext (hrpt_probes_*). Close it before its context."""

    def __init__(self, context, volume):
        self._ctx = context
        self.volume, self.probe_count, self.rays_per_probe = _volume_record(volume)
        self._h = C.c_void_p()
        context._check(lib.hrpt_probes_create(context._h, self.volume.ctypes.data, C.byref(self._h)))

    def close(self):
        if self._h:
            lib.hrpt_probes_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, constants, frame_seed, reset=False):
        """hrpt_probes_update: rays for frame_seed, trace_radiance + trace_rays, blend. Asynchronous on the context stream."""
        cb = np.ascontiguousarray(constants, S.PathTracerConstants)
        self._ctx._check(lib.hrpt_probes_update(self._h, cb.ctypes.data, int(frame_seed) & 0xFFFFFFFF, S.PROBES_RESET if reset else 0))

    def query(self, points):
        """hrpt_probes_query over host records (S.ProbePoint): float32 [n, 4] = (irradiance rgb, inside). Synchronises."""
        points = np.ascontiguousarray(points, S.ProbePoint)
        out = np.zeros((len(points), 4), np.float32)
        self._ctx._check(lib.hrpt_probes_query(self._h, points.ctypes.data, out.ctypes.data, len(points), 0))
        return out

    def query_device(self, points_ptr, out_ptr, count):
        """hrpt_probes_query over device arrays (integer addresses of `count` S.ProbePoint records and float4 slots). Asynchronous."""
        self._ctx._check(lib.hrpt_probes_query(self._h, C.c_void_p(int(points_ptr)), C.c_void_p(int(out_ptr)), int(count), S.PROBES_DEVICE_POINTERS))

    def shade_gbuffer(self, view, intensity=1.0):
        """hrpt_probes_shade_gbuffer: the query at every first hit (planes S.GB_NORMAL and S.GB_DEPTH) into the context's probe irradiance plane."""
        self._ctx._check(lib.hrpt_probes_shade_gbuffer(self._h, _view_record(view).ctypes.data, float(intensity)))

    def read(self):
        """(irradiance [P, 8, 8, 4], distance [P, 16, 16, 2]); synchronises."""
        irr = np.empty((self.probe_count,) + S.PROBE_IRRADIANCE_SHAPE, np.float32)
        dist = np.empty((self.probe_count,) + S.PROBE_DISTANCE_SHAPE, np.float32)
        self._ctx._check(lib.hrpt_probes_read(self._h, irr.ctypes.data, irr.nbytes, dist.ctypes.data, dist.nbytes))
        return irr, dist

    def write(self, irradiance=None, distance=None):
        """hrpt_probes_write: installs atlases (None = leave that one); they are the history of the next update."""
        irr = None if irradiance is None else np.ascontiguousarray(irradiance, np.float32)
        dist = None if distance is None else np.ascontiguousarray(distance, np.float32)
        self._ctx._check(lib.hrpt_probes_write(self._h, _ptr(irr), 0 if irr is None else irr.nbytes, _ptr(dist), 0 if dist is None else dist.nbytes))

    def device(self):
        """Device pointers (irradiance, distance) of the atlases."""
        a, b = C.c_void_p(), C.c_void_p()
        self._ctx._check(lib.hrpt_probes_get_device(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value


def quantize_vertices_host(vertices, nthreads=0):
    """hrpt_quantize_vertices_host: S.VertexFloat records -> S.VertexQuantized records by the library's quantiser (csrc/pt_deform.h) on host
    threads; needs no GPU and is bit-identical to PathTracerContext.quantize_vertices_device and to scenes.quantize_vertices."""
    v = np.ascontiguousarray(vertices, S.VertexFloat)
    out = np.zeros(len(v), S.VertexQuantized)
    _check_rc(lib.hrpt_quantize_vertices_host(v.ctypes.data if len(v) else None, len(v), out.ctypes.data if len(v) else None, int(nthreads)))
    return out


def animation_desc(samplers=(), channels=(), nodes=(), joints=(), key_times=(), key_values=(), targets=(), node_instances=(), animation_count=0,
                   morph_weight_count=0, reserved=0):
    """The tables of an animation as contiguous arrays in the library's layouts and the S.AnimationDesc over them: (desc, arrays). The
    arrays must outlive the desc. samplers S.AnimSampler, channels S.AnimChannel, nodes S.AnimNode, joints S.AnimJoint, key_times float32
    [keys], key_values float32 [keys, 4], targets and node_instances uint32."""
    records = lambda a, dtype: np.ascontiguousarray(a, dtype) if len(a) else np.zeros(0, dtype)      # noqa: E731
    arrays = [records(samplers, S.AnimSampler), records(channels, S.AnimChannel), records(nodes, S.AnimNode),
              records(joints, S.AnimJoint), np.ascontiguousarray(key_times, np.float32).reshape(-1),
              np.ascontiguousarray(key_values, np.float32).reshape(-1, 4), np.ascontiguousarray(targets, np.uint32).reshape(-1),
              np.ascontiguousarray(node_instances, np.uint32).reshape(-1)]
    if len(arrays[5]) != len(arrays[4]):
        raise ValueError("animation_desc: one float4 value per key time expected")
    counts = [len(arrays[k]) for k in (0, 1, 2, 3, 4, 6, 7)]
    desc = S.AnimationDesc(*[a.ctypes.data if a.size else None for a in arrays], *counts, int(animation_count), int(morph_weight_count), int(reserved))
    return desc, arrays


class Animation:
    """hrpt_animation_create: validated, resolved copy of animation tables (animation_desc's keywords); context-free. times / durations,
    advance(dt) and set_times are the host clock; evaluate_host runs csrc/pt_anim.h on host threads; PathTracerContext.animate runs it on
    the device."""

    def __init__(self, **tables):
        desc, arrays = animation_desc(**tables)
        self._h = C.c_void_p()
        _check_rc(lib.hrpt_animation_create(C.byref(desc), C.byref(self._h)))
        self.animation_count, self.node_count = desc.animationCount, desc.nodeCount
        self.joint_count, self.morph_weight_count = desc.jointCount, desc.morphWeightCount

    def close(self):
        if self._h:
            lib.hrpt_animation_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def advance(self, dt):
        _check_rc(lib.hrpt_animation_advance(self._h, float(dt)))

    def set_times(self, times):
        times = np.ascontiguousarray(times, np.float32).reshape(-1)
        _check_rc(lib.hrpt_animation_set_times(self._h, times.ctypes.data if times.size else None, len(times)))

    def _clock(self, which):
        out = np.zeros(self.animation_count, np.float32)
        args = [None, None]
        args[which] = out.ctypes.data
        _check_rc(lib.hrpt_animation_get_times(self._h, *args, self.animation_count))
        return out

    @property
    def times(self):
        return self._clock(0)

    @property
    def durations(self):
        return self._clock(1)

    def evaluate_host(self, instances=None, nthreads=0):
        """hrpt_animate_host at the current times: (instances, palette [joints, 3, 4], weights, node worlds [nodes, 4, 4]). `instances`
        (S.PerInstanceData records of the whole scene, or None) is not modified: the first result is the rolled and moved copy."""
        out = None if instances is None else np.array(instances, S.PerInstanceData, copy=True, order="C")
        palette = np.zeros((self.joint_count, 3, 4), np.float32)
        weights = np.zeros(self.morph_weight_count, np.float32)
        worlds = np.zeros((self.node_count, 4, 4), np.float32)
        _check_rc(lib.hrpt_animate_host(self._h, None, None if out is None else out.ctypes.data, 0 if out is None else len(out),
                                        palette.ctypes.data, weights.ctypes.data, worlds.ctypes.data, int(nthreads)))
        return out, palette, weights, worlds


def skin_arrays(base, joints=None, weights=None, joint_matrices=None, deltas=None, morph_weights=None):
    """The arrays of an S.SkinArgs in the layout the library reads: base S.VertexFloat [count]; joints uint16 [count, 4], weights float32
    [count, 4] and joint_matrices float32 [jointCount, 3, 4] (or all three None); deltas S.SkinMorphDelta [targetCount, count] and
    morph_weights float32 [targetCount] (or both None). Returns (arrays, count, jointCount, targetCount); what was given as None stays None."""
    base = np.ascontiguousarray(base, S.VertexFloat)
    n = len(base)
    if joints is not None:
        joints = np.ascontiguousarray(joints, np.uint16).reshape(n, 4)
        weights = np.ascontiguousarray(weights, np.float32).reshape(n, 4)
        joint_matrices = np.ascontiguousarray(joint_matrices, np.float32).reshape(-1, 3, 4)
    if deltas is not None:
        morph_weights = np.ascontiguousarray(morph_weights, np.float32).reshape(-1)
        deltas = np.ascontiguousarray(deltas, S.SkinMorphDelta).reshape(len(morph_weights), n)
    arrays = (base, joints, weights, joint_matrices, deltas, morph_weights)
    return arrays, n, 0 if joints is None else len(joint_matrices), 0 if deltas is None else len(morph_weights)


def _aligned_copy(a, align=16):
    """A copy of array `a` whose first byte lies on a multiple of `align` (NumPy promises no more than the item's own alignment)."""
    raw = np.empty(a.nbytes + align, np.uint8)
    start = -raw.ctypes.data % align
    out = raw[start:start + a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


def skin_vertices_host(base, joints=None, weights=None, joint_matrices=None, deltas=None, morph_weights=None, nthreads=0):
    """hrpt_skin_vertices_host: morph targets, then four-joint skinning, then unit normal and tangent (csrc/pt_skin.h) of the bind pose
    `base` (S.VertexFloat records) on host threads; the arrays are those of skin_arrays(). Returns S.VertexFloat records. Needs no GPU and
    is bit-identical to PathTracerContext.skin_vertices_device and to tests/skin_reference.py. A joint index out of range raises."""
    arrays, n, joint_count, target_count = skin_arrays(base, joints, weights, joint_matrices, deltas, morph_weights)
    arrays = [None if a is None else _aligned_copy(a) for a in arrays]
    out = _aligned_copy(np.zeros(n, S.VertexFloat))
    args = S.SkinArgs(*[None if a is None or not a.size else a.ctypes.data for a in arrays], n, joint_count, target_count, 0)
    _check_rc(lib.hrpt_skin_vertices_host(C.byref(args), out.ctypes.data if n else None, int(nthreads)))
    return out


_BVH_DUMP_ARRAYS = (("nodes", S.GpuNode, "nodeCount"), ("nodes4", S.GpuNode4, "node4Count"), ("nodesQ", S.GpuNodeQ, "node4Count"),
                    ("triangles", S.GpuTri, "triangleCount"), ("attributes", S.GpuTriAttr, "triangleCount"),
                    ("tangents", S.GpuTriTangent, "triangleCount"), ("instances", S.GpuInstance, "instanceCount"))


def _read_bvh_dump(call):
    """Size query, then fill (HrptBvhDump): returns a dict of the header fields and one structured numpy array per record array
    (None where the structure has none)."""
    d = S.BvhDump()
    call(d)
    present = {"nodesQ": d.hasNodesQ, "tangents": d.hasTangents}
    arrays = {}
    for name, dtype, count in _BVH_DUMP_ARRAYS:
        if present.get(name, 1):
            arrays[name] = np.zeros(getattr(d, count), dtype)
            setattr(d, name, arrays[name].ctypes.data if arrays[name].size else None)
        else:
            arrays[name] = None
    counts = [getattr(d, c) for _, _, c in _BVH_DUMP_ARRAYS]
    call(d)
    assert counts == [getattr(d, c) for _, _, c in _BVH_DUMP_ARRAYS], "the structure changed between the size query and the fill"
    out = {f: getattr(d, f) for f, _ in S.BvhDump._fields_ if f not in arrays}
    out.update(arrays)
    return out


def host_build_bvh(scene, structure=S.ACCEL_FLAT, separate_collapse=False):
    """hrpt_selftest_host_build: the host builder's structure for a SceneArrays, without a context or a device (see _read_bvh_dump)."""
    desc, keep = scene.desc()

    def call(d):
        _check_rc(lib.hrpt_selftest_host_build(C.byref(desc), int(structure), S.HOST_BUILD_SEPARATE_COLLAPSE if separate_collapse else 0, C.byref(d)))
    out = _read_bvh_dump(call)
    del keep
    return out


def allgather(contexts):
    """hrpt_allgather over PathTracerContext objects living in this process (one per GPU, or several on one GPU)."""
    arr = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
    rc = lib.hrpt_allgather(arr, len(contexts))
    if rc != 0:
        raise HrptError(rc, lib.hrpt_last_error(contexts[0]._h).decode() if contexts else "hrpt_allgather")


class PathTracerContext:
    """One context = one GPU = one stream (include/hobbyrt_pt.h)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        desc = S.DeviceDesc(device, S.ABI_VERSION)
        _check_rc(lib.hrpt_create(C.byref(desc), C.byref(self._h)))
        self.width = self.height = 0

    def _check(self, rc):
        if rc != 0:
            raise HrptError(rc, lib.hrpt_last_error(self._h).decode())

    def _read_image(self, fn, dtype=np.float32, args=()):
        """A context image of the current size, [H, W, 4], through one of the library's readers (synchronises)."""
        out = np.empty((self.height, self.width, 4), dtype)
        self._check(fn(self._h, *args, out.ctypes.data, out.nbytes))
        return out

    def _device_ptr(self, fn, args=()):
        ptr = C.c_void_p()
        self._check(fn(self._h, *args, C.byref(ptr)))
        return ptr.value

    def close(self):
        if self._h:
            lib.hrpt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_scene(self, scene):
        d, keep = scene.desc()
        self._check(lib.hrpt_upload_scene(self._h, C.byref(d)))
        del keep

    def resize(self, width, height):
        self._check(lib.hrpt_resize(self._h, width, height))
        self.width, self.height = width, height

    def render(self, constants, accum_count=1, tile=(0, 0, 0, 0), flags=S.FRAME_DEFAULT, stripes=(1, 0)):
        """stripes = (count, index): of the tile's 8-pixel columns only those with column % count == index are rendered."""
        p = _frame_params(constants, accum_count, tile, flags, stripes)
        self._check(lib.hrpt_render(self._h, p.ctypes.data))

    def render_gbuffer(self, constants, planes=S.GB_ALL_PLANES, tile=(0, 0, 0, 0), flags=S.FRAME_DEFAULT, stripes=(1, 0)):
        """hrpt_render_gbuffer: what the primary rays of one accumulation index saw (path vertex 0), into the planes of the bit mask `planes`
        (1 << S.GB_ALBEDO ...). constants.m_Jitter is used as given; tile / flags / stripes as in render. Asynchronous."""
        p = _frame_params(constants, 1, tile, flags, stripes)
        self._check(lib.hrpt_render_gbuffer(self._h, p.ctypes.data, int(planes)))

    def read_gbuffer(self, plane):
        """One G-buffer plane: float32 [H, W, 4], or uint32 [H, W, 4] for S.GB_IDS (synchronises)."""
        return self._read_image(lib.hrpt_read_gbuffer, np.uint32 if plane == S.GB_IDS else np.float32, (int(plane),))

    def gbuffer_device(self, plane):
        """Device pointer of one G-buffer plane (None when it was never requested)."""
        return self._device_ptr(lib.hrpt_get_gbuffer_device, (int(plane),))

    def render_motion_vectors(self, constants, prev_view, planes=0, tile=(0, 0, 0, 0), flags=S.FRAME_DEFAULT, stripes=(1, 0)):
        """hrpt_render_motion_vectors: screen-space motion of the first hit (previous minus current window position in pixels, change of view
        depth, valid flag) for constants["m_View"] against last frame's `prev_view` (S.PlanarViewConstants) and the instances' m_PrevWorld.
        `planes`: G-buffer planes to write in the same pass (0 = motion only). tile / flags / stripes as in render_gbuffer. Asynchronous."""
        p = _frame_params(constants, 1, tile, flags, stripes)
        pv = np.ascontiguousarray(np.asarray(prev_view, S.PlanarViewConstants))
        self._check(lib.hrpt_render_motion_vectors(self._h, p.ctypes.data, pv.ctypes.data, int(planes)))

    def read_motion_vectors(self):
        """The motion plane: float32 [H, W, 4] (synchronises)."""
        return self._read_image(lib.hrpt_read_motion_vectors)

    def motion_vectors_device(self):
        """Device pointer of the motion plane (None before the first render_motion_vectors)."""
        return self._device_ptr(lib.hrpt_get_motion_vectors_device)

    def set_stream(self, hip_stream):
        """hip_stream: integer handle (e.g. torch.cuda.current_stream().cuda_stream; 0 = the default stream), or None to go
        back to the context's own stream."""
        if hip_stream is None:
            self._check(lib.hrpt_set_stream(self._h, None, 0))
        else:
            self._check(lib.hrpt_set_stream(self._h, C.c_void_p(int(hip_stream)), 1))

    def synchronize(self):
        self._check(lib.hrpt_synchronize(self._h))

    def device_images(self):
        a, o = C.c_void_p(), C.c_void_p()
        self._check(lib.hrpt_get_device_images(self._h, C.byref(a), C.byref(o)))
        return a.value, o.value

    def read_accumulation(self):
        return self._read_image(lib.hrpt_read_accumulation)

    def read_output(self):
        return self._read_image(lib.hrpt_read_output)

    def write_accumulation(self, img):
        img = np.ascontiguousarray(img, np.float32)
        self._check(lib.hrpt_write_accumulation(self._h, img.ctypes.data, img.nbytes))

    def resolve_output(self):
        self._check(lib.hrpt_resolve_output(self._h))

    def resolve_device(self, accumulation_ptr, output_ptr, pixel_count, hip_stream=0):
        """Output = accum.rgb / accum.a over caller-owned device images, asynchronously on `hip_stream` (integer handle)."""
        self._check(lib.hrpt_resolve_device(self._h, C.c_void_p(int(accumulation_ptr)), C.c_void_p(int(output_ptr)), int(pixel_count),
                                            C.c_void_p(int(hip_stream))))

    def resolve_columns_device(self, shards_ptr, accumulation_ptr, output_ptr, width, height, ranks, hip_stream=0):
        """Rank-major column shards -> Output (= rgb / a, image order) and, unless accumulation_ptr is 0/None, the assembled accumulation image."""
        self._check(lib.hrpt_resolve_columns_device(self._h, C.c_void_p(int(shards_ptr)), C.c_void_p(int(accumulation_ptr or 0)) if accumulation_ptr else None,
                                                    C.c_void_p(int(output_ptr)), int(width), int(height), int(ranks), C.c_void_p(int(hip_stream))))

    def trace_rays(self, rays, shadow=False, thread_per_ray=False):
        """rays: structured array of S.Ray; returns a structured array of S.RayHit (see hrpt_trace_rays). thread_per_ray: the
        one-thread-per-ray cross-check kernel instead of the persistent refilling traversal kernel."""
        rays = np.ascontiguousarray(rays, S.Ray)
        hits = np.zeros(len(rays), S.RayHit)
        flags = (S.RAYS_SHADOW if shadow else S.RAYS_CLOSEST) | (S.RAYS_THREAD_PER_RAY if thread_per_ray else 0)
        self._check(lib.hrpt_trace_rays(self._h, rays.ctypes.data, hits.ctypes.data, len(rays), flags))
        return hits

    def trace_radiance(self, rays, constants, accumulate=False, thread_per_ray=False, out=None, secondary=False):
        """hrpt_trace_radiance: the path-traced radiance along each of `rays` (structured array of S.Ray: origin, unit direction, tmin and RNG
        state; tmax is ignored), float32 [n, 4] = (L.rgb, 1). Of `constants` (S.PathTracerConstants) the sun, m_LightCount and m_MaxBounces
        are read. accumulate: add (L, 1) to `out` (float32 [n, 4], required then) instead; out: the array to write, returned.
        thread_per_ray: the one-thread-per-ray cross-check kernel instead of the wavefront pipeline. secondary (S.RADIANCE_SECONDARY): the rays
        are path segment 1 -- they leave a first hit that is lit elsewhere -- so the bounce loop starts at index 1. Synchronises."""
        rays = np.ascontiguousarray(rays, S.Ray)
        if out is None:
            if accumulate:
                raise ValueError("trace_radiance: accumulate needs the array to add to (out)")
            out = np.zeros((len(rays), 4), np.float32)
        if out.dtype != np.float32 or out.shape != (len(rays), 4) or not out.flags.c_contiguous:
            raise ValueError("trace_radiance: out must be a contiguous float32 [len(rays), 4] array")
        cb = np.ascontiguousarray(constants, S.PathTracerConstants)
        flags = (S.RADIANCE_ACCUMULATE if accumulate else 0) | (S.RADIANCE_THREAD_PER_RAY if thread_per_ray else 0) | (S.RADIANCE_SECONDARY if secondary else 0)
        self._check(lib.hrpt_trace_radiance(self._h, rays.ctypes.data, out.ctypes.data, len(rays), cb.ctypes.data, flags))
        return out

    def trace_rays_device(self, rays_ptr, hits_ptr, count, flags=0):
        """hrpt_trace_rays over device arrays (integer addresses of `count` S.Ray and S.RayHit records). Asynchronous on the context stream."""
        self._check(lib.hrpt_trace_rays(self._h, C.c_void_p(int(rays_ptr)), C.c_void_p(int(hits_ptr)), int(count), int(flags) | S.RAYS_DEVICE_POINTERS))

    def probes_blend_device(self, volume, directions_ptr, radiance_ptr, hits_ptr, irradiance_ptr, distance_ptr, has_history, hip_stream=0):
        """hrpt_probes_blend_device: the blend kernel over caller-owned device arrays, asynchronous on `hip_stream`."""
        v, _, _ = _volume_record(volume)
        self._check(lib.hrpt_probes_blend_device(self._h, v.ctypes.data, *[C.c_void_p(int(p)) for p in (directions_ptr, radiance_ptr, hits_ptr, irradiance_ptr, distance_ptr)],
                                                 1 if has_history else 0, C.c_void_p(int(hip_stream))))

    def read_probe_irradiance(self):
        """The plane ProbeVolume.shade_gbuffer wrote: float32 [H, W, 4] (synchronises)."""
        return self._read_image(lib.hrpt_read_probe_irradiance)

    def probe_irradiance_device(self):
        """Device pointer of that plane (None before the first shade_gbuffer and after a resize)."""
        return self._device_ptr(lib.hrpt_get_probe_irradiance_device)

    def trace_radiance_device(self, rays_ptr, out_ptr, count, constants, flags=0):
        """hrpt_trace_radiance over device arrays (integer addresses of `count` S.Ray records and `count` float4 slots, e.g. a torch tensor's
        data_ptr()): no copies, asynchronous on the context stream. flags: S.RADIANCE_ACCUMULATE / S.RADIANCE_THREAD_PER_RAY / S.RADIANCE_SECONDARY."""
        cb = np.ascontiguousarray(constants, S.PathTracerConstants)
        self._check(lib.hrpt_trace_radiance(self._h, C.c_void_p(int(rays_ptr)), C.c_void_p(int(out_ptr)), int(count), cb.ctypes.data,
                                            int(flags) | S.RADIANCE_DEVICE_POINTERS))

    def indirect_lighting(self, constants, params=None):
        """hrpt_indirect_lighting: one traced diffuse and one traced specular ray per first hit, from the planes S.GB_ALBEDO, GB_NORMAL,
        GB_GEO_NORMAL and GB_DEPTH that render_gbuffer wrote with the same `constants`, into two library-owned planes (read_indirect). Output
        and Accumulation are not touched (csrc/pt_indirect.h). Default params: both lobes, seed 0. Asynchronous."""
        params = params if params is not None else S.IndirectParams()
        cb = np.ascontiguousarray(constants, S.PathTracerConstants)
        self._check(lib.hrpt_indirect_lighting(self._h, cb.ctypes.data, C.byref(params)))

    def indirect_compose(self, params=None):
        """hrpt_indirect_compose: Output += (diffuse * albedo * (1 - metallic) + specular) * params.intensity at hits."""
        params = params if params is not None else S.IndirectParams()
        self._check(lib.hrpt_indirect_compose(self._h, C.byref(params)))

    def read_indirect(self, which):
        """One of the planes indirect_lighting wrote (0 = diffuse, 1 = specular): float32 [H, W, 4] (synchronises)."""
        return self._read_image(lib.hrpt_read_indirect, args=(int(which),))

    def indirect_device(self, which):
        """Device pointer of that plane (None before the first indirect_lighting and after a resize)."""
        return self._device_ptr(lib.hrpt_get_indirect_device, (int(which),))

    def indirect_lighting_device(self, images, width, height, constants, params=None, hip_stream=0):
        """The same over caller-owned device images (S.IndirectImages of device addresses), with this context's scene, on `hip_stream`."""
        params = params if params is not None else S.IndirectParams()
        cb = np.ascontiguousarray(constants, S.PathTracerConstants)
        self._check(lib.hrpt_indirect_lighting_device(self._h, C.byref(images), int(width), int(height), cb.ctypes.data, C.byref(params), C.c_void_p(int(hip_stream))))

    def indirect_rays_device(self, images, width, height, constants, rays_ptr, params=None, hip_stream=0):
        """hrpt_indirect_rays_device: the ray-record kernel alone, into a device array of width * height S.Ray per flagged lobe."""
        params = params if params is not None else S.IndirectParams()
        cb = np.ascontiguousarray(constants, S.PathTracerConstants)
        self._check(lib.hrpt_indirect_rays_device(self._h, C.byref(images), int(width), int(height), cb.ctypes.data, C.byref(params), C.c_void_p(int(rays_ptr)),
                                                  C.c_void_p(int(hip_stream))))

    def indirect_resolve_device(self, images, width, height, constants, radiance_ptr, params=None, hip_stream=0):
        """hrpt_indirect_resolve_device: the resolve kernel alone, from a device array of one float4 per record into images.diffuse / specular."""
        params = params if params is not None else S.IndirectParams()
        cb = np.ascontiguousarray(constants, S.PathTracerConstants)
        self._check(lib.hrpt_indirect_resolve_device(self._h, C.byref(images), int(width), int(height), cb.ctypes.data, C.byref(params), C.c_void_p(int(radiance_ptr)),
                                                     C.c_void_p(int(hip_stream))))

    def indirect_compose_device(self, images, width, height, params=None, hip_stream=0):
        """hrpt_indirect_compose_device: images.colorInOut += the composed images.diffuse / images.specular, on `hip_stream`."""
        params = params if params is not None else S.IndirectParams()
        self._check(lib.hrpt_indirect_compose_device(self._h, C.byref(images), int(width), int(height), C.byref(params), C.c_void_p(int(hip_stream))))

    def set_shadow_overlap(self, enabled):
        """Intra-frame overlap of the shadow stage with the next bounce's traversal (default on); turn off for contexts used as lanes of
        a two-frames-in-flight loop."""
        self._check(lib.hrpt_set_shadow_overlap(self._h, 1 if enabled else 0))

    def set_bvh_builder(self, builder):
        """S.BVH_BUILDER_AUTO (default: host SAH below 65 536 triangles, GPU PLOC above), _HOST_SAH, _GPU_LBVH or _GPU_PLOC; used by the next upload_scene / update_instances."""
        self._check(lib.hrpt_set_bvh_builder(self._h, int(builder)))

    def set_acceleration_structure(self, structure):
        """S.ACCEL_AUTO (default), S.ACCEL_FLAT (one world-space tree) or S.ACCEL_TWO_LEVEL (a tree per distinct mesh + a tree over the instances;
        opaque and non-opaque instances alike; a scene with a singular instance matrix is built flat -- build_info().structure tells); used by the next upload_scene."""
        self._check(lib.hrpt_set_acceleration_structure(self._h, int(structure)))

    def update_instances(self, instances, first=0):
        """New transforms for the instances [first, first + len(instances)) (PerInstanceData records); rebuilds the acceleration structure."""
        instances = np.ascontiguousarray(instances)
        assert instances.dtype.itemsize == 160, "PerInstanceData records expected"
        self._check(lib.hrpt_update_instances(self._h, instances.ctypes.data, int(first), len(instances)))

    def refit_instances(self, instances, first=0):
        """update_instances for small motions: a tree built on the GPU keeps its hierarchy and gets new boxes (hrpt_refit_instances);
        build_info().usedBuilder then carries S.BVH_BUILDER_REFITTED."""
        instances = np.ascontiguousarray(instances)
        assert instances.dtype.itemsize == 160, "PerInstanceData records expected"
        self._check(lib.hrpt_refit_instances(self._h, instances.ctypes.data, int(first), len(instances)))

    def animate(self, animation, flags=0):
        """hrpt_animate: evaluates `animation` (an Animation) at its current times on the device and commits the instances like
        update_instances (S.ANIMATE_REFIT: like refit_instances); S.ANIMATE_NO_COMMIT: node worlds, palette and weights only, asynchronous."""
        self._check(lib.hrpt_animate(self._h, animation._h, int(flags)))

    def animation_device(self, animation):
        """hrpt_get_animation_device: device addresses (palette, weights, node worlds) of the last animate of `animation`; None for an
        empty array."""
        p = [C.c_void_p() for _ in range(3)]
        self._check(lib.hrpt_get_animation_device(self._h, animation._h, *[C.byref(x) for x in p]))
        return tuple(x.value for x in p)

    def read_animation(self, animation):
        """hrpt_read_animation: (palette [joints, 3, 4], weights, node worlds [nodes, 4, 4]) of the last animate (synchronises)."""
        palette = np.zeros((animation.joint_count, 3, 4), np.float32)
        weights = np.zeros(animation.morph_weight_count, np.float32)
        worlds = np.zeros((animation.node_count, 4, 4), np.float32)
        self._check(lib.hrpt_read_animation(self._h, animation._h, palette.ctypes.data, weights.ctypes.data, worlds.ctypes.data))
        return palette, weights, worlds

    def release_animation(self, animation):
        """hrpt_animation_release: drops the context's device copy of `animation`; the next animate uploads it again."""
        self._check(lib.hrpt_animation_release(self._h, animation._h))

    def update_lights(self, lights):
        """Replaces the light buffer (GPULight records; the count may change)."""
        lights = np.ascontiguousarray(lights)
        assert lights.dtype.itemsize == 64, "GPULight records expected"
        self._check(lib.hrpt_update_lights(self._h, lights.ctypes.data, len(lights)))

    def update_materials(self, materials, first=0):
        """New constants for the materials [first, first + len(materials)) (MaterialConstants records)."""
        materials = np.ascontiguousarray(materials)
        assert materials.dtype.itemsize == 180, "MaterialConstants records expected"
        self._check(lib.hrpt_update_materials(self._h, materials.ctypes.data, int(first), len(materials)))

    def update_vertices(self, vertices, first=0, flags=0):
        """hrpt_update_vertices: new S.VertexQuantized records for the vertices [first, first + len(vertices)) of the scene's vertex buffer;
        the acceleration structure and the per-triangle records follow. flags: S.VERTICES_REFIT (keep the hierarchy of a GPU-built flat
        tree), S.VERTICES_SAME_FRAME (a further range of the same frame: the previous positions render_motion_vectors reads are not
        reset first)."""
        vertices = np.ascontiguousarray(vertices)
        assert vertices.dtype.itemsize == 24, "VertexQuantized records expected"
        self._check(lib.hrpt_update_vertices(self._h, vertices.ctypes.data if len(vertices) else None, int(first), len(vertices), int(flags)))

    def update_vertices_device(self, ptr, first, count, flags=0, stream=0):
        """hrpt_update_vertices_device: the same from `count` S.VertexFloat records in device memory at `ptr` (16-byte aligned; e.g. a torch
        tensor's data_ptr()), quantised on the device. `stream` (integer handle, 0 = the default stream) is synchronised before they are read."""
        self._check(lib.hrpt_update_vertices_device(self._h, C.c_void_p(int(ptr)) if ptr else None, int(first), int(count), int(flags),
                                                    C.c_void_p(int(stream)) if stream else None))

    def end_vertex_frame(self):
        """A frame in which nothing deforms: previous positions = current positions, nothing is rebuilt (the count-0 call)."""
        self._check(lib.hrpt_update_vertices(self._h, None, 0, 0, 0))

    def quantize_vertices_device(self, in_ptr, count, out_ptr, stream=0):
        """hrpt_quantize_vertices_device: the quantiser kernel alone, `count` S.VertexFloat records at in_ptr (16-byte aligned) ->
        S.VertexQuantized records at out_ptr, both device addresses; asynchronous on `stream` (integer handle)."""
        self._check(lib.hrpt_quantize_vertices_device(self._h, C.c_void_p(int(in_ptr)) if in_ptr else None, int(count),
                                                      C.c_void_p(int(out_ptr)) if out_ptr else None, C.c_void_p(int(stream)) if stream else None))

    def skin_vertices_device(self, base, joints, weights, joint_matrices, deltas, morph_weights, count, joint_count, target_count, out_ptr,
                             status_ptr=0, stream=0):
        """hrpt_skin_vertices_device: the skinning kernel alone. The first six arguments are device addresses (0 = NULL) of the arrays
        skin_arrays() describes, out_ptr that of `count` S.VertexFloat records (16-byte aligned), status_ptr that of two zeroed uint32
        (word 0: an output position is not finite; word 1: a joint index is out of range) or 0. Asynchronous on `stream`."""
        args = S.SkinArgs(*[int(p) or None for p in (base, joints, weights, joint_matrices, deltas, morph_weights)], int(count), int(joint_count), int(target_count), 0)
        self._check(lib.hrpt_skin_vertices_device(self._h, C.byref(args), C.c_void_p(int(out_ptr)) if out_ptr else None,
                                                  C.c_void_p(int(status_ptr)) if status_ptr else None, C.c_void_p(int(stream)) if stream else None))

    def update_vertices_skinned(self, base, joints, weights, joint_matrices, deltas, morph_weights, count, joint_count, target_count, first,
                                flags=0, stream=0):
        """hrpt_update_vertices_skinned: update_vertices_device with the skinning kernel in front of the quantiser, in one call; the same
        device addresses as skin_vertices_device, for the vertices [first, first + count) of the scene."""
        args = S.SkinArgs(*[int(p) or None for p in (base, joints, weights, joint_matrices, deltas, morph_weights)], int(count), int(joint_count), int(target_count), 0)
        self._check(lib.hrpt_update_vertices_skinned(self._h, C.byref(args), int(first), int(flags), C.c_void_p(int(stream)) if stream else None))

    def build_info(self):
        bi = S.BuildInfo()
        self._check(lib.hrpt_get_build_info(self._h, C.byref(bi)))
        return bi

    def stats(self):
        st = S.Stats()
        self._check(lib.hrpt_get_stats(self._h, C.byref(st)))
        return st

    def post_process(self, params):
        self._check(lib.hrpt_post_process(self._h, C.byref(params)))

    def bloom(self, params=None):
        """Bloom composited into Output in place (hrpt_bloom): call between render and post_process, once per frame."""
        params = params if params is not None else S.BloomParams()
        self._check(lib.hrpt_bloom(self._h, C.byref(params)))

    def bloom_device(self, image_ptr, width, height, params=None, hip_stream=0):
        """The same over a caller-owned device image (width * height float4), asynchronously on `hip_stream` (integer handle)."""
        params = params if params is not None else S.BloomParams()
        self._check(lib.hrpt_bloom_device(self._h, C.c_void_p(int(image_ptr)), int(width), int(height), C.byref(params), C.c_void_p(int(hip_stream))))

    def clear_accumulation(self):
        """hrpt_clear_accumulation: zeroes the Accumulation image on the context stream, so that the next render may start a fresh frame at
        a non-zero accumulation index (new RNG seeds every frame -- what a temporal accumulator needs)."""
        self._check(lib.hrpt_clear_accumulation(self._h))

    def temporal_accumulate(self, view, prev_view, params=None):
        """hrpt_temporal_accumulate: reprojected accumulation of Output across frames, in place (csrc/pt_temporal.h).
        Frame order: clear_accumulation -> render -> render_motion_vectors(planes = 1 << S.GB_DEPTH | 1 << S.GB_NORMAL) -> temporal_accumulate
        -> bloom -> post_process. view / prev_view: S.PlanarViewConstants of this and of last frame; view["m_CameraDirectionOrPosition"]
        must hold (camera position, 1) -- scenes.planar_view leaves it zero, the caller fills it. The history lives in the context; the
        first call, the first call after resize and S.TEMPORAL_RESET run without it. Asynchronous."""
        params = params if params is not None else S.TemporalParams()
        v, pv = _view_record(view), _view_record(prev_view)
        self._check(lib.hrpt_temporal_accumulate(self._h, v.ctypes.data, pv.ctypes.data, C.byref(params)))

    def temporal_device(self, images, width, height, view, prev_view, params=None, hip_stream=0):
        """The same over caller-owned device images (S.TemporalImages of device addresses, width * height float4 each), asynchronously on
        `hip_stream` (integer handle). historyIn may be None (no history); historyOut must differ from it; colorOut may be color."""
        params = params if params is not None else S.TemporalParams()
        v, pv = _view_record(view), _view_record(prev_view)
        self._check(lib.hrpt_temporal_device(self._h, C.byref(images), int(width), int(height), v.ctypes.data, pv.ctypes.data, C.byref(params),
                                             C.c_void_p(int(hip_stream))))

    def read_temporal_history(self):
        """The history the last temporal_accumulate wrote: float32 [H, W, 4], rgb = accumulated radiance, a = age (synchronises)."""
        return self._read_image(lib.hrpt_read_temporal_history)

    def temporal_history_device(self):
        """Device pointer of that image (None before the first temporal_accumulate)."""
        return self._device_ptr(lib.hrpt_get_temporal_history_device)

    def upscale(self, display_width, display_height, view, prev_view, params=None):
        """hrpt_upscale: temporal upscaling of Output (the context's size) into a library-owned display_width x display_height image
        (csrc/pt_upscale.h). Frame order: clear_accumulation -> render(accum_count=1 at index i) ->
        render_motion_vectors(constants with m_Jitter = params.jitter, planes = 1 << S.GB_DEPTH) -> upscale -> bloom_device ->
        post_process_device, the last two over upscaled_device(). params.jitter = (halton(i + 1, 2) - 0.5, halton(i + 1, 3) - 0.5); with
        accum_count > 1 pass (0, 0) and render the planes without jitter. view / prev_view: the render-size views of this and of last
        frame. The history lives in the context; the first call, a call with another display size, the first call after resize and
        S.UPSCALE_RESET run without it. Asynchronous."""
        params = params if params is not None else S.UpscaleParams()
        v, pv = _view_record(view), _view_record(prev_view)
        self._check(lib.hrpt_upscale(self._h, int(display_width), int(display_height), v.ctypes.data, pv.ctypes.data, C.byref(params)))
        self._upscale_size = (int(display_width), int(display_height))

    def upscale_device(self, images, width, height, display_width, display_height, view, prev_view, params=None, hip_stream=0):
        """The same over caller-owned device images (S.UpscaleImages of device addresses), asynchronously on `hip_stream` (integer handle)."""
        params = params if params is not None else S.UpscaleParams()
        v, pv = _view_record(view), _view_record(prev_view)
        self._check(lib.hrpt_upscale_device(self._h, C.byref(images), int(width), int(height), int(display_width), int(display_height),
                                            v.ctypes.data, pv.ctypes.data, C.byref(params), C.c_void_p(int(hip_stream))))

    def _read_upscale_image(self, fn):
        W, H = getattr(self, "_upscale_size", (0, 0))
        out = np.empty((H, W, 4), np.float32)
        self._check(fn(self._h, out.ctypes.data, out.nbytes))
        return out

    def read_upscaled(self):
        """The colour image the last upscale wrote: float32 [H, W, 4] at its display size (synchronises)."""
        return self._read_upscale_image(lib.hrpt_read_upscaled)

    def read_upscale_history(self):
        """The history the last upscale wrote: rgb = resolved radiance, a = accumulated sample weight (synchronises)."""
        return self._read_upscale_image(lib.hrpt_read_upscale_history)

    def upscaled_device(self):
        """Device pointer of the upscaled colour image (None before the first upscale and after resize)."""
        return self._device_ptr(lib.hrpt_get_upscaled_device)

    def post_process_device(self, hdr_ptr, display_ptr, pixel_count, params, hip_stream=0):
        """hrpt_post_process_device: the HDR post chain over caller-owned device images (pixel_count float4 each), on the context's
        histogram and exposure, asynchronously on `hip_stream` (integer handle). The way from upscaled_device() to the tonemapper."""
        self._check(lib.hrpt_post_process_device(self._h, C.c_void_p(int(hdr_ptr)), C.c_void_p(int(display_ptr)), int(pixel_count), C.byref(params),
                                                 C.c_void_p(int(hip_stream))))

    def denoise(self, view, params=None):
        """hrpt_denoise: the edge-stopping Poisson filter over the temporal history (csrc/pt_denoise.h), after
        temporal_accumulate and before bloom; the planes S.GB_DEPTH, S.GB_NORMAL and S.GB_GEO_NORMAL must have been requested for this frame.
        params.iterations passes with a doubling radius; the last one also writes Output. By default the filtered image becomes the history
        the next temporal_accumulate reprojects (read_temporal_history returns it); with S.DENOISE_OUTPUT_ONLY the history is left alone and
        only Output is filtered. Asynchronous."""
        params = params if params is not None else S.DenoiseParams()
        v = _view_record(view)
        self._check(lib.hrpt_denoise(self._h, v.ctypes.data, C.byref(params)))

    def denoise_device(self, images, width, height, view, params=None, hip_stream=0):
        """One pass over caller-owned device images (S.DenoiseImages of device addresses; noise None = the default tile), asynchronously on
        `hip_stream` (integer handle). output must differ from input; color / colorOut are both None or both set; colorOut may be color."""
        params = params if params is not None else S.DenoiseParams()
        v = _view_record(view)
        self._check(lib.hrpt_denoise_device(self._h, C.byref(images), int(width), int(height), v.ctypes.data, C.byref(params), C.c_void_p(int(hip_stream))))

    def set_denoise_noise(self, tile):
        """hrpt_set_denoise_noise: the float32 [64, 64, 2] noise tile that denoise, and denoise_device without a tile, use from now on (e.g.
        native.noise_tile_from_png of the reference's blue-noise file); None restores the built-in default tile (white noise)."""
        if tile is None:
            self._check(lib.hrpt_set_denoise_noise(self._h, None))
            return
        t = np.ascontiguousarray(tile, np.float32)
        if t.shape != (64, 64, 2):
            raise ValueError("set_denoise_noise: a float32 [64, 64, 2] tile expected")
        self._check(lib.hrpt_set_denoise_noise(self._h, t.ctypes.data))

    def demodulate(self, view, params=None):
        """hrpt_demodulate: divides the first-hit BRDF factor out of Output, in place, and keeps the factor in a context image
        (csrc/pt_modulation.h). After render and render_motion_vectors / render_gbuffer with the planes S.GB_ALBEDO,
        S.GB_NORMAL, S.GB_GEO_NORMAL, S.GB_EMISSIVE and S.GB_DEPTH of this frame, before temporal_accumulate. view: as for
        temporal_accumulate. Asynchronous."""
        params = params if params is not None else S.ModulationParams()
        v = _view_record(view)
        self._check(lib.hrpt_demodulate(self._h, v.ctypes.data, C.byref(params)))

    def compose(self):
        """hrpt_compose: multiplies the factor the last demodulate stored back into Output and adds the emissive plane, in place; after
        denoise, before bloom. Asynchronous."""
        self._check(lib.hrpt_compose(self._h))

    def demodulate_device(self, images, width, height, view, params=None, hip_stream=0):
        """The demodulate stage over caller-owned device images (S.DemodulateImages of device addresses; emissive None = 0), asynchronously
        on `hip_stream` (integer handle). colorOut may be color; modulationOut must differ from every other image."""
        params = params if params is not None else S.ModulationParams()
        v = _view_record(view)
        self._check(lib.hrpt_demodulate_device(self._h, C.byref(images), int(width), int(height), v.ctypes.data, C.byref(params), C.c_void_p(int(hip_stream))))

    def compose_device(self, images, width, height, hip_stream=0):
        """The compose stage over caller-owned device images (S.ComposeImages of device addresses), asynchronously on `hip_stream`."""
        self._check(lib.hrpt_compose_device(self._h, C.byref(images), int(width), int(height), C.c_void_p(int(hip_stream))))

    def read_modulation(self):
        """The factor image the last demodulate wrote: float32 [H, W, 4], rgb = Mf, a = 1 at a hit, 0 at a miss (synchronises)."""
        return self._read_image(lib.hrpt_read_modulation)

    def modulation_device(self):
        """Device pointer of that image (None before the first demodulate and after a resize)."""
        return self._device_ptr(lib.hrpt_get_modulation_device)

    def deferred_lighting(self, constants, params=None):
        """hrpt_deferred_lighting: direct light with traced shadows, sky and optional probe indirect at the first hits, from the planes
        S.GB_ALBEDO, S.GB_NORMAL, S.GB_GEO_NORMAL, S.GB_EMISSIVE and S.GB_DEPTH of a render_gbuffer / render_motion_vectors with the same
        `constants`, into Output (csrc/pt_deferred.h). Accumulation is not touched. Default params: shadows and sky.
        Asynchronous."""
        params = params if params is not None else S.DeferredParams(S.DEFERRED_SHADOWS | S.DEFERRED_SKY)
        cb = np.ascontiguousarray(constants)
        self._check(lib.hrpt_deferred_lighting(self._h, cb.ctypes.data, C.byref(params)))

    def deferred_lighting_device(self, images, width, height, constants, params=None, hip_stream=0):
        """The same over caller-owned device images (S.DeferredImages of device addresses), with this context's scene and lights, every step
        on `hip_stream` (integer handle)."""
        params = params if params is not None else S.DeferredParams(S.DEFERRED_SHADOWS | S.DEFERRED_SKY)
        cb = np.ascontiguousarray(constants)
        self._check(lib.hrpt_deferred_lighting_device(self._h, C.byref(images), int(width), int(height), cb.ctypes.data, C.byref(params), C.c_void_p(int(hip_stream))))

    def read_display(self):
        return self._read_image(lib.hrpt_read_display)

    def exposure(self):
        e = C.c_float(); h = np.zeros(256, np.uint32)
        self._check(lib.hrpt_get_exposure(self._h, C.byref(e), h.ctypes.data))
        return e.value, h

    def set_exposure(self, v):
        self._check(lib.hrpt_set_exposure(self._h, v))

    def selftest_f16_decode(self):
        out = np.empty(65536, np.float32)
        self._check(lib.hrpt_selftest_f16_decode(self._h, out.ctypes.data))
        return out

    def selftest_bvh(self):
        """Number of child boxes of the acceleration structure that do not contain their subtree (0 = sound)."""
        v = C.c_uint64()
        self._check(lib.hrpt_selftest_bvh(self._h, C.byref(v)))
        return int(v.value)

    def read_bvh(self):
        """hrpt_selftest_read_bvh: the structure the kernels currently walk, as host arrays (see _read_bvh_dump)."""
        return _read_bvh_dump(lambda d: self._check(lib.hrpt_selftest_read_bvh(self._h, C.byref(d))))

    def selftest_unorm8(self):
        out = np.empty(512, np.float32)
        self._check(lib.hrpt_selftest_unorm8(self._h, out.ctypes.data))
        return out[:256], out[256:]

    def selftest_sample_textures(self, probes):
        """hrpt_selftest_sample_textures: probes = structured array of S.TextureProbe over the uploaded scene's materials; returns a
        structured array of S.TextureProbeResult (the shader's one-by-one, batched and gradient sampling of every probe)."""
        probes = np.ascontiguousarray(probes, S.TextureProbe)
        results = np.zeros(len(probes), S.TextureProbeResult)
        self._check(lib.hrpt_selftest_sample_textures(self._h, probes.ctypes.data if len(probes) else None, results.ctypes.data if len(probes) else None,
                                                      len(probes)))
        return results

    def selftest_atmosphere(self, probes):
        """hrpt_selftest_atmosphere: probes = structured array of S.AtmosphereProbe; returns a structured array of S.AtmosphereProbeResult
        (the device's sky radiance, sun radiance and transmittance lookup of every probe over the uploaded scene's tables)."""
        probes = np.ascontiguousarray(probes, S.AtmosphereProbe)
        results = np.zeros(len(probes), S.AtmosphereProbeResult)
        self._check(lib.hrpt_selftest_atmosphere(self._h, probes.ctypes.data if len(probes) else None, results.ctypes.data if len(probes) else None,
                                                 len(probes)))
        return results

    def reset_stats(self):
        self._check(lib.hrpt_reset_stats(self._h))
