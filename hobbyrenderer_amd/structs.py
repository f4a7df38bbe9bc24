"""numpy / ctypes mirrors of the reference's GPU struct layouts (include/hobbyrt_pt.h).

Reference: src/shaders/Mesh.sr:9-25, Instance.sr:2-65, GPULight.sr:1-13, Common.sr:17-43,
PathTracer.sr:6-17 under /root/reference. Sizes are asserted at import.
"""
import ctypes as C

import numpy as np

f32, u32 = np.float32, np.uint32

VertexQuantized = np.dtype([("m_Pos", f32, 3), ("m_Normal", u32), ("m_Uv", u32), ("m_Tangent", u32)])
# HrptVertexFloat: what hrpt_update_vertices_device / hrpt_quantize_vertices_* read; tangent[3] = handedness sign
VertexFloat = np.dtype([("pos", f32, 3), ("normal", f32, 3), ("uv", f32, 2), ("tangent", f32, 4)])
MeshData = np.dtype([("m_LODCount", u32), ("m_IndexOffsets", u32, 8), ("m_IndexCounts", u32, 8),
                     ("m_MeshletOffsets", u32, 8), ("m_MeshletCounts", u32, 8), ("m_LODErrors", f32, 8)])
Meshlet = np.dtype([("m_CenterRadius", u32, 2), ("m_VertexOffset", u32), ("m_TriangleOffset", u32), ("m_VertexCount", u32),
                    ("m_TriangleCount", u32), ("m_ConeAxisAndCutoff", u32)])                    # Mesh.sr:27-35, 28 B
Primitive = np.dtype([("m_VertexOffset", u32), ("m_VertexCount", u32), ("m_MaterialIndex", np.int32), ("m_MeshDataIndex", u32)])  # as serialised, 16 B
PerInstanceData = np.dtype([("m_World", f32, (4, 4)), ("m_PrevWorld", f32, (4, 4)), ("m_MaterialIndex", u32),
                            ("m_MeshDataIndex", u32), ("m_Radius", f32), ("m_LODIndex", u32), ("m_Center", f32, 3),
                            ("m_FirstGeometryInstanceIndex", u32)])
MaterialConstants = np.dtype([
    ("m_BaseColor", f32, 4), ("m_EmissiveFactor", f32, 4), ("m_RoughnessMetallic", f32, 2), ("m_TextureFlags", u32),
    ("m_AlbedoTextureIndex", u32), ("m_NormalTextureIndex", u32), ("m_RoughnessMetallicTextureIndex", u32),
    ("m_EmissiveTextureIndex", u32), ("m_AlbedoSamplerIndex", u32), ("m_NormalSamplerIndex", u32),
    ("m_RoughnessSamplerIndex", u32), ("m_EmissiveSamplerIndex", u32), ("m_AlbedoMinMipIndex", u32),
    ("m_NormalMinMipIndex", u32), ("m_RoughnessMinMipIndex", u32), ("m_EmissiveMinMipIndex", u32),
    ("m_AlbedoFeedbackIndex", u32), ("m_NormalFeedbackIndex", u32), ("m_RoughnessFeedbackIndex", u32),
    ("m_EmissiveFeedbackIndex", u32), ("m_MinMipDimsX", u32), ("m_MinMipDimsY", u32), ("m_AlphaMode", u32),
    ("m_AlphaCutoff", f32), ("m_IOR", f32), ("m_TransmissionFactor", f32), ("m_ThicknessFactor", f32),
    ("m_AttenuationDistance", f32), ("m_AttenuationColor", f32, 3), ("m_SigmaA", f32, 3), ("m_IsThinSurface", u32),
    ("m_SigmaS", f32, 3)])
GPULight = np.dtype([("m_Position", f32, 3), ("m_Intensity", f32), ("m_Direction", f32, 3), ("m_Type", u32),
                     ("m_Color", f32, 3), ("m_Range", f32), ("m_SpotInnerConeAngle", f32), ("m_SpotOuterConeAngle", f32),
                     ("m_Radius", f32), ("m_CosSunAngularRadius", f32)])
_MATS = ["m_MatWorldToView", "m_MatViewToClip", "m_MatWorldToClip", "m_MatClipToView", "m_MatViewToWorld",
         "m_MatClipToWorld", "m_MatViewToClipNoOffset", "m_MatWorldToClipNoOffset", "m_MatClipToViewNoOffset",
         "m_MatClipToWorldNoOffset"]
PlanarViewConstants = np.dtype([(m, f32, (4, 4)) for m in _MATS] + [
    ("m_ViewportOrigin", f32, 2), ("m_ViewportSize", f32, 2), ("m_ViewportSizeInv", f32, 2), ("m_PixelOffset", f32, 2),
    ("m_ClipToWindowScale", f32, 2), ("m_ClipToWindowBias", f32, 2), ("m_CameraDirectionOrPosition", f32, 4)])
PathTracerConstants = np.dtype([
    ("m_View", PlanarViewConstants), ("m_CameraPos", f32, 4), ("m_LightCount", u32), ("m_AccumulationIndex", u32),
    ("m_FrameIndex", u32), ("m_MaxBounces", u32), ("m_Jitter", f32, 2), ("m_Pad0", f32, 2), ("m_SunDirection", f32, 3),
    ("m_CosSunAngularRadius", f32)])
FrameParams = np.dtype([("constants", PathTracerConstants), ("accumCount", u32), ("tileX0", u32), ("tileY0", u32),
                        ("tileX1", u32), ("tileY1", u32), ("flags", u32), ("stripeCount", u32), ("stripeIndex", u32)])

assert VertexFloat.itemsize == 48
assert VertexQuantized.itemsize == 24 and MeshData.itemsize == 164 and PerInstanceData.itemsize == 160
assert MaterialConstants.itemsize == 180 and GPULight.itemsize == 64
assert PlanarViewConstants.itemsize == 704 and PathTracerConstants.itemsize == 768
assert PathTracerConstants.fields["m_SunDirection"][1] == 752 and PathTracerConstants.fields["m_Jitter"][1] == 736

TEXFLAG_ALBEDO, TEXFLAG_NORMAL, TEXFLAG_ROUGHNESS_METALLIC, TEXFLAG_EMISSIVE = 1, 2, 4, 8
ALPHA_MODE_OPAQUE, ALPHA_MODE_MASK, ALPHA_MODE_BLEND = 0, 1, 2
TEXTURE_PROBE_SLOT_FLAGS = (TEXFLAG_ALBEDO, TEXFLAG_ROUGHNESS_METALLIC, TEXFLAG_EMISSIVE, TEXFLAG_NORMAL)
LIGHT_DIRECTIONAL, LIGHT_POINT, LIGHT_SPOT = 0, 1, 2
FRAME_DEFAULT, FRAME_MEGAKERNEL, FRAME_WAVEFRONT, FRAME_PROFILE = 0, 1, 2, 4

LUT_TRANSMITTANCE_SHAPE = (64, 256, 4)
LUT_SCATTERING_SHAPE = (32, 128, 256, 4)
LUT_IRRADIANCE_SHAPE = (16, 64, 4)


class TextureDesc(C.Structure):      # HrptTextureDesc
    _fields_ = [("texels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_uint32), ("mipCount", C.c_uint32)]


TEXTURE_FORMAT_RGBA8_UNORM, TEXTURE_FORMAT_RGBA8_SRGB, TEXTURE_FORMAT_RGBA16_FLOAT, TEXTURE_FORMAT_RGBA32_FLOAT = 0, 1, 2, 3
TEXTURE_BYTES_PER_TEXEL = {0: 4, 1: 4, 2: 8, 3: 16}


def mip_dims(width, height, mip_count):
    return [(max(1, width >> l), max(1, height >> l)) for l in range(max(1, mip_count))]


class Texture:
    """A decoded texture with its format and mip chain (HrptTextureDesc): `data` = all levels, level 0 first, tightly packed bytes.
    SceneArrays.textures entries are either one of these or a plain (H, W, 4) uint8 array (RGBA8_UNORM, one level)."""

    def __init__(self, data, width, height, fmt=TEXTURE_FORMAT_RGBA8_UNORM, mip_count=1):
        self.data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.width, self.height, self.format, self.mip_count = int(width), int(height), int(fmt), max(1, int(mip_count))
        expect = sum(w * h for w, h in mip_dims(self.width, self.height, self.mip_count)) * TEXTURE_BYTES_PER_TEXEL[self.format]
        if self.data.size != expect:
            raise ValueError(f"texture data holds {self.data.size} bytes, {expect} expected for {width}x{height}, format {fmt}, {mip_count} level(s)")

    def level(self, l):
        """Level l as an array (h, w, 4) of uint8 / float16 / float32."""
        dims = mip_dims(self.width, self.height, self.mip_count)
        bpt = TEXTURE_BYTES_PER_TEXEL[self.format]
        off = sum(w * h for w, h in dims[:l]) * bpt
        w, h = dims[l]
        raw = self.data[off:off + w * h * bpt]
        dt = {4: np.uint8, 8: np.float16, 16: np.float32}[bpt]
        return raw.view(dt).reshape(h, w, 4)


class SceneDesc(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("vertexCount", C.c_uint32),
                ("indices", C.c_void_p), ("indexCount", C.c_uint32),
                ("meshData", C.c_void_p), ("meshDataCount", C.c_uint32),
                ("instances", C.c_void_p), ("instanceCount", C.c_uint32),
                ("materials", C.c_void_p), ("materialCount", C.c_uint32),
                ("lights", C.c_void_p), ("lightCount", C.c_uint32),
                ("textures", C.POINTER(TextureDesc)), ("textureCount", C.c_uint32),
                ("brunetonTransmittance", C.c_void_p), ("brunetonScattering", C.c_void_p),
                ("brunetonIrradiance", C.c_void_p)]


class DeviceDesc(C.Structure):
    _fields_ = [("deviceOrdinal", C.c_int32), ("abiVersion", C.c_uint32)]


class PostParams(C.Structure):
    _fields_ = [("autoExposure", C.c_uint32), ("manualExposure", C.c_float), ("deltaTimeSeconds", C.c_float), ("adaptationSpeed", C.c_float),
                ("exposureValueMin", C.c_float), ("exposureValueMax", C.c_float), ("exposureCompensation", C.c_float),
                ("hdrDisplay", C.c_uint32), ("maxDisplayNits", C.c_float)]


class BloomParams(C.Structure):
    """HrptBloomParams; the defaults are the reference's (Renderer::m_BloomKnee, m_BloomIntensity, m_UpsampleRadius)."""
    _fields_ = [("knee", C.c_float), ("intensity", C.c_float), ("upsampleRadius", C.c_float), ("reserved", C.c_uint32)]

    def __init__(self, knee=0.1, intensity=0.005, upsampleRadius=0.85, reserved=0):
        super().__init__(knee, intensity, upsampleRadius, reserved)


TEMPORAL_LINEAR, TEMPORAL_RESET = 1, 2          # HrptTemporalParams::flags


class TemporalParams(C.Structure):
    """HrptTemporalParams; blend defaults to the reference's m_SSGI_TemporalBlend (Renderer.h:358). flags: TEMPORAL_LINEAR blends in linear
    radiance (the unbiased running mean) instead of the reference's log(1 + x) space; TEMPORAL_RESET ignores the context's stored history."""
    _fields_ = [("blend", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]

    def __init__(self, blend=0.9, flags=0):
        super().__init__(blend, flags, (C.c_uint32 * 2)(0, 0))


class TemporalImages(C.Structure):
    """HrptTemporalImages: host or device addresses of width x height float4 images."""
    _fields_ = [(n, C.c_void_p) for n in ("color", "motion", "depth", "normal", "historyIn", "historyOut", "colorOut")]


UPSCALE_NO_CLAMP, UPSCALE_RESET = 1, 2          # HrptUpscaleParams::flags


class UpscaleParams(C.Structure):
    """HrptUpscaleParams. jitter: this frame's sample offset in render pixels (the m_Jitter it was rendered with), each in [-0.5, 0.5];
    kernel: tap weight exp(-kernel * d^2) with d in display pixels, in (0, 16]; maxHistory: cap of the accumulated sample weight, >= 0.
    flags: UPSCALE_NO_CLAMP skips the clamp of the history to the taps' colour range; UPSCALE_RESET ignores the context's stored history."""
    _fields_ = [("jitter", C.c_float * 2), ("kernel", C.c_float), ("maxHistory", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]

    def __init__(self, jitter=(0.0, 0.0), kernel=2.29, maxHistory=8.0, flags=0):
        super().__init__((C.c_float * 2)(float(jitter[0]), float(jitter[1])), kernel, maxHistory, flags, (C.c_uint32 * 3)(0, 0, 0))


class UpscaleImages(C.Structure):
    """HrptUpscaleImages: host or device addresses of float4 images; color / depth / motion at the render size, historyIn (may be None) /
    historyOut / colorOut at the display size."""
    _fields_ = [(n, C.c_void_p) for n in ("color", "depth", "motion", "historyIn", "historyOut", "colorOut")]


DENOISE_OUTPUT_ONLY = 1                         # HrptDenoiseParams::flags


class DenoiseParams(C.Structure):
    """HrptDenoiseParams; the defaults are the reference's m_SSGI_Denoise* (Renderer.h:362-368). iterations: passes of the context call
    (1..5; pass i uses radius * 2^i and frame * iterations + i), 1 for the single-pass calls. flags: DENOISE_OUTPUT_ONLY filters Output and
    leaves the context's temporal history as the temporal stage wrote it."""
    _fields_ = [("radius", C.c_float), ("phi", C.c_float), ("lumaPhi", C.c_float), ("depthPhi", C.c_float), ("normalPhi", C.c_float),
                ("roughnessPhi", C.c_float), ("iterations", C.c_uint32), ("frame", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, radius=3.0, phi=0.5, lumaPhi=5.0, depthPhi=2.0, normalPhi=50.0, roughnessPhi=50.0, iterations=1, frame=0, flags=0, reserved=0):
        super().__init__(radius, phi, lumaPhi, depthPhi, normalPhi, roughnessPhi, iterations, frame, flags, reserved)


class DenoiseImages(C.Structure):
    """HrptDenoiseImages: host or device addresses of width x height float4 images; noise: 64 * 64 * 2 floats or None (the default tile);
    color / colorOut: both None or both set."""
    _fields_ = [(n, C.c_void_p) for n in ("input", "depth", "normal", "geoNormal", "noise", "output", "color", "colorOut")]


class ModulationParams(C.Structure):
    """HrptModulationParams; floor is the lower bound of every channel of the factor the demodulate stage divides by (default 0.04: the
    least value a non-metal's factor takes, so it only bites on dark metals)."""
    _fields_ = [("floor", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]

    def __init__(self, floor=0.04, flags=0):
        super().__init__(floor, flags, (C.c_uint32 * 2)(0, 0))


class DemodulateImages(C.Structure):
    """HrptDemodulateImages: host or device addresses of width x height float4 images; emissive may be None (= 0); colorOut may be color."""
    _fields_ = [(n, C.c_void_p) for n in ("color", "albedo", "normal", "geoNormal", "depth", "emissive", "colorOut", "modulationOut")]


class ComposeImages(C.Structure):
    """HrptComposeImages: host or device addresses of width x height float4 images; emissive may be None (= 0); colorOut may be color."""
    _fields_ = [(n, C.c_void_p) for n in ("color", "modulation", "emissive", "colorOut")]


# HrptSkinMorphDelta: one vertex of one morph target (hrpt_skin_vertices_* / hrpt_update_vertices_skinned), 36 B
SkinMorphDelta = np.dtype([("pos", f32, 3), ("normal", f32, 3), ("tangent", f32, 3)])
assert SkinMorphDelta.itemsize == 36
SKIN_LDS_MAX_JOINTS = 256          # HRPT_SKIN_LDS_MAX_JOINTS: up to this many joints the kernels serve the palette from LDS


class SkinArgs(C.Structure):
    """HrptSkinArgs: host addresses for skin_vertices_host, device addresses for the two context calls. joints None: no skinning;
    deltas None iff targetCount == 0."""
    _fields_ = [(n, C.c_void_p) for n in ("base", "joints", "weights", "jointMatrices", "deltas", "morphWeights")] + \
               [(n, C.c_uint32) for n in ("count", "jointCount", "targetCount", "reserved")]


# ---- keyframe animation (hrpt_animation_create, hrpt_animate_host, hrpt_animate; csrc/pt_anim.h has the definition) ----
ANIM_PATH_TRANSLATION, ANIM_PATH_ROTATION, ANIM_PATH_SCALE, ANIM_PATH_WEIGHTS = 0, 1, 2, 3
ANIM_STEP, ANIM_LINEAR, ANIM_CUBICSPLINE, ANIM_CATMULLROM, ANIM_SLERP = 0, 1, 2, 3, 4
ANIMATE_REFIT, ANIMATE_NO_COMMIT = 1, 2
ANIM_LDS_MAX_ANIMATIONS = 256      # HRPT_ANIM_LDS_MAX_ANIMATIONS: up to this many animation times the sampling kernel stages in LDS
AnimSampler = np.dtype([("interpolation", u32), ("firstKey", u32), ("keyCount", u32), ("animation", u32)])
AnimChannel = np.dtype([("path", u32), ("sampler", u32), ("firstTarget", u32), ("targetCount", u32)])
AnimNode = np.dtype([("parent", np.int32), ("translation", f32, 3), ("rotation", f32, 4), ("scale", f32, 3), ("baseWorld", f32, (4, 4)),
                     ("firstInstance", u32), ("instanceCount", u32)])
AnimJoint = np.dtype([("node", u32), ("inverseBind", f32, (4, 4))])
assert AnimSampler.itemsize == 16 and AnimChannel.itemsize == 16 and AnimNode.itemsize == 116 and AnimJoint.itemsize == 68


class AnimationDesc(C.Structure):
    """HrptAnimationDesc: host addresses of the flat tables and their counts."""
    _fields_ = [(n, C.c_void_p) for n in ("samplers", "channels", "nodes", "joints", "keyTimes", "keyValues", "targets", "nodeInstances")] + \
               [(n, C.c_uint32) for n in ("samplerCount", "channelCount", "nodeCount", "jointCount", "keyCount", "targetCount", "nodeInstanceCount",
                                          "animationCount", "morphWeightCount", "reserved")]


class Stats(C.Structure):
    _fields_ = [("closestRays", C.c_uint64), ("shadowRays", C.c_uint64), ("paths", C.c_uint64),
                ("lastRenderMs", C.c_float), ("traceKernelMs", C.c_float), ("traceKernelLaunches", C.c_uint32),
                ("shadeKernelMs", C.c_float), ("shadeKernelLaunches", C.c_uint32),
                ("shadowKernelMs", C.c_float), ("shadowKernelLaunches", C.c_uint32),
                ("bvhNodeCount", C.c_uint32), ("bvhTriangleCount", C.c_uint32), ("bvhMaxDepth", C.c_uint32),
                ("megakernelFallbacks", C.c_uint32), ("raygenKernelMs", C.c_float), ("raygenKernelLaunches", C.c_uint32),
                ("resolveKernelMs", C.c_float), ("resolveKernelLaunches", C.c_uint32), ("pad0", C.c_uint32),
                ("raygenQueueBytes", C.c_uint64), ("traceQueueBytes", C.c_uint64), ("shadeQueueBytes", C.c_uint64),
                ("shadowQueueBytes", C.c_uint64), ("resolveQueueBytes", C.c_uint64), ("neeEntries", C.c_uint64),
                ("neeSamples", C.c_uint64), ("queuePoolBytes", C.c_uint64)]


Ray = np.dtype([("origin", f32, 3), ("tmin", f32), ("direction", f32, 3), ("tmax", f32), ("rng", u32), ("pad", u32, 3)])       # HrptRay, 48 B
RayHit = np.dtype([("t", f32), ("u", f32), ("v", f32), ("instance", u32), ("primitive", u32), ("hit", u32), ("rng", u32), ("pad", u32)])   # HrptRayHit, 32 B
RAYS_CLOSEST, RAYS_SHADOW, RAYS_DEVICE_POINTERS, RAYS_THREAD_PER_RAY = 0, 1, 0x100, 0x200
RADIANCE_DEVICE_POINTERS, RADIANCE_THREAD_PER_RAY, RADIANCE_ACCUMULATE = 0x100, 0x200, 0x400       # hrpt_trace_radiance flags
RADIANCE_SECONDARY = 0x1000     # ray i is path segment 1 (a ray that leaves a first hit), not 0
# first-hit G-buffer (hrpt_render_gbuffer): plane indices HRPT_GB_*, the all-planes mask, the flag bits of the ids plane's w
GB_ALBEDO, GB_NORMAL, GB_GEO_NORMAL, GB_EMISSIVE, GB_DEPTH, GB_IDS, GB_PLANES = 0, 1, 2, 3, 4, 5, 6
GB_ALL_PLANES = 0x3F
GB_FLAG_HIT, GB_FLAG_FRONT_FACE = 1, 2
# hrpt_selftest_sample_textures; slots of single / batched: albedo, roughness-metallic, emissive, normal (TEXTURE_PROBE_SLOT_FLAGS)
TextureProbe = np.dtype([("material", u32), ("uv", f32, 2), ("ddx", f32, 2), ("ddy", f32, 2), ("texFlags", u32)])                       # HrptTextureProbe, 32 B
TextureProbeResult = np.dtype([("single", f32, (4, 4)), ("batched", f32, (4, 4)), ("batchedAccepted", u32), ("pad", u32, 3), ("grad", f32, 4)])   # HrptTextureProbeResult, 160 B
assert TextureProbe.itemsize == 32 and TextureProbeResult.itemsize == 160
# hrpt_selftest_atmosphere: the run-time sky / sun / transmittance lookups on one camera position, view ray and sun direction
AtmosphereProbe = np.dtype([("cameraPos", f32, 3), ("viewRay", f32, 3), ("sunDir", f32, 3), ("sunIntensity", f32), ("addSunDisk", u32), ("pad", u32)])   # HrptAtmosphereProbe, 48 B
AtmosphereProbeResult = np.dtype([("sky", f32, 3), ("sun", f32, 3), ("transmittance", f32, 3), ("r", f32), ("mu", f32), ("pad", f32)])                  # HrptAtmosphereProbeResult, 48 B
assert AtmosphereProbe.itemsize == 48 and AtmosphereProbeResult.itemsize == 48
# irradiance probe volume (hrpt_probes_*)
ProbeVolume = np.dtype([("origin", f32, 3), ("hysteresis", f32), ("spacing", f32, 3), ("maxRayDistance", f32), ("counts", u32, 3), ("raysPerProbe", u32),
                        ("distanceExponent", f32), ("normalBias", f32), ("viewBias", f32), ("pad", u32)])                               # HrptProbeVolume, 64 B
ProbePoint = np.dtype([("position", f32, 3), ("pad0", f32), ("normal", f32, 3), ("pad1", f32), ("view", f32, 3), ("pad2", f32)])       # HrptProbePoint, 48 B
assert ProbeVolume.itemsize == 64 and ProbePoint.itemsize == 48
PROBES_RESET, PROBES_DEVICE_POINTERS = 1, 0x100
PROBE_IRRADIANCE_SHAPE, PROBE_DISTANCE_SHAPE = (8, 8, 4), (16, 16, 2)      # one probe's tiles; the atlases are [P, 8, 8, 4] and [P, 16, 16, 2]
# deferred lighting (hrpt_deferred_lighting)
DEFERRED_SHADOWS, DEFERRED_SKY, DEFERRED_INDIRECT = 1, 2, 4


class DeferredParams(C.Structure):
    """HrptDeferredParams. flags: DEFERRED_SHADOWS traces one shadow ray per lit (pixel, light) pair, DEFERRED_SKY takes the sky at misses and
    the sun's radiance from the atmosphere, DEFERRED_INDIRECT adds the diffuse indirect image times indirectIntensity."""
    _fields_ = [("flags", C.c_uint32), ("indirectIntensity", C.c_float), ("reserved", C.c_uint32 * 2)]

    def __init__(self, flags=0, indirectIntensity=1.0):
        super().__init__(flags, indirectIntensity)


class DeferredImages(C.Structure):
    """HrptDeferredImages: host or device addresses of width x height float4 images; indirect may be None without DEFERRED_INDIRECT."""
    _fields_ = [(n, C.c_void_p) for n in ("albedo", "normal", "geoNormal", "emissive", "depth", "indirect", "colorOut")]


# traced indirect lighting (hrpt_indirect_lighting)
INDIRECT_DIFFUSE, INDIRECT_SPECULAR, INDIRECT_THREAD_PER_RAY = 1, 2, 0x200


class IndirectParams(C.Structure):
    """HrptIndirectParams. flags: INDIRECT_DIFFUSE / INDIRECT_SPECULAR pick the lobes (at least one), INDIRECT_THREAD_PER_RAY traces with the
    one-thread-per-ray kernel; frameSeed seeds the per-pixel draws; intensity scales what compose adds."""
    _fields_ = [("flags", C.c_uint32), ("frameSeed", C.c_uint32), ("intensity", C.c_float), ("reserved", C.c_uint32)]

    def __init__(self, flags=INDIRECT_DIFFUSE | INDIRECT_SPECULAR, frameSeed=0, intensity=1.0):
        super().__init__(flags, frameSeed, intensity)


class IndirectImages(C.Structure):
    """HrptIndirectImages: host or device addresses of width x height float4 images. Lighting / resolve write diffuse and specular (the plane of
    a lobe that is not flagged may be None); compose reads them and adds into colorInOut."""
    _fields_ = [(n, C.c_void_p) for n in ("albedo", "normal", "geoNormal", "depth", "diffuse", "specular", "colorInOut")]


# resampled direct lighting (hrpt_restir_lighting)
RESTIR_SHADOWS, RESTIR_SKY, RESTIR_TEMPORAL, RESTIR_SPATIAL, RESTIR_INITIAL_VISIBILITY, RESTIR_RESET = 1, 2, 4, 8, 16, 32
RESTIR_EMPTY = 0xFFFFFFFF          # HrptRestirReservoir.light of an empty reservoir
RESTIR_LDS_MAX_LIGHTS = 512
RestirReservoir = np.dtype([("light", u32), ("W", f32), ("M", f32), ("pHat", f32)])       # HrptRestirReservoir, 16 B


class RestirParams(C.Structure):
    """HrptRestirParams. flags: RESTIR_SHADOWS traces the chosen light's shadow ray, RESTIR_SKY takes the sky at misses and the sun's radiance
    from the atmosphere, RESTIR_TEMPORAL / RESTIR_SPATIAL switch the two reuse passes on, RESTIR_INITIAL_VISIBILITY adds a shadow ray for the
    initial sample (biased), RESTIR_RESET drops the history. The defaults are the documented ones."""
    _fields_ = [("flags", C.c_uint32), ("frameSeed", C.c_uint32), ("candidates", C.c_uint32), ("spatialSamples", C.c_uint32), ("spatialRadius", C.c_float),
                ("maxHistory", C.c_float), ("depthThreshold", C.c_float), ("normalThreshold", C.c_float), ("reserved", C.c_uint32 * 4)]

    def __init__(self, flags=RESTIR_SHADOWS | RESTIR_SKY | RESTIR_TEMPORAL | RESTIR_SPATIAL, frameSeed=0, candidates=8, spatialSamples=1, spatialRadius=32.0,
                 maxHistory=20.0, depthThreshold=0.1, normalThreshold=0.5):
        super().__init__(flags, frameSeed, candidates, spatialSamples, spatialRadius, maxHistory, depthThreshold, normalThreshold)


class RestirImages(C.Structure):
    """HrptRestirImages: host or device addresses. The five planes and motion are width x height float4 images (motion may be None without
    RESTIR_TEMPORAL); reservoirIn / keyIn are the history (both None = none); reservoirOut (RestirReservoir records), keyOut and colorOut are
    written."""
    _fields_ = [(n, C.c_void_p) for n in ("albedo", "normal", "geoNormal", "emissive", "depth", "motion", "reservoirIn", "keyIn", "reservoirOut", "keyOut", "colorOut")]


# hash-grid radiance cache (hrpt_rcache_*)
RCACHE_RESET, RCACHE_NO_FALLBACK, RCACHE_NO_WAVE_COMBINE = 1, 2, 4
RcacheDesc = np.dtype([("capacityLog2", u32), ("sceneScale", f32), ("levelBias", f32), ("radianceScale", f32), ("maxSamples", u32), ("staleFramesMax", u32),
                       ("sparseBlock", u32), ("roughnessThreshold", f32)])                                                                  # HrptRcacheDesc, 32 B
RcacheAccum = np.dtype([("r", np.uint64), ("g", np.uint64), ("b", np.uint64), ("count", u32), ("pad", u32)])                               # HrptRcacheAccum, 32 B
RcacheEntry = np.dtype([("r", f32), ("g", f32), ("b", f32), ("meta", u32)])                                    # HrptRcacheEntry, 16 B; meta = samples | stale << 16
RcacheSample = np.dtype([("position", f32, 3), ("valid", f32), ("normal", f32, 3), ("pad0", f32), ("radiance", f32, 3), ("pad1", f32)])    # HrptRcacheSample, 48 B
RcachePoint = np.dtype([("position", f32, 3), ("pad0", f32), ("normal", f32, 3), ("pad1", f32)])                                           # HrptRcachePoint, 32 B
RcacheSurface = np.dtype([("position", f32, 3), ("t", f32), ("normal", f32, 3), ("hit", u32), ("rng", u32), ("pad", u32, 3)])              # HrptRcacheSurface, 48 B
assert (RcacheDesc.itemsize, RcacheAccum.itemsize, RcacheEntry.itemsize, RcacheSample.itemsize, RcachePoint.itemsize, RcacheSurface.itemsize) == (32, 32, 16, 48, 32, 48)


class RcacheParams(C.Structure):
    """HrptRcacheParams. flags: RCACHE_NO_FALLBACK leaves pixels the cache does not serve at zero instead of tracing their path."""
    _fields_ = [("flags", C.c_uint32), ("frameSeed", C.c_uint32), ("reserved", C.c_uint32 * 2)]

    def __init__(self, flags=0, frameSeed=0):
        super().__init__(flags, frameSeed)


class BuildInfo(C.Structure):      # HrptBuildInfo, 64 B
    _fields_ = [("requestedBuilder", C.c_uint32), ("usedBuilder", C.c_uint32), ("buildMs", C.c_float), ("deviceBuildMs", C.c_float),
                ("triangleCount", C.c_uint32), ("nodeCount", C.c_uint32), ("node4Count", C.c_uint32), ("maxDepth", C.c_uint32),
                ("maxDepth4", C.c_uint32), ("mortonBits", C.c_uint32), ("sahCost", C.c_float), ("structure", C.c_uint32),
                ("instanceNodeCount", C.c_uint32), ("distinctMeshes", C.c_uint32), ("leafAreaPermille", C.c_uint32), ("nodeFormat", C.c_uint32)]


# Records of the acceleration structure as the kernels read them (csrc/pt_scene_records.h), for hrpt_selftest_read_bvh / hrpt_selftest_host_build.
i32 = np.int32
GpuNode = np.dtype([("lmin", f32, 3), ("left", i32), ("lmax", f32, 3), ("right", i32), ("rmin", f32, 3), ("pad0", u32), ("rmax", f32, 3), ("pad1", u32)])
GpuNode4 = np.dtype([("minx", f32, 4), ("maxx", f32, 4), ("miny", f32, 4), ("maxy", f32, 4), ("minz", f32, 4), ("maxz", f32, 4), ("child", i32, 4), ("pad", u32, 4)])
GpuNodeQ = np.dtype([("o", f32, 3), ("sx", f32), ("lox", u32), ("hix", u32), ("loy", u32), ("hiy", u32), ("loz", u32), ("hiz", u32), ("sy", f32), ("sz", f32),
                     ("child", i32, 4)])
GpuTri = np.dtype([("p0", f32, 3), ("inst", u32), ("p1", f32, 3), ("prim", u32), ("p2", f32, 3), ("flags", u32)])
GpuTriAttr = np.dtype([("n0", f32, 3), ("n1", f32, 3), ("n2", f32, 3), ("uv0", f32, 2), ("uv1", f32, 2), ("uv2", f32, 2), ("material", u32), ("inst", u32),
                       ("prim", u32), ("pad", u32, 2)])
GpuTriTangent = np.dtype([("t0", f32, 4), ("t1", f32, 4), ("t2", f32, 4)])
GpuInstance = np.dtype([("world", f32, (4, 3)), ("inv", f32, (4, 3)), ("blasRoot", i32), ("flags", u32), ("material", u32), ("boxEps", f32), ("mesh", u32),
                        ("objMaxAbs", f32), ("invNorm", f32), ("pad", u32)])
assert (GpuNode.itemsize, GpuNode4.itemsize, GpuNodeQ.itemsize, GpuTri.itemsize, GpuTriAttr.itemsize, GpuTriTangent.itemsize, GpuInstance.itemsize) == \
    (64, 128, 64, 48, 80, 48, 128)
BVH_EMPTY_CHILD = 0x7fffffff       # unused slot of a 4-wide node
HOST_BUILD_SEPARATE_COLLAPSE = 1   # HRPT_HOST_BUILD_SEPARATE_COLLAPSE


class BvhDump(C.Structure):        # HrptBvhDump
    _fields_ = [("structure", C.c_uint32), ("nodeCount", C.c_uint32), ("node4Count", C.c_uint32), ("triangleCount", C.c_uint32),
                ("instanceCount", C.c_uint32), ("instanceNodeCount", C.c_uint32), ("rootLeaf", C.c_int32), ("hasNodesQ", C.c_uint32),
                ("hasTangents", C.c_uint32), ("maxDepth", C.c_uint32), ("maxDepth4", C.c_uint32), ("maxDepth4Tlas", C.c_uint32),
                ("maxDepth4Blas", C.c_uint32), ("sahCost", C.c_float), ("nodes4Capacity", C.c_uint32), ("nodesQCapacity", C.c_uint32),
                ("nodes", C.c_void_p), ("nodes4", C.c_void_p), ("nodesQ", C.c_void_p), ("triangles", C.c_void_p), ("attributes", C.c_void_p),
                ("tangents", C.c_void_p), ("instances", C.c_void_p)]


ABI_VERSION = 3                    # HRPT_ABI_VERSION (include/hobbyrt_pt.h)
BVH_BUILDER_HOST_SAH, BVH_BUILDER_GPU_LBVH, BVH_BUILDER_GPU_PLOC, BVH_BUILDER_AUTO = 0, 1, 2, 3
BVH_BUILDER_REFITTED = 0x100     # ORed into BuildInfo.usedBuilder after a refit (hrpt_refit_instances)
VERTICES_REFIT, VERTICES_SAME_FRAME = 1, 2            # HRPT_VERTICES_* (hrpt_update_vertices)
ACCEL_AUTO, ACCEL_FLAT, ACCEL_TWO_LEVEL = 0, 1, 2     # HRPT_ACCEL_* (hrpt_set_acceleration_structure)


def default_material():
    """Scene::Material defaults, src/Scene.h:163-178."""
    m = np.zeros((), MaterialConstants)
    m["m_BaseColor"] = (1, 1, 1, 1)
    m["m_EmissiveFactor"] = (0, 0, 0, 1)
    m["m_RoughnessMetallic"] = (1, 0)
    m["m_AlbedoTextureIndex"] = 1       # DEFAULT_TEXTURE_WHITE
    m["m_NormalTextureIndex"] = 3       # DEFAULT_TEXTURE_NORMAL
    m["m_RoughnessMetallicTextureIndex"] = 4  # DEFAULT_TEXTURE_PBR
    m["m_EmissiveTextureIndex"] = 0     # DEFAULT_TEXTURE_BLACK
    m["m_AlphaMode"] = ALPHA_MODE_OPAQUE
    m["m_AlphaCutoff"] = 0.5
    m["m_IOR"] = 1.5
    m["m_AttenuationDistance"] = np.finfo(np.float32).max
    m["m_AttenuationColor"] = (1, 1, 1)
    # MaterialConstantsFromMaterial (src/SceneLoader.cpp:1525-1545): no textures -> sampler = Wrap (1)
    for k in ("m_AlbedoSamplerIndex", "m_NormalSamplerIndex", "m_RoughnessSamplerIndex", "m_EmissiveSamplerIndex"):
        m[k] = 1
    return m


class SceneArrays:
    """Host-side scene in the exact layouts the C ABI (and the oracle) consume. Owns the numpy arrays."""

    def __init__(self, vertices, indices, mesh_data, instances, materials, lights, luts, textures=None):
        self.vertices = np.ascontiguousarray(vertices, VertexQuantized)
        self.indices = np.ascontiguousarray(indices, np.uint32)
        self.mesh_data = np.ascontiguousarray(mesh_data, MeshData)
        self.instances = np.ascontiguousarray(instances, PerInstanceData)
        self.materials = np.ascontiguousarray(materials, MaterialConstants)
        self.lights = np.ascontiguousarray(lights, GPULight)
        self.lut_transmittance, self.lut_scattering, self.lut_irradiance = luts
        self.textures = list(textures or [])   # list of None | uint8 array (h, w, 4) | Texture
        self.sun_direction = None              # filled by scene builders (Scene::GetSunDirection)
        self.sun_angular_size_deg = 0.533

    def desc(self):
        """Returns (SceneDesc, keepalive)."""
        d = SceneDesc()
        keep = [self]

        def ptr(a):
            return a.ctypes.data if a.size else None

        d.vertices, d.vertexCount = ptr(self.vertices), len(self.vertices)
        d.indices, d.indexCount = ptr(self.indices), len(self.indices)
        d.meshData, d.meshDataCount = ptr(self.mesh_data), len(self.mesh_data)
        d.instances, d.instanceCount = ptr(self.instances), len(self.instances)
        d.materials, d.materialCount = ptr(self.materials), len(self.materials)
        d.lights, d.lightCount = ptr(self.lights), len(self.lights)
        n = len(self.textures)
        if n:
            arr = (TextureDesc * n)()
            for i, t in enumerate(self.textures):
                if isinstance(t, Texture):
                    keep.append(t.data)
                    arr[i].texels, arr[i].height, arr[i].width, arr[i].format, arr[i].mipCount = t.data.ctypes.data, t.height, t.width, t.format, t.mip_count
                elif t is not None:
                    t = np.ascontiguousarray(t, np.uint8)
                    keep.append(t)
                    arr[i].texels, arr[i].height, arr[i].width, arr[i].format, arr[i].mipCount = t.ctypes.data, t.shape[0], t.shape[1], 0, 1
            d.textures, d.textureCount = arr, n
            keep.append(arr)
        d.brunetonTransmittance = self.lut_transmittance.ctypes.data
        d.brunetonScattering = self.lut_scattering.ctypes.data
        d.brunetonIrradiance = self.lut_irradiance.ctypes.data if self.lut_irradiance is not None else None
        return d, keep
