/*
 * hobbyrt_pt.h -- C ABI of libhobbyrt_pt.so, the MI355X (gfx950) drop-in for the
 * reference path-tracer pass of lawfuyang/HobbyRenderer.
 *
 * What it replaces (reference file:line, all under /root/reference):
 *   - the GPU work of PathTracerRenderer::Render, src/PathTracerRenderer.cpp:31-106:
 *     writeBuffer(PathTracerCB) + PathTracerInputs binding + dispatch of
 *     PathTracer_CSMain (src/shaders/PathTracer.hlsl:53-340);
 *   - the acceleration structures of Scene::BuildAccelerationStructures,
 *     src/Scene.cpp:67-214 (driver BLAS/TLAS -> library-owned BVH);
 *   - the scene buffer uploads of SceneLoader::CreateAndUploadGpuBuffers /
 *     CreateAndUploadLightBuffer, src/SceneLoader.cpp:2319-2493;
 *   - the Bruneton LUT upload of CommonResources, src/CommonResources.cpp:519-569.
 *
 * Conventions: extern "C", plain pointers and sizes, no exceptions, no torch types.
 * Every call returns HRPT_OK (0) or a negative HrptStatus; the message of the last
 * failure on a context is available from hrpt_last_error(). The reference has no
 * return codes (SDL_assert + log, src/pch.h:77); a reference-side caller asserts on
 * != HRPT_OK. One context = one GPU = one HIP stream; calls on one context must be
 * serialised by the caller, different contexts may be driven from different threads
 * (mirrors: Render runs on a TaskScheduler worker with its own command list,
 * src/RenderGraph.cpp:329-349).
 *
 * All struct layouts are the structured-buffer / cbuffer layouts of the reference
 * shaders (the .sr files under src/shaders); sizes are checked with static asserts below.
 */
#ifndef HOBBYRT_PT_H
#define HOBBYRT_PT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HRPT_ABI_VERSION 3

typedef enum HrptStatus {
    HRPT_OK = 0,
    HRPT_ERR_INVALID_ARGUMENT = -1,   /* null pointer, bad size, index out of range in scene data */
    HRPT_ERR_NO_DEVICE = -2,          /* no HIP device / device ordinal out of range */
    HRPT_ERR_HIP = -3,                /* a HIP runtime call failed; see hrpt_last_error */
    HRPT_ERR_NO_SCENE = -4,           /* render before upload_scene */
    HRPT_ERR_OUT_OF_MEMORY = -5,
    HRPT_ERR_UNSUPPORTED = -6
} HrptStatus;

/* ---- GPU struct layouts (src/shaders/Mesh.sr, Instance.sr, GPULight.sr, Common.sr, PathTracer.sr) ---- */

typedef struct HrptVertexQuantized {       /* Mesh.sr:9-15, 24 B */
    float    m_Pos[3];
    uint32_t m_Normal;                     /* 10:10:10 snorm+511, bit 30 = tangent sign (1 => -1) */
    uint32_t m_Uv;                         /* 2 x fp16 */
    uint32_t m_Tangent;                    /* 8:8 octahedral +127 */
} HrptVertexQuantized;

typedef struct HrptMeshData {              /* Mesh.sr:17-25, 164 B */
    uint32_t m_LODCount;
    uint32_t m_IndexOffsets[8];
    uint32_t m_IndexCounts[8];
    uint32_t m_MeshletOffsets[8];
    uint32_t m_MeshletCounts[8];
    float    m_LODErrors[8];
} HrptMeshData;

typedef struct HrptPerInstanceData {       /* Instance.sr:49-65, 160 B */
    float    m_World[16];                  /* row-major, row-vector convention: p_world = p * M, translation in row 3 */
    float    m_PrevWorld[16];
    uint32_t m_MaterialIndex;
    uint32_t m_MeshDataIndex;
    float    m_Radius;
    uint32_t m_LODIndex;
    float    m_Center[3];
    uint32_t m_FirstGeometryInstanceIndex;
} HrptPerInstanceData;

typedef struct HrptMaterialConstants {     /* Instance.sr:2-46, 180 B */
    float    m_BaseColor[4];
    float    m_EmissiveFactor[4];
    float    m_RoughnessMetallic[2];
    uint32_t m_TextureFlags;
    uint32_t m_AlbedoTextureIndex;
    uint32_t m_NormalTextureIndex;
    uint32_t m_RoughnessMetallicTextureIndex;
    uint32_t m_EmissiveTextureIndex;
    uint32_t m_AlbedoSamplerIndex;
    uint32_t m_NormalSamplerIndex;
    uint32_t m_RoughnessSamplerIndex;
    uint32_t m_EmissiveSamplerIndex;
    uint32_t m_AlbedoMinMipIndex;
    uint32_t m_NormalMinMipIndex;
    uint32_t m_RoughnessMinMipIndex;
    uint32_t m_EmissiveMinMipIndex;
    uint32_t m_AlbedoFeedbackIndex;
    uint32_t m_NormalFeedbackIndex;
    uint32_t m_RoughnessFeedbackIndex;
    uint32_t m_EmissiveFeedbackIndex;
    uint32_t m_MinMipDimsX;
    uint32_t m_MinMipDimsY;
    uint32_t m_AlphaMode;
    float    m_AlphaCutoff;
    float    m_IOR;
    float    m_TransmissionFactor;
    float    m_ThicknessFactor;
    float    m_AttenuationDistance;
    float    m_AttenuationColor[3];
    float    m_SigmaA[3];
    uint32_t m_IsThinSurface;
    float    m_SigmaS[3];
} HrptMaterialConstants;

typedef struct HrptGPULight {              /* GPULight.sr:1-13, 64 B */
    float    m_Position[3];
    float    m_Intensity;
    float    m_Direction[3];
    uint32_t m_Type;                       /* 0 directional, 1 point, 2 spot */
    float    m_Color[3];
    float    m_Range;
    float    m_SpotInnerConeAngle;
    float    m_SpotOuterConeAngle;
    float    m_Radius;
    float    m_CosSunAngularRadius;
} HrptGPULight;

typedef struct HrptPlanarViewConstants {   /* Common.sr:17-43, 704 B */
    float m_MatWorldToView[16];
    float m_MatViewToClip[16];
    float m_MatWorldToClip[16];
    float m_MatClipToView[16];
    float m_MatViewToWorld[16];
    float m_MatClipToWorld[16];
    float m_MatViewToClipNoOffset[16];
    float m_MatWorldToClipNoOffset[16];
    float m_MatClipToViewNoOffset[16];
    float m_MatClipToWorldNoOffset[16];
    float m_ViewportOrigin[2];
    float m_ViewportSize[2];
    float m_ViewportSizeInv[2];
    float m_PixelOffset[2];
    float m_ClipToWindowScale[2];
    float m_ClipToWindowBias[2];
    float m_CameraDirectionOrPosition[4];
} HrptPlanarViewConstants;

/* cbuffer PathTracerConstants, PathTracer.sr:6-17, 768 B (offsets follow HLSL cbuffer
 * packing; the generated srrhi header is not in the reference tree). */
typedef struct HrptPathTracerConstants {
    HrptPlanarViewConstants m_View;        /* @0   */
    float    m_CameraPos[4];               /* @704 */
    uint32_t m_LightCount;                 /* @720 */
    uint32_t m_AccumulationIndex;          /* @724 */
    uint32_t m_FrameIndex;                 /* @728 (written, never read by the shader) */
    uint32_t m_MaxBounces;                 /* @732 */
    float    m_Jitter[2];                  /* @736 */
    float    m_Pad0[2];                    /* @744 (float3 may not straddle a 16-byte row) */
    float    m_SunDirection[3];            /* @752 */
    float    m_CosSunAngularRadius;        /* @764 */
} HrptPathTracerConstants;

/* CommonConsts (Common.sr:47-140) used on this path */
enum {
    HRPT_TEXFLAG_ALBEDO = 1, HRPT_TEXFLAG_NORMAL = 2, HRPT_TEXFLAG_ROUGHNESS_METALLIC = 4, HRPT_TEXFLAG_EMISSIVE = 8,
    HRPT_ALPHA_MODE_OPAQUE = 0, HRPT_ALPHA_MODE_MASK = 1, HRPT_ALPHA_MODE_BLEND = 2,
    HRPT_TRANSMITTANCE_TEXTURE_WIDTH = 256, HRPT_TRANSMITTANCE_TEXTURE_HEIGHT = 64,
    HRPT_SCATTERING_TEXTURE_WIDTH = 256, HRPT_SCATTERING_TEXTURE_HEIGHT = 128, HRPT_SCATTERING_TEXTURE_DEPTH = 32,
    HRPT_IRRADIANCE_TEXTURE_WIDTH = 64, HRPT_IRRADIANCE_TEXTURE_HEIGHT = 16,
    HRPT_LIGHT_DIRECTIONAL = 0, HRPT_LIGHT_POINT = 1, HRPT_LIGHT_SPOT = 2
};

/* A bindless 2D texture. The stb path of the reference produces RGBA8_UNORM with one level (src/TextureLoader.cpp:215-250); its DDS
 * path keeps the file's format and mip chain (:66-135, :196-213): *_SRGB formats are linearised by the sampler BEFORE filtering,
 * BC1-5 / BC7 decode to 8-bit channels, BC6H and the float formats to float channels. The caller hands over DECODED texels
 * (hobbyrt::DecodeImage, include/hobbyrt_scene.h, does the block decompression): */
enum {
    HRPT_TEXTURE_FORMAT_RGBA8_UNORM = 0,   /* 4 bytes per texel */
    HRPT_TEXTURE_FORMAT_RGBA8_SRGB = 1,    /* 4 bytes per texel; r, g, b through the sRGB -> linear table (include/hobbyrt/srgb_table.h), a linear */
    HRPT_TEXTURE_FORMAT_RGBA16_FLOAT = 2,  /* 8 bytes per texel (binary16) */
    HRPT_TEXTURE_FORMAT_RGBA32_FLOAT = 3   /* 16 bytes per texel */
};
#define HRPT_TEXTURE_MAX_MIPS 16
typedef struct HrptTextureDesc {
    const void* texels;                    /* all levels, level 0 first, tightly packed, rows top to bottom; level l is max(1, width >> l) x
                                              max(1, height >> l) texels; NULL for an unused slot */
    uint32_t width, height;
    uint32_t format;                       /* HRPT_TEXTURE_FORMAT_* */
    uint32_t mipCount;                     /* 0 or 1: level 0 only; at most HRPT_TEXTURE_MAX_MIPS. Only the gradient-sampled alpha test of shadow
                                              rays (AlphaTestGrad, RaytracingCommon.hlsli:112-130,207-240) reads levels above 0 */
} HrptTextureDesc;

/* Everything the reference binds to PathTracerInputs (PathTracer.sr:19-32) plus the
 * global bindless tables it reads (src/Renderer.cpp:1834-1841). Host pointers; the
 * library copies during hrpt_upload_scene and the caller keeps ownership. */
typedef struct HrptSceneDesc {
    const HrptVertexQuantized*   vertices;   uint32_t vertexCount;     /* Scene::m_VertexBufferQuantized */
    const uint32_t*              indices;    uint32_t indexCount;      /* Scene::m_IndexBuffer (global vertex indices) */
    const HrptMeshData*          meshData;   uint32_t meshDataCount;   /* Scene::m_MeshData */
    const HrptPerInstanceData*   instances;  uint32_t instanceCount;   /* Scene::m_InstanceData; index == TLAS instanceID */
    const HrptMaterialConstants* materials;  uint32_t materialCount;   /* MaterialConstantsFromMaterial output */
    const HrptGPULight*          lights;     uint32_t lightCount;      /* CreateAndUploadLightBuffer order */
    /* bindless Texture2D table, index = MaterialConstants::m_*TextureIndex. Slots 0..10 are the
     * reference's default textures (Common.sr:103-113); entries with texels == NULL are unbound. */
    const HrptTextureDesc*       textures;   uint32_t textureCount;
    /* Bruneton LUTs in the file format of bin/bruneton/{transmittance,scattering,irradiance}.dat: raw float32 RGBA. The library
     * converts to RGBA16F like CommonResources.cpp:550-558. irradiance may be NULL (not read on this path). */
    const float* brunetonTransmittance;    /* 256*64*4 floats */
    const float* brunetonScattering;       /* 256*128*32*4 floats */
    const float* brunetonIrradiance;       /* 64*16*4 floats or NULL */
} HrptSceneDesc;

typedef struct HrptDeviceDesc {
    int32_t  deviceOrdinal;                /* HIP device index */
    uint32_t abiVersion;                   /* HRPT_ABI_VERSION */
} HrptDeviceDesc;

/* One dispatch of the reference == one accumulation index. `accumCount` > 1 renders
 * indices first..first+accumCount-1 in one call (the "spp" of BASELINE.json); the
 * per-index jitter / accumulation-index fields of `constants` are then recomputed
 * by the library exactly as PathTracerRenderer::Render does (:62,:65). */
typedef struct HrptFrameParams {
    HrptPathTracerConstants constants;     /* as filled by PathTracerRenderer::Render :58-75 for the FIRST index */
    uint32_t accumCount;                   /* >= 1 */
    /* pixel rectangle [x0,x1) x [y0,y1) rendered by this context (image-tile sharding); 0,0,0,0 = full viewport */
    uint32_t tileX0, tileY0, tileX1, tileY1;
    uint32_t flags;                        /* HRPT_FRAME_* */
    /* column interleaving inside the rectangle (multi-GPU load balance): the rectangle is cut into columns of 8 pixels
     * (the reference's thread-group width, PathTracer.hlsl:52) and only the columns k with k % stripeCount == stripeIndex are rendered;
     * every rank then works on all parts of the image. stripeCount 0 or 1 = the whole rectangle. Pixels outside are not touched. */
    uint32_t stripeCount, stripeIndex;
} HrptFrameParams;

enum {
    HRPT_FRAME_DEFAULT = 0,
    HRPT_FRAME_MEGAKERNEL = 1,             /* one-thread-per-pixel restatement kernel (validation path) */
    HRPT_FRAME_WAVEFRONT = 2,              /* persistent wavefront pipeline (default when available) */
    HRPT_FRAME_PROFILE = 4                 /* record HIP events around every kernel launch: fills HrptStats::*KernelMs (adds launch gaps) */
};

typedef struct HrptStats {
    uint64_t closestRays;                  /* TraceRayStandard queries launched */
    uint64_t shadowRays;                   /* CalculateRTShadow queries launched */
    uint64_t paths;                        /* pixel-paths started */
    float    lastRenderMs;                 /* device time of the last hrpt_render (HIP events on the context stream) */
    /* summed device time / launch count per kernel class of the wavefront pipeline since hrpt_reset_stats
     * (HIP events recorded on the context stream around every launch); zero in megakernel mode */
    float    traceKernelMs;                /* wf_extend: closest-hit traversal */
    uint32_t traceKernelLaunches;
    float    shadeKernelMs;                /* wf_shade: attributes, BSDF, NEE sample generation, compaction */
    uint32_t shadeKernelLaunches;
    float    shadowKernelMs;               /* wf_shadow: NEE visibility */
    uint32_t shadowKernelLaunches;
    uint32_t bvhNodeCount;
    uint32_t bvhTriangleCount;
    uint32_t bvhMaxDepth;
    /* ---- ABI 3: queue accounting of the wavefront pipeline (cumulative since hrpt_reset_stats) -------------------------------
     * Bytes each kernel class moves through its queue streams in HBM: records read / written x record size, from counters the
     * kernels keep (paths per bounce, shadow-queue entries, light samples, sampleRadiance updates) and the record layouts of the
     * configuration the LAST hrpt_render used. BVH nodes / triangles / attribute records / textures are not included: they are served
     * by LDS and L2 (rocprofv3 FETCH_SIZE / WRITE_SIZE give the HBM total). Zero in megakernel mode. */
    uint32_t megakernelFallbacks;          /* hrpt_render calls that asked for the wavefront pipeline but ran the validation megakernel */
    float    raygenKernelMs;               /* wf_raygen (HRPT_FRAME_PROFILE) */
    uint32_t raygenKernelLaunches;
    float    resolveKernelMs;              /* wf_resolve (HRPT_FRAME_PROFILE) */
    uint32_t resolveKernelLaunches;
    uint32_t pad0;
    uint64_t raygenQueueBytes;
    uint64_t traceQueueBytes;              /* ray records read + hit records written */
    uint64_t shadeQueueBytes;              /* path + hit records read, surviving paths + shadow-queue entries written, sampleRadiance updates */
    uint64_t shadowQueueBytes;             /* shadow-queue entries + light samples read, sampleRadiance updates (+ shadow-ray queue in the any-hit schedule) */
    uint64_t resolveQueueBytes;            /* sampleRadiance read, Accumulation read / written, Output written */
    uint64_t neeEntries;                   /* path vertices with at least one light sample */
    uint64_t neeSamples;                   /* light samples drawn (>= shadowRays: a sample below the horizon traces no ray) */
    uint64_t queuePoolBytes;               /* size of the context's queue pool in HBM */
} HrptStats;

typedef struct HrptContext HrptContext;

int  hrpt_create(const HrptDeviceDesc* desc, HrptContext** out);
void hrpt_destroy(HrptContext* ctx);
const char* hrpt_last_error(const HrptContext* ctx);      /* ctx may be NULL: last creation error */

/* Replaces scene buffer upload + BLAS/TLAS build. Validates every index in the scene data.
 * Size limit: one acceleration structure holds fewer than 2^32 / 48 (89 M) triangle records -- world-space triangles (instances x mesh triangles)
 * for the flat structure, distinct mesh triangles for the two-level one (hrpt_set_acceleration_structure) -- and fewer than 2^25 tree nodes,
 * because the traversal kernels address both arrays by 32-bit byte offsets; larger scenes fail with HRPT_ERR_INVALID_ARGUMENT. */
int  hrpt_upload_scene(HrptContext* ctx, const HrptSceneDesc* scene);

/* (Re)allocates the RGBA32F Accumulation (u1) and Output (u0) images, PathTracerRenderer::Setup :14-29. */
int  hrpt_resize(HrptContext* ctx, uint32_t width, uint32_t height);

/* The dispatch. Asynchronous on the context stream. */
int  hrpt_render(HrptContext* ctx, const HrptFrameParams* params);
int  hrpt_synchronize(HrptContext* ctx);
/* Run all further work of the context on the caller's HIP stream (the counterpart of recording into the caller's
 * command list, src/RenderGraph.cpp:329-349; also lets an RCCL all-gather follow the render without a host sync).
 * useCallerStream != 0: hipStream is used as is (NULL = the legacy default stream); 0: back to the context's own
 * stream. The previous stream is drained first. */
int  hrpt_set_stream(HrptContext* ctx, void* hipStream, int useCallerStream);

/* Device pointers of the two images (width*height float4, row-major) for zero-copy consumers
 * (the HDR post chain, RCCL all-gather). */
int  hrpt_get_device_images(HrptContext* ctx, void** accumulation, void** output);
/* ---- acceleration-structure builder --------------------------------------------------------------
 * Scene::BuildAccelerationStructures (src/Scene.cpp:67-214) is a driver BLAS/TLAS build in the reference. Here
 * hrpt_upload_scene builds the library's own structure either on the host (binned SAH on up to 16 host threads: the best tree, ~0.25 s per million
 * triangles) or on the GPU (Morton-order LBVH or PLOC clustering: milliseconds). Radiance is identical either way (the hit
 * definition is BVH-independent). The GPU builders fall back to the host one for scenes under 8 triangles or when their
 * tree is deeper than the traversal stacks allow. The default, HRPT_BVH_BUILDER_AUTO, takes the host builder below 65 536
 * triangles and PLOC above (measured on MI355X: same frame time as the SAH tree at 101 k and 1.17 M triangles, 2 ms / 5 ms
 * instead of 32 ms / 548 ms of build time; on small scenes the SAH tree still renders up to 20 % faster). */
#define HRPT_BVH_BUILDER_HOST_SAH 0
#define HRPT_BVH_BUILDER_GPU_LBVH 1      /* Morton radix tree (Karras 2012): fastest build */
#define HRPT_BVH_BUILDER_GPU_PLOC 2      /* Morton order + nearest-neighbour clustering (PLOC): better tree, a few times the LBVH build time;
                                            falls back to the LBVH hierarchy when its tree is too deep for the traversal stacks */
#define HRPT_BVH_BUILDER_AUTO     3      /* default: HOST_SAH below 65 536 triangles, GPU_PLOC from there on */
#define HRPT_BVH_BUILDER_REFITTED 0x100u /* ORed into HrptBuildInfo::usedBuilder when the last hrpt_refit_instances kept the hierarchy of an earlier GPU build */
int  hrpt_set_bvh_builder(HrptContext* ctx, int builder);       /* takes effect at the next hrpt_upload_scene / hrpt_update_instances */
typedef struct HrptBuildInfo {
    uint32_t requestedBuilder, usedBuilder;     /* HRPT_BVH_BUILDER_* */
    float    buildMs;                           /* host wall time of the last build inside hrpt_upload_scene / hrpt_update_instances (copies included) */
    float    deviceBuildMs;                     /* GPU builder: device time, instance-table copy to last kernel; else 0 */
    uint32_t triangleCount, nodeCount, node4Count, maxDepth, maxDepth4;
    uint32_t mortonBits;                        /* GPU builder: Morton bits of the hierarchy (63 unless the full-code tree was too deep) */
    float    sahCost;                           /* surface-area-heuristic cost of the 2-wide tree: 1 + sum(area(child) * (inner ? 1 : triangles)) / area(root) */
    uint32_t structure;                         /* HRPT_ACCEL_FLAT or HRPT_ACCEL_TWO_LEVEL: what the last build produced */
    uint32_t instanceNodeCount;                 /* two-level: 4-wide nodes of the tree over the instances (node4Count counts those + the mesh trees) */
    uint32_t distinctMeshes;                    /* two-level: meshes with a tree of their own (triangleCount counts THEIR triangles, not instances x triangles) */
    uint32_t leafAreaPermille;                  /* flat structure: surface area of the leaf boxes in the 64-byte quantised nodes / in the fp32 nodes, x 1000 (0: no tree) */
    uint32_t nodeFormat;                        /* what the wavefront kernels walk when the tree is in global memory: 1 = 128-byte fp32 nodes, 2 = 64-byte quantised nodes
                                                   (four instead of seven 16-byte requests per lane and step; chosen when leafAreaPermille <= 1100; HRPT_BVH_NODE_FORMAT=1|2 forces) */
} HrptBuildInfo;                                /* 64 B */
int  hrpt_get_build_info(HrptContext* ctx, HrptBuildInfo* out);

/* Shape of the acceleration structure. The reference builds one BLAS per mesh and a TLAS over the instances (src/Scene.cpp:98-154).
 * HRPT_ACCEL_FLAT (what AUTO picks for all but heavily instanced scenes) transforms every instance's triangles to world space once
 * and builds ONE tree: no ray transform, one tree walk -- the fastest traversal while the tree stays cache-resident, but memory and build
 * time grow with instances x triangles (~600 B per world triangle with the GPU builders' buffers). HRPT_ACCEL_TWO_LEVEL keeps one
 * object-space tree per distinct mesh plus a tree over the instances: memory grows with distinct triangles + instances, hrpt_update_instances rebuilds only the small instance tree (the
 * reference's per-frame TLAS build), traversal pays a ray transform per visited instance. Radiance is identical: hits are still
 * decided in world space on the world-space vertices the flat upload would produce, non-opaque instances (MASK / BLEND / transmissive
 * materials) included: their candidates are visited in the same front-to-back order. Every render / query entry point traverses it: the wavefront
 * pipeline, the validation megakernel (HRPT_FRAME_MEGAKERNEL) and both ray-query kernels (the last two with a private 64-entry stack: deeper
 * structures answer HRPT_ERR_INVALID_ARGUMENT there); hrpt_selftest_bvh is a flat-structure check and answers HRPT_ERR_INVALID_ARGUMENT
 * on such a scene. A scene that cannot be held
 * in this form (an instance whose world matrix has no inverse, now or after a later hrpt_update_instances) is built flat whatever was
 * asked -- HrptBuildInfo::structure tells. AUTO: two-level when the scene has at least 2 M world triangles (16 M if any instance is non-opaque: measured cross-over) and at least 8
 * instances per distinct mesh on average (measured on MI355X, opaque spheres / cylinders of ~400 triangles, 1920x1080, 8 spp, 4 bounces:
 * 4 096 instances 19.3 ms flat vs 16.2 ms two-level, 16 384: 27.7 vs 17.3 ms, 65 536: 44.4 vs 18.4 ms and 17.6 GB vs 30 MB -- the small trees stay in cache).
 * Takes effect at the next hrpt_upload_scene. */
#define HRPT_ACCEL_AUTO      0
#define HRPT_ACCEL_FLAT      1
#define HRPT_ACCEL_TWO_LEVEL 2
int  hrpt_set_acceleration_structure(HrptContext* ctx, int structure);

/* Moving objects: writes instances[0..count) over the scene's instances [firstInstance, firstInstance + count) -- the closed dirty range
 * Renderer::UploadDirtyInstanceTransforms copies into m_InstanceDataBuffer / m_RTInstanceDescBuffer (src/Renderer.cpp:924-967, fed by
 * Scene::Update, src/Scene.cpp:536-556) -- and rebuilds the acceleration structure, the job of TLASRenderer's per-frame
 * buildTopLevelAccelStructFromBuffer (src/CommonRenderers.cpp:234-246). Only m_World, m_PrevWorld (read by hrpt_render_motion_vectors alone) and the unused m_Center / m_Radius
 * may differ from the uploaded instance; a changed mesh, material or LOD index is HRPT_ERR_INVALID_ARGUMENT. With a GPU builder selected
 * the geometry and all build buffers are already on the device: the call uploads count-independent O(instances) data and runs the build
 * kernels (hrpt_get_build_info reports the rebuild); with the host builder the tree is rebuilt on the host from the library's copy of
 * the scene. Waits for frames in flight, returns when the new tree is in place. The accumulation image is not touched: like
 * PathTracerRenderer::Render's reset on a changed view matrix (src/PathTracerRenderer.cpp:41-50), restarting accumulation
 * (firstAccumulationIndex = 0) is the caller's decision. If the rebuild fails the scene is unusable until hrpt_upload_scene. */
int  hrpt_update_instances(HrptContext* ctx, const HrptPerInstanceData* instances, uint32_t firstInstance, uint32_t count);
/* The same call for SMALL motions: where a GPU builder holds the hierarchy of the previous build (flat structure built by LBVH / PLOC; the
 * instance tree of a two-level structure from 1 024 instances on) the boxes are recomputed bottom-up on that hierarchy instead of the tree
 * being rebuilt -- the refit of a driver's acceleration-structure update (the reference always rebuilds its TLAS,
 * src/CommonRenderers.cpp:234-246; its BLASes are static). No sort and no hierarchy construction: a PLOC tree is refitted in a fraction of its
 * build time and keeps its topology, so its quality follows the motion (large moves: call hrpt_update_instances). Radiance is the same
 * either way (the hit definition does not depend on the tree). Everywhere else (host-built trees, the first call after an upload with the
 * host builder) it IS hrpt_update_instances. HrptBuildInfo::usedBuilder carries HRPT_BVH_BUILDER_REFITTED when the hierarchy was kept. */
int  hrpt_refit_instances(HrptContext* ctx, const HrptPerInstanceData* instances, uint32_t firstInstance, uint32_t count);
/* The other two per-frame uploads of the reference's main loop (src/Renderer.cpp:500-507):
 * hrpt_update_lights replaces the whole light buffer, like SceneLoader::CreateAndUploadLightBuffer when Scene::m_LightsDirty is set
 * (count may differ from the uploaded scene's; at least one light; HrptPathTracerConstants::m_LightCount of later frames must not
 * exceed it). hrpt_update_materials writes materials[0..count) over the material constants [firstMaterial, firstMaterial + count),
 * the closed dirty range of Renderer::UploadDirtyMaterialConstants (src/Renderer.cpp:976-1025; emissive animations mark it,
 * src/Scene.cpp:440-470). Texture indices keep referring to the uploaded texture table. A material that switches between OPAQUE and
 * MASK / BLEND, or the first material with a normal map, changes what the acceleration structure caches per triangle: the call then
 * rebuilds it (as hrpt_update_instances would); anything else is a buffer write. Both wait for frames in flight. */
int  hrpt_update_lights(HrptContext* ctx, const HrptGPULight* lights, uint32_t count);
int  hrpt_update_materials(HrptContext* ctx, const HrptMaterialConstants* materials, uint32_t firstMaterial, uint32_t count);

/* Deforming meshes (skinning, cloth, morph targets, simulation output, an editor dragging a vertex): writes vertices[0..count) over the
 * vertices [firstVertex, firstVertex + count) of the scene's vertex buffer -- which is global, shared by all meshes -- and brings the
 * acceleration structure and every per-triangle record after them. Indices, meshes, instances, materials and the vertex count stay.
 * Contract (that of hrpt_update_instances): after the call every product of the context -- hrpt_render on both kernel paths,
 * hrpt_trace_rays, hrpt_render_gbuffer, hrpt_selftest_read_bvh -- is bit-identical to that of a context which uploaded a scene built with
 * the new vertices. Synchronous: waits for frames in flight, returns when the new structure is in place.
 *   flat structure held by a GPU builder: the builder's device vertex buffer is patched in place and its build kernels run; with
 *     HRPT_VERTICES_REFIT the hierarchy of the previous build is kept where there is one (as hrpt_refit_instances; HrptBuildInfo::usedBuilder
 *     then carries HRPT_BVH_BUILDER_REFITTED). No allocation, no index, texture or material traffic.
 *   flat structure of the host builder: rebuilt on the host from the library's copy of the scene (HRPT_VERTICES_REFIT means rebuild).
 *   two-level structure: the whole structure, mesh trees included, is rebuilt from the library's copy as at an upload.
 * hrpt_update_vertices takes quantised vertices in host memory. hrpt_update_vertices_device takes float vertices in DEVICE memory
 * (HrptVertexFloat, what a skinning or simulation kernel writes -- hrpt_skin_vertices_device below is one, and
 * hrpt_update_vertices_skinned runs it in front of the quantiser in one call; 16-byte aligned), synchronises `stream` (NULL = the default stream)
 * before it reads them, quantises them on the device by the arithmetic of hrpt_quantize_vertices_host and copies the quantised range
 * back into the library's host copy (24 bytes per vertex over PCIe), which the host builder, the two-level build, later
 * hrpt_update_instances / hrpt_update_materials calls and hrpt_selftest_* read.
 * Atomic on bad input: a position that is not finite (found on the host, or by the quantising kernel before anything is committed), a
 * NULL array with count > 0, a range beyond the vertex count, unknown flag bits: HRPT_ERR_INVALID_ARGUMENT, and the scene renders
 * exactly as before the call. No scene: what hrpt_update_instances answers there. If the rebuild itself fails the scene is unusable
 * until hrpt_upload_scene.
 * Previous positions (what hrpt_render_motion_vectors forms the previous world position from): the context keeps, per vertex, the
 * object-space position of the previous frame. A call WITHOUT HRPT_VERTICES_SAME_FRAME first sets previous = current for all vertices
 * (what lies outside the range did not deform this frame), then records the old positions of its range as previous and installs the new
 * ones; a call WITH the flag skips the reset (a second range updated in the same frame). count == 0 is HRPT_OK and builds nothing;
 * without the flag it still resets, so hrpt_update_vertices(ctx, NULL, 0, 0, 0) ends a deformation. A context that never calls this has
 * previous == current. */
typedef struct HrptVertexFloat {           /* 48 B */
    float pos[3]; float normal[3]; float uv[2]; float tangent[4];      /* tangent[3] = handedness sign */
} HrptVertexFloat;
enum { HRPT_VERTICES_REFIT = 1, HRPT_VERTICES_SAME_FRAME = 2 };
int  hrpt_update_vertices(HrptContext* ctx, const HrptVertexQuantized* vertices, uint32_t firstVertex, uint32_t count, uint32_t flags);
int  hrpt_update_vertices_device(HrptContext* ctx, const HrptVertexFloat* deviceVertices, uint32_t firstVertex, uint32_t count,
                                 uint32_t flags, void* stream);
/* The quantiser alone (csrc/pt_deform.h): QuantizeVertex of the scene format (10:10:10 snorm normal + tangent sign, 2 x fp16 uv, 8:8
 * octahedral tangent), bit-identical on host threads (needs no GPU; nthreads <= 0: one per hardware thread, at most 16) and in the
 * gfx950 kernel (asynchronous on `stream`; deviceIn 16-byte aligned, deviceOut 4-byte aligned, not overlapping). A NaN normal component,
 * and the NaN an infinite tangent divides to, count as 0. Positions are copied as they are. NULL pointers with count > 0:
 * HRPT_ERR_INVALID_ARGUMENT. */
int  hrpt_quantize_vertices_host(const HrptVertexFloat* in, uint32_t count, HrptVertexQuantized* out, int nthreads);
int  hrpt_quantize_vertices_device(HrptContext* ctx, const HrptVertexFloat* deviceIn, uint32_t count, HrptVertexQuantized* deviceOut, void* stream);

/* The producer in front of the quantiser (csrc/pt_skin.h has the definition, DESIGN.md section 22 the prose): morph targets, then
 * linear-blend skinning with four joints per vertex, then unit normal and tangent, from a bind pose to HrptVertexFloat records with the
 * conventions the quantiser expects (tangent[3] = handedness sign, flipped by a mirroring joint; unit normals). float32, one rounding per
 * operation, bit-identical on host threads, in the gfx950 kernels and in tests/skin_reference.py. The reference renderer has no skinning:
 * parity unpinned by the reference.
 *   morph   for k < targetCount in order, w = morphWeights[k]: skipped when w == 0 (+0 or -0), else pos / normal / tangent += w * delta
 *   skin    (joints != NULL) B = ((w0 M0 + w1 M1) + w2 M2) + w3 M3 with Mj = jointMatrices[joints[4i + j]], a row-major 3 x 4 with
 *           p' = M [p; 1] (for glTF: the top three rows of globalJoint * inverseBind, pre-multiplied by the inverse of the mesh node's world
 *           transform for object space). Weights are used as given. Position by B, tangent by its 3 x 3 part, normal by the cofactor
 *           matrix of that part; a negative determinant negates the normal and tangent[3].
 *   unit    normal and tangent are divided by their length where its square is positive and finite, and left as they are otherwise.
 * A joint index >= jointCount, and an output position that is not finite, are errors of the input: _host returns
 * HRPT_ERR_INVALID_ARGUMENT for the first and leaves `out` untouched (the second it writes like any other value, as the quantiser copies
 * one); the kernels stay inside the palette (they read joint jointCount - 1) and raise a word of their status array: word 0 "output
 * position not finite", word 1 "joint index out of range".
 * hrpt_skin_vertices_device is asynchronous on `stream`; deviceOut is 16-byte aligned and does not overlap base; deviceStatus2 is two
 * words the caller zeroed, or NULL. hrpt_update_vertices_skinned is hrpt_update_vertices_device with the skinning kernel in front of the
 * quantiser, both on the context's stream: the caller parks no float vertices (the context holds them, 48 bytes per vertex of the scene,
 * allocated at first use) and there is one call and one wait on `stream` instead of two. Same checks (count = args->count), same
 * synchronisation, same previous-position protocol, same flags; either status word set is HRPT_ERR_INVALID_ARGUMENT and the scene renders
 * exactly as before.
 * All three: NULL args, non-zero reserved, a misaligned pointer, a NULL base with count > 0, joints without weights or jointMatrices or
 * with jointCount == 0, targetCount > 0 with NULL deltas or morphWeights: HRPT_ERR_INVALID_ARGUMENT. count == 0 is HRPT_OK (in the update
 * call it rolls the previous positions as hrpt_update_vertices_device does).
 * A palette of at most HRPT_SKIN_LDS_MAX_JOINTS joints is served from LDS, a larger one gathered from global memory: same bits. */
#define HRPT_SKIN_LDS_MAX_JOINTS 256
typedef struct HrptSkinMorphDelta { float pos[3]; float normal[3]; float tangent[3]; } HrptSkinMorphDelta;   /* 36 B */
typedef struct HrptSkinArgs {
    const HrptVertexFloat*    base;           /* count records, the bind pose; 16-byte aligned */
    const uint16_t*           joints;         /* count x 4, 8-byte aligned; NULL: no skinning (weights, jointMatrices, jointCount ignored) */
    const float*              weights;        /* count x 4, 16-byte aligned */
    const float*              jointMatrices;  /* jointCount x 12 (row-major 3x4, p' = M [p;1]); 16-byte aligned */
    const HrptSkinMorphDelta* deltas;         /* targetCount x count, target-major; NULL iff targetCount == 0 */
    const float*              morphWeights;   /* targetCount */
    uint32_t count, jointCount, targetCount, reserved /* 0 */;
} HrptSkinArgs;   /* every pointer: host memory for _host, device memory for the other two */
int  hrpt_skin_vertices_host(const HrptSkinArgs* args, HrptVertexFloat* out, int nthreads);
int  hrpt_skin_vertices_device(HrptContext* ctx, const HrptSkinArgs* args, HrptVertexFloat* deviceOut, uint32_t* deviceStatus2, void* stream);
int  hrpt_update_vertices_skinned(HrptContext* ctx, const HrptSkinArgs* args, uint32_t firstVertex, uint32_t flags, void* stream);

/* ---- keyframe animation and node hierarchies (csrc/pt_anim.h has the definition, DESIGN.md section 23 the prose) -----------------
 * The producer at the head of a moving frame: animation times -> node poses -> instance matrices + joint palette + morph weights, what
 * Scene::Update and EvaluateAnimSampler do on the host in the reference (src/Scene.cpp:345-570; composed set and order: :220-273).
 * float32, one rounding per operation, bit-identical on host threads (hrpt_animate_host), in the gfx950 kernels (hrpt_animate) and in
 * tests/anim_reference.py. Slerp uses this project's own sine and arctangent: parity with DirectXMath's approximations is unpinned.
 *   clock     per animation: current += dt; duration > 0: current = fmodf(current, duration); duration = the largest last key time of
 *             the animation's samplers. Host side (hrpt_animation_advance / _set_times); the evaluation gets one time per animation.
 *   sampler   keys [firstKey, firstKey + keyCount): one time and one float4 each. No keys: its channels do nothing. One key: that value.
 *             t <= first: the first value, t >= last: the last; else k0 = the last i <= n - 2 with t >= time[i], k1 = k0 + 1,
 *             d = time[k1] - time[k0], alpha = d > 0 ? (t - time[k0]) / d : 0, and
 *               STEP v0 | LINEAR, CUBICSPLINE v0 + alpha (v1 - v0) | CATMULLROM over v[k0-1], v0, v1, v[k1+1] with clamped neighbours |
 *               SLERP of the normalised keys, the second negated when their dot product is negative, linear above a dot of 0.9995
 *   channel   path TRANSLATION / SCALE: xyz of the value; ROTATION: the value normalised; WEIGHTS: .x, into the morph-weight slots its
 *             targets name (the reference drops weight channels: defined here). targets[firstTarget .. + targetCount) are node indices,
 *             or weight slots for WEIGHTS. Channels apply ordered by (animation of their sampler, channel index); the last writer of a
 *             (node, path) or of a slot wins. A path no channel writes keeps the node's base value, a slot nothing writes is 0.
 *   pose      local = scale . rotation . translation (row vectors, translation in row 3); world = local . world(parent), a full 4 x 4
 *             product, each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3; a root's world is its local. Composed: every node a channel with keys
 *             targets, and all their descendants. Every other node keeps baseWorld.
 *   instances m_PrevWorld = m_World for EVERY instance, then m_World = world(node) for the instances listed under composed nodes
 *             (nodeInstances[firstInstance .. + instanceCount)); every other field stays.
 *   joints    palette[j] = the top three rows of transpose(inverseBind[j] . world(node[j])): the row-major 3 x 4 with p' = M [p; 1] of
 *             HrptSkinArgs::jointMatrices. The instance of a skinned mesh is expected to carry an identity world.
 * hrpt_animation_create validates and copies everything (context-free): an index out of range (parent, node, sampler, animation, weight
 * slot, a target or instance range beyond its array), a parent cycle, an instance listed twice, key times that decrease or are not finite,
 * keys beyond the arrays, an unknown path or interpolation, a NULL array with a non-zero count, a non-zero reserved word:
 * HRPT_ERR_INVALID_ARGUMENT and *out = NULL. All times start at 0.
 * hrpt_animate_host: the evaluation on host threads (no GPU; nthreads as in hrpt_skin_vertices_host). Every output may be NULL.
 * instancesInOut holds instanceCount records; with prevInstances != NULL these are first copied from there. instanceCount not above every
 * listed instance index (with instancesInOut != NULL): HRPT_ERR_INVALID_ARGUMENT, nothing written. paletteOut: jointCount x 12 floats,
 * weightsOut: morphWeightCount floats, nodeWorldsOut: nodeCount x 16 floats.
 * hrpt_animate: the same on the device, on the context's stream. The tables are uploaded at the first call for this (context, animation)
 * and kept until hrpt_animation_release / hrpt_destroy (destroy the animation only after that). Without HRPT_ANIMATE_NO_COMMIT it then
 * commits like hrpt_update_instances (hrpt_refit_instances with HRPT_ANIMATE_REFIT): the closed range of the listed instances is evaluated
 * in a device copy of those records, read back into the library's host copy, the m_PrevWorld roll of the instances outside it is done on
 * the host, and the acceleration structure is rebuilt; an animation that lists no instance under a composed node commits and builds
 * nothing. No scene, or an instance index beyond the scene's: what hrpt_update_instances answers, nothing changed. With
 * HRPT_ANIMATE_NO_COMMIT the call is asynchronous, needs no scene, evaluates node worlds, palette and weights only and leaves the scene's
 * instances alone (a scene that animates joints and no instances: follow with hrpt_update_vertices_skinned on the same stream).
 * hrpt_get_animation_device: device pointers of the palette (jointCount x 12 floats), the weights and the node worlds of the last
 * hrpt_animate, each at least 256-byte aligned -- palette and weights go straight into HrptSkinArgs::jointMatrices / ::morphWeights; valid
 * until the animation is released from the context; an array of zero length gives NULL. hrpt_read_animation copies them to the host
 * (synchronises; any pointer may be NULL). Before the first hrpt_animate of the pair both answer HRPT_ERR_INVALID_ARGUMENT.
 * Not here: the reference's emissive-intensity channels (hrpt_update_materials takes their result), light nodes, bounding spheres. */
enum { HRPT_ANIM_PATH_TRANSLATION = 0, HRPT_ANIM_PATH_ROTATION = 1, HRPT_ANIM_PATH_SCALE = 2, HRPT_ANIM_PATH_WEIGHTS = 3 };
enum { HRPT_ANIM_STEP = 0, HRPT_ANIM_LINEAR = 1, HRPT_ANIM_CUBICSPLINE = 2, HRPT_ANIM_CATMULLROM = 3, HRPT_ANIM_SLERP = 4 };
enum { HRPT_ANIMATE_REFIT = 1, HRPT_ANIMATE_NO_COMMIT = 2 };
#define HRPT_ANIM_LDS_MAX_ANIMATIONS 256       /* up to this many animation times are staged in LDS by the sampling kernel */
typedef struct HrptAnimSampler { uint32_t interpolation, firstKey, keyCount, animation; } HrptAnimSampler;             /* 16 B */
typedef struct HrptAnimChannel { uint32_t path, sampler, firstTarget, targetCount; } HrptAnimChannel;                  /* 16 B */
typedef struct HrptAnimNode {                  /* 116 B */
    int32_t  parent;                           /* -1: a root */
    float    translation[3], rotation[4] /* x, y, z, w */, scale[3];
    float    baseWorld[16];                    /* row-major, row vectors: what the node's instances were uploaded with */
    uint32_t firstInstance, instanceCount;     /* into nodeInstances */
} HrptAnimNode;
typedef struct HrptAnimJoint { uint32_t node; float inverseBind[16]; } HrptAnimJoint;                                   /* 68 B */
typedef struct HrptAnimationDesc {
    const HrptAnimSampler* samplers;
    const HrptAnimChannel* channels;
    const HrptAnimNode*    nodes;
    const HrptAnimJoint*   joints;
    const float*           keyTimes;           /* keyCount */
    const float*           keyValues;          /* keyCount x 4 */
    const uint32_t*        targets;            /* targetCount */
    const uint32_t*        nodeInstances;      /* nodeInstanceCount scene instance indices */
    uint32_t samplerCount, channelCount, nodeCount, jointCount, keyCount, targetCount, nodeInstanceCount, animationCount, morphWeightCount, reserved /* 0 */;
} HrptAnimationDesc;                           /* 104 B */
typedef struct HrptAnimation HrptAnimation;
int  hrpt_animation_create(const HrptAnimationDesc* desc, HrptAnimation** out);
void hrpt_animation_destroy(HrptAnimation* anim);
int  hrpt_animation_advance(HrptAnimation* anim, float dt);
int  hrpt_animation_set_times(HrptAnimation* anim, const float* times, uint32_t count);       /* count == animationCount; taken as given, not wrapped */
int  hrpt_animation_get_times(const HrptAnimation* anim, float* times, float* durations, uint32_t count);   /* either array may be NULL */
int  hrpt_animate_host(const HrptAnimation* anim, const HrptPerInstanceData* prevInstances, HrptPerInstanceData* instancesInOut, uint32_t instanceCount,
                       float* paletteOut, float* weightsOut, float* nodeWorldsOut, int nthreads);
int  hrpt_animate(HrptContext* ctx, const HrptAnimation* anim, uint32_t flags);
int  hrpt_get_animation_device(HrptContext* ctx, const HrptAnimation* anim, void** palette, void** weights, void** nodeWorlds);
int  hrpt_read_animation(HrptContext* ctx, const HrptAnimation* anim, float* palette, float* weights, float* nodeWorlds);
int  hrpt_animation_release(HrptContext* ctx, const HrptAnimation* anim);

/* ---- in-process multi-GPU: one context per GPU inside ONE process ------------------------------------
 * Rank i of n has rendered the row band [i*H/n, (i+1)*H/n) of its accumulation image (HrptFrameParams::tile*; H must be a
 * multiple of n, every context the same size). hrpt_allgather sends every band to every other context with
 * hipMemcpyPeerAsync (xGMI between GPUs, a plain device copy when two contexts share a GPU), orders the copies against each
 * context's stream with events, and resolves Output = rgb / a on every context. Asynchronous: follow with hrpt_synchronize on
 * the contexts that are read. The one-process-per-GPU form of the same exchange (torch.distributed / RCCL) is
 * hobbyrenderer_amd/distributed.py. */
int  hrpt_allgather(HrptContext* const* ranks, int n);

/* ---- stand-alone ray queries ("other inline-RT consumers") ------------------------------------------
 * The two queries every inline-ray-tracing pass of the reference is built from, over the uploaded scene:
 *   HRPT_RAYS_CLOSEST  TraceRayStandard (src/shaders/RaytracingCommon.hlsli:138-198): closest hit, MASK candidates alpha-tested,
 *                      BLEND candidates committed stochastically from the ray's own RNG state (returned advanced in HrptRayHit::rng)
 *   HRPT_RAYS_SHADOW   CalculateRTShadow<true> (src/shaders/CommonLighting.hlsli:380-496): origin = shaded point, direction = L,
 *                      tmax = distance to the light; the visibility in [0, 1] comes back in HrptRayHit::t (tmin is ignored:
 *                      the query applies its own 0.01 bias)
 * A ray with a NaN or infinite origin or direction component is a miss (hit == 0, visibility 1) and is not traced. Finite rays are expected
 * to keep direction components below about 1e20 and tmax * |direction| below 1e29 (what the far-away boxes of unused node slots allow).
 * rays / hits are host arrays unless HRPT_RAYS_DEVICE_POINTERS is set (then both are device pointers and the call is asynchronous
 * on the context stream). */
typedef struct HrptRay    { float origin[3]; float tmin; float direction[3]; float tmax; uint32_t rng; uint32_t pad[3]; } HrptRay;       /* 48 B */
typedef struct HrptRayHit { float t, u, v; uint32_t instance, primitive, hit, rng, pad; } HrptRayHit;                                  /* 32 B */
#define HRPT_RAYS_CLOSEST 0u
#define HRPT_RAYS_SHADOW  1u
#define HRPT_RAYS_DEVICE_POINTERS 0x100u
#define HRPT_RAYS_THREAD_PER_RAY  0x200u   /* testing: the one-thread-per-ray kernel instead of the persistent refilling traversal kernel (same results) */
int  hrpt_trace_rays(HrptContext* ctx, const HrptRay* rays, HrptRayHit* hits, uint64_t count, uint32_t flags);

/* ---- path-traced radiance for arbitrary ray batches -----------------------------------------------------------------
 * The radiance that arrives along rays the caller made (probes, cube maps, panoramas, other sensor models, lightmap texels, ray-sampled
 * training sets): the estimator of hrpt_render on rays that do not come from its pinhole camera.
 * Ray i is path segment 0 of PathTracer_CSMain (src/shaders/PathTracer.hlsl:53-340) with ray.o = rays[i].origin, ray.d = rays[i].direction
 * AS GIVEN (the library does not normalise it: pass a unit vector, which keeps camera rays bit-identical to the render's), ray.tmin =
 * rays[i].tmin, the RNG state rays[i].rng, throughput 1, outside any medium. rays[i].tmax is IGNORED: the first segment is unbounded at 1e10
 * as in the reference. From there it is the render's loop with no change of arithmetic or order: constants->m_MaxBounces bounces, next event
 * estimation over the first constants->m_LightCount lights, the sun disk on a bounce-0 miss, specular direct light at bounce 0 only, Russian
 * roulette from bounce 2, the g_Lights[0] sun-intensity quirk. Of `constants` only m_SunDirection, m_CosSunAngularRadius, m_LightCount and
 * m_MaxBounces are read; the view, the jitter, the camera position and the accumulation index are not. For the origin, direction and
 * seed of PathTracer.hlsl:61-72 the result is, bit for bit, the term hrpt_render adds to Accumulation for that pixel and index.
 * radiance4 receives one float4 per ray: (L.r, L.g, L.b, 1); with HRPT_RADIANCE_ACCUMULATE (old.rgb + L, old.w + 1), the addition the
 * render performs for an accumulation index above 0. A ray with a NaN or infinite origin, direction or tmin is not traced (the rule of
 * hrpt_trace_rays): it writes (0, 0, 0, 0), and with HRPT_RADIANCE_ACCUMULATE leaves its slot alone.
 * rays / radiance4 are host arrays (the call synchronises) unless HRPT_RADIANCE_DEVICE_POINTERS is set: then both are device pointers, 16-byte
 * aligned, nothing is copied and the call is asynchronous on the context stream. Either way it is ordered on that stream with renders and
 * scene updates. hrpt_resize is not required. Accumulation, Output, every G-buffer plane and every history, the exposure buffer and every
 * HrptStats field (megakernelFallbacks included) stay as they were.
 * HRPT_RADIANCE_SECONDARY: ray i is path segment 1, a ray that leaves a first hit somebody else has lit (hrpt_indirect_lighting). The bounce
 * loop runs bounce = 1 .. m_MaxBounces - 1 and everything that depends on the bounce index takes the true index: no sun disk at a miss, no
 * specular direct light, roulette from index 2. With m_MaxBounces <= 1 nothing is traced and a finite ray stores (0, 0, 0, 1). The record,
 * the batching, the other flags, the non-finite rule and the errors are the same.
 * count == 0: HRPT_OK, nothing happens. No scene: HRPT_ERR_NO_SCENE. m_MaxBounces above 64 or m_LightCount above the scene's light count (as
 * hrpt_render), unknown flag bits, a NULL pointer, more than 2^31 rays, HRPT_RADIANCE_THREAD_PER_RAY on a two-level structure deeper than
 * that kernel's 64-entry stack: HRPT_ERR_INVALID_ARGUMENT. An error changes nothing. */
#define HRPT_RADIANCE_DEVICE_POINTERS 0x100u  /* rays / radiance are device pointers; asynchronous on the context stream */
#define HRPT_RADIANCE_THREAD_PER_RAY  0x200u  /* testing: the one-thread-per-ray kernel (same results) */
#define HRPT_RADIANCE_ACCUMULATE      0x400u  /* radiance[i].rgb += L, radiance[i].w += 1 instead of (L, 1) */
#define HRPT_RADIANCE_SECONDARY       0x1000u /* ray i is path segment 1 instead of 0 (0x800 stays an unknown bit) */
int  hrpt_trace_radiance(HrptContext* ctx, const HrptRay* rays, float* radiance4, uint64_t count,
                         const HrptPathTracerConstants* constants, uint32_t flags);

/* ---- first-hit G-buffer ------------------------------------------------------------------------------------------
 * What the primary ray of every pixel saw: path vertex 0 of ONE accumulation index, with the contents of the reference's GBufferOut
 * (src/shaders/BasePass.hlsl:184-192, 485-493) computed by the path tracer's own stages. For pixel (px, py) and params->constants:
 * the ray and the RNG seed are those of PathTracer.hlsl:61-72 with constants.m_Jitter AS GIVEN (pass 0, 0 for pixel-centre guides;
 * hrpt_render recomputes the jitter from the index, this call does not) and constants.m_AccumulationIndex; the hit is TraceRayStandard's,
 * MASK / stochastic BLEND candidates drawing from that RNG state -- for the constants hrpt_render uses for an index this is the surface it
 * shades at bounce 0. m_MaxBounces, the lights and the sun are not read. accumCount must be 1.
 * Six planes of width x height texels, 16 bytes each, owned by the library; a plane is allocated (zeroed) by the first call that requests
 * it and re-allocated (zeroed) by hrpt_resize. Normals are unit vectors in binary32 (no octahedral packing, no render-target formats).
 *   plane                 type     hit                                                                          miss
 *   HRPT_GB_ALBEDO        float4   pbr.baseColor, pbr.alpha                                                     0, 0, 0, 0
 *   HRPT_GB_NORMAL        float4   shading normal N, negated when dot(N, -d) < 0 (PathTracer.hlsl:111-117); w = roughness (>= 0.04)   0, 0, 0, 0
 *   HRPT_GB_GEO_NORMAL    float4   Ng = normalize(interpolated vertex normal in world space), not flipped; w = metallic     0, 0, 0, 0
 *   HRPT_GB_EMISSIVE      float4   pbr.emissive, 1                                                              0, 0, 0, 0
 *   HRPT_GB_DEPTH         float4   t, viewDepth = (float4(o + d t, 1) * m_MatWorldToClipNoOffset).w, u, v (weights of v1, v2)   1e10, 1e10, 0, 0
 *   HRPT_GB_IDS           uint4    instance, primitive, material index, flags (HRPT_GB_FLAG_*)                  0xFFFFFFFF x 3, 0
 * hrpt_render_gbuffer honours the tile rectangle, the stripes and HRPT_FRAME_MEGAKERNEL / _WAVEFRONT of params exactly as hrpt_render does,
 * writes only the planes in planeMask and only the pixels of the tile, is asynchronous on the context stream (ordered with renders) and
 * leaves Accumulation, Output, the exposure buffer and every HrptStats field as they were. planeMask == 0 or a bit >= HRPT_GB_PLANES:
 * HRPT_ERR_INVALID_ARGUMENT; no scene: HRPT_ERR_NO_SCENE. Motion vectors: hrpt_render_motion_vectors below (bit 6 stays an error here). */
enum { HRPT_GB_ALBEDO = 0, HRPT_GB_NORMAL = 1, HRPT_GB_GEO_NORMAL = 2, HRPT_GB_EMISSIVE = 3, HRPT_GB_DEPTH = 4, HRPT_GB_IDS = 5, HRPT_GB_PLANES = 6 };
#define HRPT_GB_ALL_PLANES 0x3Fu
#define HRPT_GB_FLAG_HIT 1u          /* the primary ray committed a hit */
#define HRPT_GB_FLAG_FRONT_FACE 2u   /* dot(Ng, d) < 0 (isFrontFace, PathTracer.hlsl:113) */
int  hrpt_render_gbuffer(HrptContext* ctx, const HrptFrameParams* params, uint32_t planeMask);
/* Host read-back of one plane (synchronises); bytes must be width*height*16. A plane that was never requested: HRPT_ERR_INVALID_ARGUMENT. */
int  hrpt_read_gbuffer(HrptContext* ctx, uint32_t plane, void* dst, size_t bytes);
/* Device pointer of one plane (valid until hrpt_resize / hrpt_destroy); NULL when the plane was never requested. */
int  hrpt_get_gbuffer_device(HrptContext* ctx, uint32_t plane, void** devicePtr);

/* ---- first-hit motion vectors -------------------------------------------------------------------------------------
 * The sixth target of the reference's GBufferOut: screen-space motion of the surface the primary ray of every pixel saw, by
 * ComputeMotionVectors (src/shaders/CommonLighting.hlsli:242-260) fed as the raster pass feeds it (src/shaders/BasePass.hlsl:53,492).
 * The hit (instance i, primitive p, barycentrics u, v) is the one hrpt_render_gbuffer commits for the same params. With q_k the object-space
 * positions of the primitive's LOD-0 vertices, cur_k = q_k * m_World_i, prev_k = q_k * m_PrevWorld_i (row-vector products, left to right),
 * bx = (1 - u) - v:  worldPos = (cur_0 bx + cur_1 u) + cur_2 v  and prevWorldPos likewise -- the INTERPOLATED vertex position, not o + d t,
 * so equal transforms and equal views give exactly (0, 0, 0). After hrpt_update_vertices, prev_k is formed from the object-space positions of
 * the PREVIOUS frame (see there); a context that never deforms has previous == current. Then
 *   clip = float4(worldPos, 1) * params->constants.m_View.m_MatWorldToClip,   prevClip = float4(prevWorldPos, 1) * prevView->m_MatWorldToClip
 *   window = clip.xy / clip.w * m_ClipToWindowScale + m_ClipToWindowBias      (prevWindow with prevView's scale and bias)
 *   texel  = (prevWindow.x - window.x, prevWindow.y - window.y, prevClip.w - clip.w, 1)        miss: (0, 0, 0, 0)
 * in binary32, one rounding per operation. x, y are in pixels and point from this frame's position to last frame's;
 * z is the change of linear view depth; w is the valid flag (the reference leaves it unused). The matrices are the jittered ones, as in the reference.
 * The caller maintains m_PrevWorld as the reference's Scene::Update does (src/Scene.cpp:413-417): before moving anything, m_PrevWorld <- m_World
 * for ALL instances, then hrpt_update_instances / hrpt_refit_instances over the full range; prevView is last frame's m_View.
 * planeMask names G-buffer planes (bits 0..5) to write in the same pass from the same hits, 0 = motion only; planes not named keep their
 * contents. Tile rectangle, stripes, frame flags, asynchrony and hrpt_set_stream as in hrpt_render_gbuffer; Accumulation, Output, exposure and
 * HrptStats are not touched. The motion plane (width x height x 16 bytes) is owned by the library, allocated (zeroed) by the first call and
 * re-allocated (zeroed) by hrpt_resize; the first call also uploads the tables it reads (positions, indices, one 64-byte record per instance),
 * later calls refresh what an upload or an instance update made stale. NULL params or prevView, accumCount != 1, a mask bit >= 6:
 * HRPT_ERR_INVALID_ARGUMENT; no scene: HRPT_ERR_NO_SCENE. prevClip.w == 0 or non-finite inputs give what IEEE 754 gives. */
int  hrpt_render_motion_vectors(HrptContext* ctx, const HrptFrameParams* params, const HrptPlanarViewConstants* prevView, uint32_t planeMask);
/* Host read-back of the motion plane (synchronises); bytes must be width*height*16. Before the first hrpt_render_motion_vectors: HRPT_ERR_INVALID_ARGUMENT. */
int  hrpt_read_motion_vectors(HrptContext* ctx, float* dst, size_t bytes);
/* Device pointer of the motion plane (valid until hrpt_resize / hrpt_destroy); NULL until the first hrpt_render_motion_vectors. */
int  hrpt_get_motion_vectors_device(HrptContext* ctx, void** devicePtr);

/* Host read-back (synchronises). bytes must be width*height*16. */
int  hrpt_read_accumulation(HrptContext* ctx, float* rgba, size_t bytes);
int  hrpt_read_output(HrptContext* ctx, float* rgba, size_t bytes);
/* Host write of the accumulation image (resume a progressive render). */
int  hrpt_write_accumulation(HrptContext* ctx, const float* rgba, size_t bytes);
/* Output = accum.rgb / accum.a for every pixel (PathTracer.hlsl:339), e.g. after an all-gather of accumulation tiles. */
int  hrpt_resolve_output(HrptContext* ctx);
/* The same resolve over caller-owned DEVICE images (pixelCount float4 each) on the caller's stream: the consumer of a
 * gathered accumulation image that lives outside the context (pipelined multi-GPU frames, hobbyrenderer_amd/distributed.py).
 * Asynchronous; stream is a hipStream_t (NULL = the default stream). */
int  hrpt_resolve_device(HrptContext* ctx, const float* accumulationDevice, float* outputDevice, uint64_t pixelCount, void* stream);
/* The consumer of column-interleaved shards (HrptFrameParams::stripeCount): `shardsDevice` holds the all-gathered accumulation shards of
 * `ranks` ranks, rank-major -- rank r's block is [height][width / 8 / ranks][8] float4, its k-th column being image column k * ranks + r.
 * Writes Output = rgb / a in image order to outputDevice and, unless accumulationDevice is NULL, the re-assembled accumulation image:
 * one pass over the data instead of re-assembly followed by hrpt_resolve_device. width must be a multiple of 8 * ranks. Asynchronous. */
int  hrpt_resolve_columns_device(HrptContext* ctx, const float* shardsDevice, float* accumulationDevice, float* outputDevice,
                                 uint32_t width, uint32_t height, uint32_t ranks, void* stream);

/* ---- HDR post chain: the consumer of the pass -------------------------------------------------
 * HDRRenderer::Render (src/HDRRenderer.cpp:88-224) over Output (u0 = g_RG_HDRColor in path-tracer mode):
 * luminance histogram (src/shaders/LuminanceHistogram.hlsl), exposure adaptation (ExposureAdaptation.hlsl) or manual
 * exposure (Camera::m_Exposure, src/Camera.cpp:107-108), then Tonemap_PSMain (PBR-Neutral + sRGB OETF) or
 * TonemapHDR_PSMain (scRGB roll-off) of src/shaders/Tonemap.hlsl into a W x H float4 display image. */
typedef struct HrptPostParams {
    uint32_t autoExposure;          /* Renderer::m_EnableAutoExposure (src/Renderer.h:303) */
    float    manualExposure;        /* Camera::m_Exposure = 1 / (2^EV * 1.2); used when autoExposure == 0 */
    float    deltaTimeSeconds;      /* m_FrameTime / 1000 */
    float    adaptationSpeed;       /* Renderer::m_AdaptationSpeed, default 5 */
    float    exposureValueMin;      /* Camera::m_ExposureValueMin, default -7 */
    float    exposureValueMax;      /* Camera::m_ExposureValueMax, default 23 */
    float    exposureCompensation;  /* Camera::m_ExposureCompensation */
    uint32_t hdrDisplay;            /* GraphicRHI::m_bIsHDR: 0 = Tonemap_PSMain, 1 = TonemapHDR_PSMain */
    float    maxDisplayNits;        /* GraphicRHI::m_MaxDisplayNits */
} HrptPostParams;
int  hrpt_post_process(HrptContext* ctx, const HrptPostParams* params);
int  hrpt_read_display(HrptContext* ctx, float* rgba, size_t bytes);           /* W*H*16 bytes */
/* The exposure and the histogram of the last auto-exposure pass (histogram may be NULL). The histogram is all zero until the first
 * auto-exposure pass, and again after every manual-exposure pass; before any post pass or hrpt_set_exposure: HRPT_ERR_INVALID_ARGUMENT. */
int  hrpt_get_exposure(HrptContext* ctx, float* exposure, uint32_t histogram256[256]);
int  hrpt_set_exposure(HrptContext* ctx, float exposure);                      /* the persistent exposure buffer, initially 1 */
/* The same chain over caller-owned DEVICE images (pixelCount float4 each; e.g. the upscaled image of hrpt_upscale, whose size is not the
 * context's), asynchronous on the caller's stream (a hipStream_t; NULL = the default stream). It runs on the context's histogram and
 * exposure, exactly as hrpt_post_process does: on a copy of Output it writes hrpt_post_process's display image bit for bit and leaves the
 * same exposure. hdrDevice is only read; displayDevice must differ from it. pixelCount may be anything in 1..2^32-1: above 524288 pixels
 * (2048 blocks of 256 threads) the kernels walk the image in strides, with a 64-bit index that cannot wrap. NULL pointers or pixelCount
 * outside 1..2^32-1: HRPT_ERR_INVALID_ARGUMENT, before anything is launched. */
int  hrpt_post_process_device(HrptContext* ctx, const float* hdrDevice, float* displayDevice, uint64_t pixelCount, const HrptPostParams* params, void* stream);

/* ---- Bloom: the stage in front of the post chain ---------------------------------------------------------------
 * BloomRenderer::Render (src/BloomRenderer.cpp:48-175) + src/shaders/Bloom.hlsl over the HDR colour image: soft-knee prefilter into a
 * half-resolution pyramid of up to six R11G11B10_FLOAT levels, Jimenez 13-tap downsamples, 9-tap tent upsamples, additive composite
 * hdr.rgb += bloom * intensity (alpha untouched). The reference schedules it in its raster modes only and off by default
 * (Renderer::m_EnableBloom); here it is an opt-in call and nothing calls it implicitly. Call order of a frame:
 * hrpt_render -> hrpt_bloom -> hrpt_post_process. Pixel uv, the bilinear filter, the packed format's rounding and the schedule for
 * images with fewer than six levels are defined in hobbyrenderer_amd/csrc/pt_bloom.h (an image narrower or lower than 2 pixels has no
 * level and is left unchanged). knee, intensity and upsampleRadius must be finite and >= 0. */
typedef struct HrptBloomParams {
    float knee;            /* Renderer::m_BloomKnee,      src/Renderer.h:378, default 0.1   */
    float intensity;       /* Renderer::m_BloomIntensity, src/Renderer.h:307, default 0.005 */
    float upsampleRadius;  /* Renderer::m_UpsampleRadius, src/Renderer.h:379, default 0.85  */
    uint32_t reserved;     /* 0 */
} HrptBloomParams;
/* Composites into the context's Output image in place, asynchronously on the context stream like hrpt_post_process: a following
 * hrpt_post_process / hrpt_read_output sees the bloomed image. Every render re-resolves Output from the accumulation, so bloom never
 * feeds back into it; two calls without a render in between bloom twice (one call per frame, like the reference). The pyramids are
 * context-owned, allocated at the first call and after a resize. */
int  hrpt_bloom(HrptContext* ctx, const HrptBloomParams* params);
/* The same over a caller-owned DEVICE image (width * height float4, e.g. the assembled multi-GPU frame), asynchronous on the caller's
 * stream (a hipStream_t; NULL = the default stream). It uses the context's pyramids as scratch: do not overlap it with another bloom
 * call of the same context on a different stream. */
int  hrpt_bloom_device(HrptContext* ctx, float* hdrDevice, uint32_t width, uint32_t height, const HrptBloomParams* params, void* stream);
/* The same arithmetic on host threads over host images (no GPU needed; nthreads <= 0: one per hardware thread, at most 16). hdrOut may
 * be hdrIn. Bit-identical to the device calls. */
int  hrpt_bloom_host(const float* hdrIn, float* hdrOut, uint32_t width, uint32_t height, const HrptBloomParams* params, int nthreads);
/* Test hook (host only): packed[i] = the R11G11B10_FLOAT word the pyramids store for rgb[3i .. 3i + 2], unpackedRgb[3i ..] = what a
 * sample reads back from it. Either output may be NULL. */
int  hrpt_bloom_pack_probe(const float* rgb, uint32_t count, uint32_t* packed, float* unpackedRgb);

/* ---- Temporal accumulation: reprojected accumulation across frames --------------------------------------------------
 * The consumer of the G-buffer and the motion vectors: the reference's SSGI temporal pass (src/shaders/SSGITemporalReproject.hlsl, driven by
 * src/SSGIRenderer.cpp:170-230, m_SSGI_TemporalBlend = 0.9) over the path tracer's own images. Per pixel: reproject through the motion
 * vector, validate the reprojected position against this frame's depth, normal and velocity, resample last call's history with
 * SampleTextureCatmullRom (nine bilinear taps + anti-ringing clamp), blend with an age kept in the history's alpha, cap the history weight
 * at `blend` where the pixel moves more than a pixel. hobbyrenderer_amd/csrc/pt_temporal.h is the definition: what
 * the samplers do, the depth convention, the miss rule, and the differences from the reference (no history = confidence 0; the linear mode).
 * All images are width x height float4: color = Output of hrpt_render; motion = the plane of hrpt_render_motion_vectors; depth / normal =
 * the planes HRPT_GB_DEPTH / HRPT_GB_NORMAL of the same frame; history: rgb = accumulated radiance, a = age (frames behind the estimate).
 * Outputs: historyOut = (blended rgb, new age), colorOut = (blended rgb, color.a). view->m_ViewportSize must equal (width, height);
 * view->m_CameraDirectionOrPosition.xyz must hold the camera position. Opt-in: nothing calls it implicitly. Not part of multi-GPU tiles:
 * it works on whole images, run it after the gather. */
#define HRPT_TEMPORAL_LINEAR 1u   /* blend in linear radiance instead of the reference's log(1 + x) space */
#define HRPT_TEMPORAL_RESET  2u   /* context call: ignore the stored history this call */
typedef struct HrptTemporalParams {
    float blend;          /* SSGITemporalConstants::m_Blend, default 0.9 (src/Renderer.h:358); finite, in [0, 1] */
    uint32_t flags;       /* HRPT_TEMPORAL_* */
    uint32_t reserved[2]; /* 0 */
} HrptTemporalParams;
typedef struct HrptTemporalImages {
    const float *color, *motion, *depth, *normal;
    const float *historyIn;     /* NULL = no history */
    float *historyOut;          /* must differ from historyIn */
    float *colorOut;            /* may equal color */
} HrptTemporalImages;
/* The stage on host threads over host images (no GPU needed; nthreads <= 0: one per hardware thread, at most 16). Bit-identical to the
 * device calls. NULL arguments or images (historyIn excepted), historyOut == historyIn, a size outside 1..65535, m_ViewportSize != the
 * size, blend outside [0, 1] or not finite, unknown flag bits, non-zero reserved: HRPT_ERR_INVALID_ARGUMENT. HRPT_TEMPORAL_RESET is
 * accepted and means nothing here (pass historyIn = NULL). */
int  hrpt_temporal_host(const HrptTemporalImages* images, uint32_t width, uint32_t height, const HrptPlanarViewConstants* view,
                        const HrptPlanarViewConstants* prevView, const HrptTemporalParams* params, int nthreads);
/* The same over caller-owned DEVICE images, asynchronous on the caller's stream (a hipStream_t; NULL = the default stream). */
int  hrpt_temporal_device(HrptContext* ctx, const HrptTemporalImages* deviceImages, uint32_t width, uint32_t height,
                          const HrptPlanarViewConstants* view, const HrptPlanarViewConstants* prevView, const HrptTemporalParams* params, void* stream);
/* The stage over the context's own images: color = colorOut = Output, the motion plane and the planes HRPT_GB_DEPTH and HRPT_GB_NORMAL as
 * the caller filled them for this frame with hrpt_render_motion_vectors(..., planeMask = DEPTH | NORMAL), and a library-owned ping-pong
 * pair of history images, allocated by the first call and re-allocated (history dropped) by hrpt_resize. The first call, the first call
 * after a resize and a call with HRPT_TEMPORAL_RESET run without history. Asynchronous on the context stream, ordered with renders,
 * honours hrpt_set_stream. Accumulation, the planes, exposure and HrptStats are not touched; every render re-resolves Output, so the
 * stage never feeds back into the accumulation. Frame order:
 *   hrpt_clear_accumulation -> hrpt_render -> hrpt_render_motion_vectors -> [hrpt_demodulate] -> hrpt_temporal_accumulate -> [hrpt_denoise]
 *   -> [hrpt_compose] -> hrpt_bloom -> hrpt_post_process
 * A motion, depth or normal plane that was never requested, and the argument errors of hrpt_temporal_host: HRPT_ERR_INVALID_ARGUMENT. */
int  hrpt_temporal_accumulate(HrptContext* ctx, const HrptPlanarViewConstants* view, const HrptPlanarViewConstants* prevView, const HrptTemporalParams* params);
/* Host read-back of the history the last hrpt_temporal_accumulate wrote (synchronises); bytes must be width*height*16. Before the first
 * call: HRPT_ERR_INVALID_ARGUMENT; after a resize: the new size, zeroed (as hrpt_read_motion_vectors). */
int  hrpt_read_temporal_history(HrptContext* ctx, float* dst, size_t bytes);
/* Device pointer of that image (valid until the next hrpt_temporal_accumulate / hrpt_resize / hrpt_destroy); NULL before the first call. */
int  hrpt_get_temporal_history_device(HrptContext* ctx, void** devicePtr);

/* ---- Temporal upscaling: a display-size image from jittered render-size frames ------------------------------------------------
 * The stage in the slot where the reference schedules its TAARenderer, between lighting and bloom / the HDR pass (src/Renderer.cpp:1296,1311).
 * The reference's body there is a closed FSR3 call (src/TAARenderer.cpp:226-252) that it runs at render size == display size; none of its
 * code is in the reference, so this stage is DEFINED by this library (hobbyrenderer_amd/csrc/pt_upscale.h) and parity
 * with FSR is out of scope. Cost in a path tracer is proportional to pixels: render width x height, reconstruct displayWidth x displayHeight
 * from the sub-pixel jitter of successive frames. Per display pixel: a Gaussian-weighted resolve of the 3 x 3 render texels around it (the
 * weights measured in display pixels from where this frame's jittered samples lie), reprojection of the display-size history through the
 * motion of the nearest-depth tap, SampleTextureCatmullRom, a clamp of the history to the taps' colour range, and a blend whose weight is
 * how well this frame samples the pixel against the sample weight the history holds (kept in its alpha, capped at maxHistory).
 * Images are row-major float4. width x height: color = Output of hrpt_render (rgb radiance, a); depth = the plane HRPT_GB_DEPTH; motion = the
 * plane of hrpt_render_motion_vectors (.xy in render pixels). displayWidth x displayHeight: historyIn / historyOut (rgb, a = accumulated
 * sample weight), colorOut (rgb, a = alpha of the nearest render texel). Sizes are 1..65535 with width <= displayWidth <= 4 * width and
 * height <= displayHeight <= 4 * height; ratios need not be integers, and displayWidth == width is plain temporal antialiasing.
 * view / prevView are the RENDER-size views of this and of last frame: view->m_ViewportSize must equal (width, height).
 * Which jitter to pass: a frame rendered with accumCount == 1 at accumulation index i takes its primary-ray offset from that index, so pass
 * jitter = (hrpt_halton(i + 1, 2) - 0.5, hrpt_halton(i + 1, 3) - 0.5), and pass the same pair as m_Jitter to hrpt_render_motion_vectors so
 * that depth and motion belong to the same samples. With accumCount > 1 the samples of a pixel are already spread over it: pass (0, 0) and
 * render the planes with zero jitter.
 * Left out on purpose: sharpening (m_TAASharpness), tonemapped-space blend weights, a kept previous depth (disocclusion is handled by the
 * clamp alone), a reactive mask. Opt-in: nothing calls it implicitly. Not part of multi-GPU tiles: it works on whole images, run it after
 * the gather. */
#define HRPT_UPSCALE_NO_CLAMP 1u   /* do not clamp the reprojected history to the colour range of the pixel's nine taps */
#define HRPT_UPSCALE_RESET    2u   /* context call: ignore the stored history this call */
typedef struct HrptUpscaleParams {
    float jitter[2];      /* this frame's sample offset in render pixels (the m_Jitter it was rendered with); finite, each in [-0.5, 0.5] */
    float kernel;         /* tap weight exp(-kernel * d^2), d in display pixels; default 2.29 (the Gaussian fit to Blackman-Harris); finite, in (0, 16] */
    float maxHistory;     /* cap of the accumulated sample weight, default 8; finite, >= 0 */
    uint32_t flags;       /* HRPT_UPSCALE_* */
    uint32_t reserved[3]; /* 0 */
} HrptUpscaleParams;
typedef struct HrptUpscaleImages {
    const float *color, *depth, *motion;   /* width x height */
    const float *historyIn;                /* displayWidth x displayHeight; NULL = no history */
    float *historyOut;                     /* must differ from historyIn */
    float *colorOut;                       /* must differ from historyIn and historyOut */
} HrptUpscaleImages;
/* The stage on host threads over host images (no GPU needed; nthreads <= 0: one per hardware thread, at most 16). Bit-identical to the
 * device calls. NULL arguments or images (historyIn excepted), historyOut == historyIn, colorOut == historyIn or historyOut, a size outside
 * 1..65535, a display size outside [size, 4 * size], m_ViewportSize != (width, height), a parameter outside the ranges above, unknown flag
 * bits, non-zero reserved: HRPT_ERR_INVALID_ARGUMENT, and nothing is written. HRPT_UPSCALE_RESET is accepted and means nothing here (pass
 * historyIn = NULL). */
int  hrpt_upscale_host(const HrptUpscaleImages* images, uint32_t width, uint32_t height, uint32_t displayWidth, uint32_t displayHeight,
                       const HrptPlanarViewConstants* view, const HrptPlanarViewConstants* prevView, const HrptUpscaleParams* params, int nthreads);
/* The same over caller-owned DEVICE images, asynchronous on the caller's stream (a hipStream_t; NULL = the default stream). */
int  hrpt_upscale_device(HrptContext* ctx, const HrptUpscaleImages* deviceImages, uint32_t width, uint32_t height, uint32_t displayWidth,
                         uint32_t displayHeight, const HrptPlanarViewConstants* view, const HrptPlanarViewConstants* prevView,
                         const HrptUpscaleParams* params, void* stream);
/* The stage over the context's own images: color = Output, depth and motion = the plane HRPT_GB_DEPTH and the motion plane as the caller
 * filled them for this frame with hrpt_render_motion_vectors(..., planeMask = DEPTH), a library-owned ping-pong pair of display-size
 * histories and a library-owned display-size colour image. These are allocated by the first call and re-allocated, with the history
 * dropped, when the display size changes or after hrpt_resize. The first call, the first call after either, and a call with
 * HRPT_UPSCALE_RESET run without history. Asynchronous on the context stream, honours hrpt_set_stream. It touches nothing else: Output,
 * Accumulation, the planes, the temporal history, exposure and HrptStats stay as they were. Frame order:
 *   hrpt_clear_accumulation -> hrpt_render -> hrpt_render_motion_vectors -> [hrpt_demodulate -> hrpt_temporal_accumulate -> hrpt_denoise
 *   -> hrpt_compose] -> hrpt_upscale -> hrpt_bloom_device -> hrpt_post_process_device
 * the last two over the upscaled image (hrpt_get_upscaled_device) at the display size. A motion or depth plane that was never requested,
 * and the argument errors of hrpt_upscale_host: HRPT_ERR_INVALID_ARGUMENT, and nothing changes. */
int  hrpt_upscale(HrptContext* ctx, uint32_t displayWidth, uint32_t displayHeight, const HrptPlanarViewConstants* view,
                  const HrptPlanarViewConstants* prevView, const HrptUpscaleParams* params);
/* Host read-backs of the colour image and of the history the last hrpt_upscale wrote (synchronise); bytes must be displayWidth *
 * displayHeight * 16 of that call. With no such image (before the first call, after hrpt_resize): HRPT_ERR_INVALID_ARGUMENT. */
int  hrpt_read_upscaled(HrptContext* ctx, float* dst, size_t bytes);
int  hrpt_read_upscale_history(HrptContext* ctx, float* dst, size_t bytes);
/* Device pointer of the colour image (valid until a call of hrpt_upscale with another display size, hrpt_resize or hrpt_destroy); NULL
 * where hrpt_read_upscaled would fail. */
int  hrpt_get_upscaled_device(HrptContext* ctx, void** devicePtr);

/* ---- Denoise: edge-stopping Poisson filter after the temporal accumulation ---------------------------------------------
 * The spatial half of the real-time chain: the reference's SSGI denoise pass (src/shaders/SSGIDenoise.hlsl, iterated with a doubling radius
 * by src/SSGIRenderer.cpp:217-276) over the path tracer's own images. An 8-tap Poisson disk, rotated per pixel by a 64 x 64 noise tile,
 * gathers neighbours in log(1 + x) space; each tap is weighted by normal, plane distance, roughness and luminance against the centre, and
 * the younger a pixel's history is (input.a, clamped at 64), the wider and the more permissive its filter. After a camera cut or a
 * disocclusion hrpt_temporal_accumulate hands back raw samples with age 0: this is the stage that filters them.
 * hobbyrenderer_amd/csrc/pt_denoise.h is the definition. All images are width x height float4:
 *   input     rgb = radiance, a = age (the history of the temporal stage)
 *   depth     HRPT_GB_DEPTH (view depth in .y, miss: .x == 1e10f)      normal  HRPT_GB_NORMAL (unit normal, roughness in .w)
 *   geoNormal HRPT_GB_GEO_NORMAL (metallic in .w)                      noise   64 * 64 * 2 floats, noise[y][x][2], or NULL
 *   output    (filtered rgb, input.a unclamped); must differ from input
 *   color / colorOut   both NULL or both set: colorOut = (filtered rgb, color.a). colorOut may equal color; neither may equal input.
 * Differences from the reference, on purpose: a miss passes its input texel through (the reference writes 0; here Output holds the sky
 * there); one radiance image, so the separate specular signal (w2, m_SpecularPhi, specularFactor) is not restated, and the image plays both
 * signals in the age falloff; the planes hold unit normals, so there is no DecodeNormal. The noise tile is an input. The reference ships its
 * 64 x 64 blue-noise texture as a data file (external/LDR_RG01_0.png, loaded by src/CommonResources.cpp:575); the library may not embed that
 * file, so with noise == NULL it uses its built-in default tile, texel (x, y) = the first two numbers of hrt_rng_seed(x, y, 0) -- WHITE
 * noise, not blue noise. A caller that has the reference's tile (or any other) passes it here, or installs it on a context with
 * hrpt_set_denoise_noise, and gets the reference's behaviour.
 * view->m_ViewportSize must equal (width, height); view->m_CameraDirectionOrPosition.xyz must hold the camera position. Opt-in: nothing
 * calls it implicitly. Not part of multi-GPU tiles: it works on whole images, run it after the gather. */
#define HRPT_DENOISE_OUTPUT_ONLY 1u   /* context call: filter Output only, leave the temporal history as the temporal stage wrote it */
typedef struct HrptDenoiseParams {
    float radius;         /* Renderer::m_SSGI_DenoiseRadius, default 3 (src/Renderer.h:362-368); finite, > 0 */
    float phi;            /* m_SSGI_DenoisePhi, default 0.5; finite, > 0 */
    float lumaPhi;        /* m_SSGI_DenoiseLumaPhi, default 5; finite, >= 0 */
    float depthPhi;       /* m_SSGI_DenoiseDepthPhi, default 2; finite, >= 0 */
    float normalPhi;      /* m_SSGI_DenoiseNormalPhi, default 50; finite, >= 0 */
    float roughnessPhi;   /* m_SSGI_DenoiseRoughnessPhi, default 50; finite, >= 0 */
    uint32_t iterations;  /* m_SSGI_DenoiseIterations, default 1; 1..5. Pass i uses radius * 2^i, which must stay finite */
    uint32_t frame;       /* the frame number that seeds the disk rotation (Renderer::m_FrameNumber) */
    uint32_t flags;       /* HRPT_DENOISE_* */
    uint32_t reserved;    /* 0 */
} HrptDenoiseParams;
typedef struct HrptDenoiseImages {
    const float *input, *depth, *normal, *geoNormal;
    const float *noise;         /* 64 * 64 * 2 floats, or NULL = the default tile */
    float *output;              /* must differ from input */
    const float *color;         /* NULL, or the image whose alpha colorOut keeps */
    float *colorOut;            /* NULL exactly when color is; may equal color */
} HrptDenoiseImages;
/* ONE pass on host threads over host images (no GPU needed; nthreads <= 0: one per hardware thread, at most 16), with params->radius and
 * params->frame as given; params->iterations must be 1. Bit-identical to the device calls. NULL arguments or images (noise, and color with
 * colorOut, excepted), output == input, color or colorOut == input, one of color / colorOut without the other, a size outside 1..65535,
 * m_ViewportSize != the size, a parameter outside the ranges above, unknown flag bits, non-zero reserved: HRPT_ERR_INVALID_ARGUMENT.
 * HRPT_DENOISE_OUTPUT_ONLY is accepted and means nothing here. */
int  hrpt_denoise_host(const HrptDenoiseImages* images, uint32_t width, uint32_t height, const HrptPlanarViewConstants* view,
                       const HrptDenoiseParams* params, int nthreads);
/* The same pass over caller-owned DEVICE images (noise, where given, is a device address too), asynchronous on the caller's stream (a
 * hipStream_t; NULL = the default stream). The default tile is uploaded once per context. */
int  hrpt_denoise_device(HrptContext* ctx, const HrptDenoiseImages* deviceImages, uint32_t width, uint32_t height,
                         const HrptPlanarViewConstants* view, const HrptDenoiseParams* params, void* stream);
/* The stage over the context's own images, after hrpt_temporal_accumulate: input = the temporal history, the planes HRPT_GB_DEPTH,
 * HRPT_GB_NORMAL and HRPT_GB_GEO_NORMAL as the caller filled them for this frame, the context's noise tile (hrpt_set_denoise_noise; the
 * default tile until it is called). It runs params->iterations passes;
 * pass i uses radius * (float)(1u << i) and frame * iterations + i (uint32, wrapping), and the last pass also writes Output as
 * (filtered rgb, Output.a). By default, as in the reference, the passes ping-pong between the two history images (the stale one is free
 * after the temporal call) and the filtered image BECOMES the history: the next hrpt_temporal_accumulate reprojects it, and
 * hrpt_read_temporal_history / hrpt_get_temporal_history_device return it. With HRPT_DENOISE_OUTPUT_ONLY the history stays bit for bit
 * what the temporal stage wrote and only Output is filtered (this keeps the exact running mean of HRPT_TEMPORAL_LINEAR); the passes then
 * use a library-owned scratch pair, allocated at first use and dropped by hrpt_resize. Asynchronous on the context stream, honours
 * hrpt_set_stream; Accumulation, the planes, exposure and HrptStats are not touched. Frame order:
 *   ... -> [hrpt_demodulate] -> hrpt_temporal_accumulate -> hrpt_denoise -> [hrpt_compose] -> hrpt_bloom -> hrpt_post_process
 * No valid temporal history at the current size (hrpt_temporal_accumulate not called since hrpt_resize), a depth, normal or geo-normal
 * plane that was never requested, and the argument errors of hrpt_denoise_host (iterations 1..5 here): HRPT_ERR_INVALID_ARGUMENT. */
int  hrpt_denoise(HrptContext* ctx, const HrptPlanarViewConstants* view, const HrptDenoiseParams* params);
/* Replaces the noise tile that hrpt_denoise, and hrpt_denoise_device with noise == NULL, use for this context: hostTile holds 64 * 64 * 2
 * floats, hostTile[y][x][2]; NULL restores the built-in default tile. The copy is ordered on the context stream (calls enqueued before it
 * see the old tile, calls after it the new one) and hostTile may be reused on return. Until it is called the behaviour is that of the
 * default tile. A value that is not finite: HRPT_ERR_INVALID_ARGUMENT, and the tile in use stays. */
int  hrpt_set_denoise_noise(HrptContext* ctx, const float* hostTile);

/* ---- Demodulate / compose: keep textures out of the temporal and spatial filters -----------------------------------------------
 * The two stages around hrpt_temporal_accumulate and hrpt_denoise. The reference never filters radiance: its SSGI passes run on a signal
 * with the first-hit BRDF factored out, and its compose pass (src/shaders/SSGICompose.hlsl:75-107) multiplies albedo * (1 - metalness) *
 * (1 - F) and F back in, F being a Schlick Fresnel term at a deterministic GGX half vector. The denoiser's edge stops (normal, plane
 * distance, roughness, luminance) do not see albedo, so filtering radiance itself averages a texture away. hrpt_demodulate divides the
 * factor out of the colour image and stores it; hrpt_compose multiplies the stored factor back in. Per pixel (the definition is
 * hobbyrenderer_amd/csrc/pt_modulation.h), with E = emissive.rgb (0 without an emissive image):
 *   miss (depth.x == 1e10f)   modulation = (1, 1, 1, 0); both stages pass the colour texel through bit for bit
 *   hit                       M = albedo * (1 - metallic) * (1 - F) + F per channel, Mf = max(M, floor), modulation = (Mf, 1)
 *   demodulate                colorOut = (max(color.rgb - E, 0) / Mf, color.a)
 *   compose                   colorOut = (color.rgb * Mf + E, color.a), Mf read from `modulation` (a == 0 marks a miss)
 * floor (finite, > 0; default 0.04, the least value a channel of M takes on a non-metal, so that it only bites on dark metals) bounds the
 * amplification of the division. Both stages use the same Mf: where nothing was filtered compose undoes demodulate up to rounding
 * (|compose(demodulate(x)) - x| <= 5 * 2^-24 * x for normal numbers with x >= E >= 0, 3 * 2^-24 * x when E == 0).
 * All images are width x height float4: color = Output of hrpt_render; albedo, normal (roughness in .w), geoNormal (metallic in .w),
 * emissive, depth = the planes HRPT_GB_ALBEDO, HRPT_GB_NORMAL, HRPT_GB_GEO_NORMAL, HRPT_GB_EMISSIVE, HRPT_GB_DEPTH of the same frame.
 * view->m_ViewportSize must equal (width, height); view->m_CameraDirectionOrPosition.xyz must hold the camera position. Opt-in: nothing
 * calls them implicitly. Not part of multi-GPU tiles: they work on whole images, run them after the gather. */
typedef struct HrptModulationParams {
    float floor;          /* lower bound of every channel of the factor; finite, > 0; default 0.04 */
    uint32_t flags;       /* 0 */
    uint32_t reserved[2]; /* 0 */
} HrptModulationParams;
typedef struct HrptDemodulateImages {
    const float *color, *albedo, *normal, *geoNormal, *depth;
    const float *emissive;      /* NULL = 0 */
    float *colorOut;            /* may equal color; must differ from every other image */
    float *modulationOut;       /* required; must differ from every other image */
} HrptDemodulateImages;
typedef struct HrptComposeImages {
    const float *color, *modulation;
    const float *emissive;      /* NULL = 0 */
    float *colorOut;            /* may equal color; must differ from modulation and emissive */
} HrptComposeImages;
/* The stages on host threads over host images (no GPU needed; nthreads <= 0: one per hardware thread, at most 16). Bit-identical to the
 * device calls. NULL arguments or images (emissive excepted), an output that equals an image it must differ from, a size outside
 * 1..65535, m_ViewportSize != the size, floor not finite or <= 0, flags != 0, non-zero reserved: HRPT_ERR_INVALID_ARGUMENT. */
int  hrpt_demodulate_host(const HrptDemodulateImages* images, uint32_t width, uint32_t height, const HrptPlanarViewConstants* view,
                          const HrptModulationParams* params, int nthreads);
int  hrpt_compose_host(const HrptComposeImages* images, uint32_t width, uint32_t height, int nthreads);
/* The same over caller-owned DEVICE images, asynchronous on the caller's stream (a hipStream_t; NULL = the default stream). */
int  hrpt_demodulate_device(HrptContext* ctx, const HrptDemodulateImages* deviceImages, uint32_t width, uint32_t height,
                            const HrptPlanarViewConstants* view, const HrptModulationParams* params, void* stream);
int  hrpt_compose_device(HrptContext* ctx, const HrptComposeImages* deviceImages, uint32_t width, uint32_t height, void* stream);
/* The stages over the context's own images. hrpt_demodulate: color = colorOut = Output, the planes HRPT_GB_ALBEDO, HRPT_GB_NORMAL,
 * HRPT_GB_GEO_NORMAL, HRPT_GB_EMISSIVE and HRPT_GB_DEPTH as the caller filled them for this frame (hrpt_render_motion_vectors or
 * hrpt_render_gbuffer with those five in planeMask), and a library-owned modulation image, allocated at first use and dropped by
 * hrpt_resize. hrpt_compose: Output in place, from that image and the emissive plane. Both are asynchronous on the context stream, honour
 * hrpt_set_stream, and touch neither Accumulation, the planes, the temporal history, exposure nor HrptStats. They are stateless otherwise,
 * like hrpt_bloom: every render re-resolves Output, two hrpt_demodulate calls without a render in between divide twice, two hrpt_compose
 * calls multiply twice. Frame order:
 *   hrpt_clear_accumulation -> hrpt_render -> hrpt_render_motion_vectors -> hrpt_demodulate -> hrpt_temporal_accumulate -> hrpt_denoise
 *   -> hrpt_compose -> hrpt_bloom -> hrpt_post_process
 * (the temporal history then holds the demodulated signal, as the reference's does). hrpt_demodulate with one of the five planes never
 * requested: HRPT_ERR_INVALID_ARGUMENT, the message names the plane. hrpt_compose with no modulation image at the current size
 * (hrpt_demodulate not called since hrpt_resize): HRPT_ERR_INVALID_ARGUMENT, the message names hrpt_demodulate. The argument errors of
 * hrpt_demodulate_host apply. */
int  hrpt_demodulate(HrptContext* ctx, const HrptPlanarViewConstants* view, const HrptModulationParams* params);
int  hrpt_compose(HrptContext* ctx);
/* Host read-back of the modulation image the last hrpt_demodulate wrote (synchronises); bytes must be width*height*16. With no such image
 * at the current size (before the first call, after a resize): HRPT_ERR_INVALID_ARGUMENT. */
int  hrpt_read_modulation(HrptContext* ctx, float* dst, size_t bytes);
/* Device pointer of that image (valid until hrpt_resize / hrpt_destroy); NULL where hrpt_read_modulation would fail. */
int  hrpt_get_modulation_device(HrptContext* ctx, void** devicePtr);
/* Test hook (host only): the factor of one hit with the view vector given instead of reconstructed -- outM3 = Mf for albedo3, the unit
 * normal N3, the unit vector V3 towards the camera, roughness, metallic and floor (pt_modulation.h factor()). It reaches branches that no
 * camera produces reliably (N == V exactly, both tangent-frame choices, grazing and back-facing V). NULL pointers: HRPT_ERR_INVALID_ARGUMENT. */
int  hrpt_modulation_probe(const float* albedo3, const float* N3, const float* V3, float rough, float metal, float floor, float* outM3);
/* Zeroes the Accumulation image, asynchronously on the context stream: a fresh frame that starts at a non-zero accumulation index. A
 * following hrpt_render with first index k > 0 and accumCount s leaves Accumulation.a == s and Output = rgb / s of exactly the indices
 * k .. k + s - 1 (both kernel paths add onto the stored image whenever the index is > 0). A per-frame render at index 0 would instead
 * reuse the same RNG seeds every frame, and a temporal accumulator fed by it converges to one fixed sample set. */
int  hrpt_clear_accumulation(HrptContext* ctx);

/* ---- irradiance probe volume ---------------------------------------------------------------------------------------------
 * A grid of probes that shoot path-traced rays, folds them into octahedral irradiance and distance atlases, and answers "what diffuse
 * light arrives at this point with this normal": the reference's real-time indirect-diffuse chain (src/shaders/ddgi/ProbeTraceCS.hlsl, the
 * two blending passes, IndirectQueryCS.hlsl -> g_RG_DDGIIndirect). The SDK arithmetic behind those shaders is not in the reference tree, so
 * the stage is DEFINED by this project after the published algorithm (Majercik et al., "Dynamic Diffuse Global Illumination with Ray-Traced
 * Irradiance Fields"); DESIGN.md section 26 has every operation in order, and pt_probes.h is its one source for kernels and host executors.
 * Parity with the RTXGI SDK, its texture formats and gamma blend, probe relocation / classification / scrolling, back-face detection and a
 * specular lookup are out of scope. Unlike the reference, a probe ray carries the path tracer's full estimate (hrpt_trace_radiance), so
 * there is no feedback of last frame's atlas and no energy clamp.
 *
 * Volume. Probe (x, y, z) has index p = x + counts[0] * (y + counts[1] * z) and position origin + (x, y, z) * spacing; P = the number of
 * probes. Valid: counts >= 1 and P <= 2^20; 1 <= raysPerProbe <= 1024; spacing and maxRayDistance finite and > 0; hysteresis in [0, 1);
 * distanceExponent finite and >= 1; normalBias and viewBias finite and >= 0; pad == 0. Anything else: HRPT_ERR_INVALID_ARGUMENT.
 * Atlases, per probe and contiguous, linear binary32: irradiance [P][8][8] float4 (6 x 6 interior texels plus a one-texel border; a texel
 * is (M, 1) with M the cosine-weighted mean radiance, so irradiance is pi * M), 1 KiB per probe; distance [P][16][16] float2 (14 x 14
 * interior plus border; (mean d, mean d^2)), 2 KiB per probe. */
typedef struct HrptProbeVolume {
    float origin[3]; float hysteresis;
    float spacing[3]; float maxRayDistance;
    uint32_t counts[3]; uint32_t raysPerProbe;
    float distanceExponent, normalBias, viewBias; uint32_t pad;
} HrptProbeVolume;                                                                                                         /* 64 B */
typedef struct HrptProbePoint { float position[3]; float pad0; float normal[3]; float pad1; float view[3]; float pad2; } HrptProbePoint;   /* 48 B */
typedef struct HrptProbes HrptProbes;
#define HRPT_PROBES_RESET           1u        /* hrpt_probes_update: ignore the stored history, store the new values */
#define HRPT_PROBES_DEVICE_POINTERS 0x100u    /* hrpt_probes_query: points / irradiance4 are device pointers; asynchronous on the context stream */
/* A volume on `ctx` with zeroed atlases and its own ray, radiance and hit buffers (P * raysPerProbe records each, sized here). Destroy it
 * before its context. hrpt_probes_destroy(NULL) is allowed. */
int  hrpt_probes_create(HrptContext* ctx, const HrptProbeVolume* volume, HrptProbes** out);
void hrpt_probes_destroy(HrptProbes* probes);
/* One update: ray generation for `frameSeed` (raysPerProbe directions shared by all probes: a spherical Fibonacci set under a rotation drawn
 * from the seed), hrpt_trace_radiance and hrpt_trace_rays (HRPT_RAYS_CLOSEST) on those records, and the blend into the atlases: the first
 * update after creation or with HRPT_PROBES_RESET stores the new value, later ones new + hysteresis * (old - new). The result equals, bit
 * for bit, hrpt_probes_rays_host -> hrpt_trace_radiance -> hrpt_trace_rays -> hrpt_probes_blend_host through the public calls.
 * Asynchronous on the context stream, ordered with renders and scene updates; Accumulation, Output, every plane and history, the exposure
 * and every HrptStats field stay as they were (the guarantees of hrpt_trace_radiance). No scene: HRPT_ERR_NO_SCENE. The argument rules of
 * the two trace calls apply to `constants`; unknown flag bits: HRPT_ERR_INVALID_ARGUMENT. An error leaves the atlases as they were. */
int  hrpt_probes_update(HrptProbes* probes, const HrptPathTracerConstants* constants, uint32_t frameSeed, uint32_t flags);
/* irradiance4[i] = (E.rgb, inside) at points[i]: position, unit normal, unit direction to the viewer (for the view bias). E is the
 * irradiance (pi * the blended mean radiance): a Lambertian surface reflects albedo / pi * E. inside = 1 when the biased point lies in the
 * grid's box; a point outside still gets the answer of the clamped cell. A non-finite position, normal or view gives (0, 0, 0, 0).
 * Host arrays (the call synchronises), or device pointers (16-byte aligned) with HRPT_PROBES_DEVICE_POINTERS. count == 0: HRPT_OK. */
int  hrpt_probes_query(HrptProbes* probes, const HrptProbePoint* points, float* irradiance4, uint64_t count, uint32_t flags);
/* The query at the first hit of every pixel, into a library-owned width x height float4 plane of the context (allocated on first use, dropped
 * by hrpt_resize): (E * intensity, 1) at a hit, (0, 0, 0, 0) at a miss. It reads the planes HRPT_GB_NORMAL and HRPT_GB_DEPTH as the caller
 * filled them for this frame (either never requested: HRPT_ERR_INVALID_ARGUMENT, the message names the plane); the world position is
 * ReconstructWorldPos of the view depth and the view vector normalize(camera position - world position), as hrpt_demodulate forms them.
 * This is the reference's g_RG_DDGIIndirect: multiply by albedo * (1 - metallic) / pi and add it to Output.
 * view->m_ViewportSize != the context's size, intensity not finite or < 0: HRPT_ERR_INVALID_ARGUMENT. Asynchronous on the context stream. */
int  hrpt_probes_shade_gbuffer(HrptProbes* probes, const HrptPlanarViewConstants* view, float intensity);
/* Host read-back of that plane (synchronises; bytes must be width * height * 16) and its device pointer (NULL before the first
 * hrpt_probes_shade_gbuffer and after hrpt_resize, where the read answers HRPT_ERR_INVALID_ARGUMENT). */
int  hrpt_read_probe_irradiance(HrptContext* ctx, float* dst, size_t bytes);
int  hrpt_get_probe_irradiance_device(HrptContext* ctx, void** devicePtr);
/* The atlases: host read-back (synchronises), device pointers (valid until hrpt_probes_destroy), and hrpt_probes_write, which installs
 * atlases (tests, baked volumes; synchronises) and makes them the history of the next update. irradiance: P * 256 floats, distance: P * 512
 * floats; either pointer may be NULL (skipped); a byte count that is not exactly that: HRPT_ERR_INVALID_ARGUMENT. */
int  hrpt_probes_read(HrptProbes* probes, float* irradiance, size_t irradianceBytes, float* distance, size_t distanceBytes);
int  hrpt_probes_get_device(HrptProbes* probes, void** irradiance, void** distance);
int  hrpt_probes_write(HrptProbes* probes, const float* irradiance, size_t irradianceBytes, const float* distance, size_t distanceBytes);
/* The stages alone, with no context (_host: host arrays, host threads, nthreads <= 0 = one per hardware thread up to 16) or on caller-owned
 * device memory (_device: every pointer 16-byte aligned, asynchronous on `stream`). Same bits as the stages inside hrpt_probes_update /
 * hrpt_probes_query. rays: raysOut receives P * raysPerProbe records (record p * N + k: origin = probe p, direction k, tmin 0, tmax 1e10,
 * rng = pcg(g + pcg(frameSeed))), directions4Out the N shared directions as float4 (w = 0); either may be NULL. blend: directions4 [N],
 * radiance4 and hits [P * N] as the trace calls wrote them (a ray with radiance4.w == 0 takes no part), the atlases updated in place;
 * hasHistory == 0 stores the new values. */
int  hrpt_probes_rays_host(const HrptProbeVolume* volume, uint32_t frameSeed, HrptRay* raysOut, float* directions4Out);
int  hrpt_probes_blend_host(const HrptProbeVolume* volume, const float* directions4, const float* radiance4, const HrptRayHit* hits,
                            float* irradianceInOut, float* distanceInOut, uint32_t hasHistory, int nthreads);
int  hrpt_probes_blend_device(HrptContext* ctx, const HrptProbeVolume* volume, const float* directions4, const float* radiance4, const HrptRayHit* hits,
                              float* irradianceInOut, float* distanceInOut, uint32_t hasHistory, void* stream);
int  hrpt_probes_query_host(const HrptProbeVolume* volume, const float* irradiance, const float* distance, const HrptProbePoint* points, float* out4,
                            uint64_t count, int nthreads);

/* ---- deferred lighting -----------------------------------------------------------------------------------------------------
 * Turns the first-hit G-buffer into a lit image: the reference's DeferredLighting.hlsl with AccumulateDirectLighting
 * (src/shaders/CommonLighting.hlsli:501-603) and Sky.hlsl, over the planes HRPT_GB_ALBEDO (A), HRPT_GB_NORMAL (N, roughness in .w),
 * HRPT_GB_GEO_NORMAL (metallic in .w), HRPT_GB_EMISSIVE (E) and HRPT_GB_DEPTH (.x = t, miss == 1e10f) of a frame rendered with `constants`.
 * One source for kernels and host executors: hobbyrenderer_amd/csrc/pt_deferred.h; DESIGN.md section 27 has every operation in order.
 * Per pixel: (o, d) = the primary ray of `constants` (no RNG). Miss: (sky_radiance(o, d, sun, I0, sun disk), 1) with HRPT_DEFERRED_SKY,
 * else (0, 0, 0, 0); I0 = lights[0].m_Intensity (0 with an empty list). Hit: X = o + d * t, V = -d, ior 1.5; lights 0 .. m_LightCount - 1 in
 * order -- directional: L = m_SunDirection, skipped when dot(N, L) <= 0, radiance = sun_radiance(X) with HRPT_DEFERRED_SKY else m_Color *
 * m_Intensity; point / spot: the culls of the path tracer's light sample (intensity, range, spot facing and outer cone), L = normalize(
 * m_Position - X) (m_Radius ignored: hard shadows), skipped when dot(N, L) <= 0, radiance with distance and cone attenuation; other types
 * skipped -- each adding (diffuse, specular) of EvaluateDirectLight times vis, vis = CalculateRTShadow<true>(X, L, maxDist) with
 * HRPT_DEFERRED_SHADOWS else 1. rgb = (sumDiffuse + sumSpecular) + E.rgb; with HRPT_DEFERRED_INDIRECT, where the indirect texel's w == 1,
 * rgb += (((irr.rgb * A.rgb) * (1 - metallic)) * 0.31830988618f) * indirectIntensity; alpha = A.a.
 * Differences from DeferredLighting.hlsl, on purpose: X and V come from the primary ray and t, not from a depth reconstruction at the pixel
 * centre; the sun's shadow goes through CalculateRTShadow<true> like the path tracer's; point lights are lit (the reference's raster loop
 * skips type 1); the CSM mask, IBL, ReSTIR / SHARC / SSGI inputs and the debug views are not reproduced. */
#define HRPT_DEFERRED_SHADOWS  1u   /* one shadow ray per lit (pixel, light) pair through hrpt_trace_rays(HRPT_RAYS_SHADOW) */
#define HRPT_DEFERRED_SKY      2u   /* the atmosphere: sky at misses, sun_radiance(X) for directional lights */
#define HRPT_DEFERRED_INDIRECT 4u   /* add the diffuse indirect image (context call: the plane of hrpt_probes_shade_gbuffer) */
typedef struct HrptDeferredParams {
    uint32_t flags;              /* HRPT_DEFERRED_* */
    float indirectIntensity;     /* finite; read with HRPT_DEFERRED_INDIRECT */
    uint32_t reserved[2];        /* 0 */
} HrptDeferredParams;
typedef struct HrptDeferredImages {
    const float *albedo, *normal, *geoNormal, *emissive, *depth;
    const float *indirect;       /* NULL unless HRPT_DEFERRED_INDIRECT */
    float *colorOut;             /* must differ from every other image */
} HrptDeferredImages;
/* Over the context's own planes into Output (Accumulation is not touched, like hrpt_demodulate). Three steps per batch of B consecutive
 * lights (B = min(m_LightCount, 4); HRPT_DEFERRED_LIGHT_BATCH = 1..16 at hrpt_create overrides it; the result does not depend on B, bit for
 * bit): a kernel writes one HrptRay per (light in batch, pixel) at g = j * W * H + y * W + x (a lit pair: origin X, direction L, tmin 0,
 * tmax maxDist; an unlit pair or a miss: origin = NaN, the rest 0, which hrpt_trace_rays does not trace), hrpt_trace_rays(HRPT_RAYS_SHADOW |
 * HRPT_RAYS_DEVICE_POINTERS) on library-owned buffers (W * H * B records, allocated on first use, dropped by hrpt_resize; skipped without
 * HRPT_DEFERRED_SHADOWS), and a shade kernel that adds the batch's lights into running sums and on the last batch writes Output. The
 * result equals, bit for bit, hrpt_deferred_rays_host -> hrpt_trace_rays -> hrpt_deferred_shade_host through the public calls.
 * Asynchronous on the context stream. No scene: HRPT_ERR_NO_SCENE. hrpt_resize not called, one of the five planes never requested (the
 * message names it), HRPT_DEFERRED_INDIRECT without a probe plane at the current size (the message names hrpt_probes_shade_gbuffer),
 * m_LightCount above the scene's light count, unknown flag bits, non-zero reserved, a non-finite indirectIntensity:
 * HRPT_ERR_INVALID_ARGUMENT. An error changes nothing. */
int  hrpt_deferred_lighting(HrptContext* ctx, const HrptPathTracerConstants* constants, const HrptDeferredParams* params);
/* The same over caller-owned DEVICE images of width x height float4 (16-byte aligned), with the scene, lights and ray buffers of `ctx`;
 * every step runs on `stream` (a hipStream_t; NULL = the default stream). */
int  hrpt_deferred_lighting_device(HrptContext* ctx, const HrptDeferredImages* deviceImages, uint32_t width, uint32_t height,
                                   const HrptPathTracerConstants* constants, const HrptDeferredParams* params, void* stream);
/* The two stages on the host, with no GPU and no scene; same bits as the kernels. `lights` is a host array; constants->m_LightCount is
 * not read (the arguments say which lights).
 * rays: raysOut receives lightCount * width * height records for lights[firstLight .. firstLight + lightCount), laid out as above.
 * shade: all of lights[0 .. lightCount) in one pass. visibility: float [lightCount][height][width], read at lit pairs only, NULL = 1.
 * sunRadiance: a float4 image, rgb = the radiance of a directional light at the pixel's X, NULL = m_Color * m_Intensity. sky: a float4
 * image whose texel is stored at a miss, NULL = (0, 0, 0, 0). The atmosphere terms enter as images because the tables live with a
 * scene; the device path computes them in the kernel. params->flags: only HRPT_DEFERRED_INDIRECT is read (images->indirect required). */
int  hrpt_deferred_rays_host(const HrptDeferredImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants,
                             const HrptGPULight* lights, uint32_t firstLight, uint32_t lightCount, HrptRay* raysOut);
int  hrpt_deferred_shade_host(const HrptDeferredImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants,
                              const HrptGPULight* lights, uint32_t lightCount, const float* visibility, const float* sunRadiance, const float* sky,
                              const HrptDeferredParams* params, int nthreads);

/* ---- traced indirect lighting at the first hit --------------------------------------------------------------------------------------
 * The producer of the reference's SSGI.hlsl -- one GGX-VNDF specular ray and one cosine diffuse ray per pixel from the G-buffer, two
 * demodulated signals for the temporal, denoise and compose passes -- with the screen-space march replaced by path-traced rays
 * (hrpt_trace_radiance with HRPT_RADIANCE_SECONDARY). Additive; HRPT_ABI_VERSION stays 3.
 * One source for kernels and host executors: hobbyrenderer_amd/csrc/pt_indirect.h; DESIGN.md section 29 has every operation in order.
 * Per pixel (x, y), g = y * W + x, over the planes ALBEDO (A), NORMAL (N, roughness in w), GEO_NORMAL (metallic in w), DEPTH (.x = t):
 * (o, d) = the primary ray of `constants` (the ones the G-buffer was rendered with); X = o + d * t, V = -d; s = pcg_hash(g +
 * pcg_hash(frameSeed)), u0..u3 = rng_next(&s). Diffuse record: untraced when !(1 - metallic > 0) or !(dot(N, dirD) > 0), dirD =
 * sample_hemisphere_cosine(u0, u1, N); else origin X, tmin 1e-4f, direction dirD, tmax 1e10f, rng s. Specular record: H =
 * sample_ggx_vndf(u2, u3, N, V, roughness), dirS = reflect(-V, H), wS = eval_ggx_vndf_weight(compute_f0(A.rgb, metallic, 1.5f), N, V, dirS,
 * H, roughness); untraced when !(dot(N, dirS) > 0) or !(maxcomp(wS) > 0); else origin X, tmin 1e-4f, direction dirS, tmax 1e10f, rng
 * pcg_hash(s). An untraced record (every record of a miss): origin = NaN, the rest 0. Diffuse records at [g], specular records at
 * [W * H + g]; with one lobe flagged its records sit at [g]. Resolve: diffuse = (Ld.rgb, 1) where the record's radiance has w == 1, else
 * zeros (DEMODULATED: no albedo, cosine-sampling weight 1); specular = (Ls.rgb * wS, 1), else zeros (carries F * G1). A miss resolves to
 * zeros. Compose, where depth.x != 1e10f: rgb = C.rgb + ((((Dp.rgb * A.rgb) * (1 - metallic)) + Sp.rgb) * intensity); alpha is kept and
 * misses pass through. */
#define HRPT_INDIRECT_DIFFUSE        1u
#define HRPT_INDIRECT_SPECULAR       2u
#define HRPT_INDIRECT_THREAD_PER_RAY 0x200u   /* testing: passed to the trace as HRPT_RADIANCE_THREAD_PER_RAY (same results) */
typedef struct HrptIndirectParams {
    uint32_t flags;              /* HRPT_INDIRECT_*; at least one lobe */
    uint32_t frameSeed;
    float intensity;             /* finite; read by compose */
    uint32_t reserved;           /* 0 */
} HrptIndirectParams;
typedef struct HrptIndirectImages {
    const float *albedo, *normal, *geoNormal, *depth;
    float *diffuse, *specular;   /* lighting / resolve: written (the plane of a lobe that is not flagged may be NULL); compose: read */
    float *colorInOut;           /* compose only; lighting ignores it */
} HrptIndirectImages;            /* a written image must differ from every other image of the call */
/* Over the context's own planes into two library-owned float4 planes (allocated on first use, dropped by hrpt_resize; the plane of a lobe
 * that is not flagged is zeroed): a kernel writes the records, hrpt_trace_radiance(HRPT_RADIANCE_DEVICE_POINTERS | HRPT_RADIANCE_SECONDARY)
 * runs on library-owned buffers and reads m_MaxBounces, m_LightCount and the sun from `constants`, a kernel resolves. The result equals,
 * bit for bit, hrpt_indirect_rays_host -> hrpt_trace_radiance -> hrpt_indirect_resolve_host through the public calls. Accumulation, Output,
 * the G-buffer, histories, exposure and HrptStats are untouched. Asynchronous on the context stream. No scene: HRPT_ERR_NO_SCENE.
 * hrpt_resize not called, one of the four planes never requested (the message names it), no lobe flag, unknown flag bits, non-zero
 * reserved, a non-finite intensity, the argument errors of hrpt_trace_radiance: HRPT_ERR_INVALID_ARGUMENT. An error changes nothing. */
int  hrpt_indirect_lighting(HrptContext* ctx, const HrptPathTracerConstants* constants, const HrptIndirectParams* params);
/* Output.rgb += the composed planes of the last hrpt_indirect_lighting at the current size (before one: HRPT_ERR_INVALID_ARGUMENT). */
int  hrpt_indirect_compose(HrptContext* ctx, const HrptIndirectParams* params);
/* which: 0 = diffuse, 1 = specular. read synchronises; bytes = width * height * 16. */
int  hrpt_read_indirect(HrptContext* ctx, uint32_t which, float* dst, size_t bytes);
int  hrpt_get_indirect_device(HrptContext* ctx, uint32_t which, void** devicePtr);
/* The same over caller-owned DEVICE images of width x height float4 (16-byte aligned), with the scene and ray buffers of `ctx`; every step
 * runs on `stream` (a hipStream_t; NULL = the default stream). Null or aliased images: HRPT_ERR_INVALID_ARGUMENT. */
int  hrpt_indirect_lighting_device(HrptContext* ctx, const HrptIndirectImages* deviceImages, uint32_t width, uint32_t height,
                                   const HrptPathTracerConstants* constants, const HrptIndirectParams* params, void* stream);
int  hrpt_indirect_compose_device(HrptContext* ctx, const HrptIndirectImages* deviceImages, uint32_t width, uint32_t height,
                                  const HrptIndirectParams* params, void* stream);
/* The two kernels around the trace on their own, for a caller that traces the records itself: raysOut receives width * height HrptRay per
 * flagged lobe, radiance4 holds one float4 per record, both DEVICE arrays in the layout above. Neither needs a scene. */
int  hrpt_indirect_rays_device(HrptContext* ctx, const HrptIndirectImages* deviceImages, uint32_t width, uint32_t height,
                               const HrptPathTracerConstants* constants, const HrptIndirectParams* params, HrptRay* raysOut, void* stream);
int  hrpt_indirect_resolve_device(HrptContext* ctx, const HrptIndirectImages* deviceImages, uint32_t width, uint32_t height,
                                  const HrptPathTracerConstants* constants, const HrptIndirectParams* params, const float* radiance4, void* stream);
/* The three stages on the host, with no GPU and no scene; same bits as the kernels. rays: raysOut receives width * height records per
 * flagged lobe, laid out as above (only albedo, normal, geoNormal and depth of `images` are read). resolve: radiance4 holds one float4
 * per record in the same layout. */
int  hrpt_indirect_rays_host(const HrptIndirectImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants,
                             const HrptIndirectParams* params, HrptRay* raysOut, int nthreads);
int  hrpt_indirect_resolve_host(const HrptIndirectImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants,
                                const HrptIndirectParams* params, const float* radiance4, int nthreads);
int  hrpt_indirect_compose_host(const HrptIndirectImages* images, uint32_t width, uint32_t height, const HrptIndirectParams* params,
                                int nthreads);

/* ---- resampled direct lighting (ReSTIR DI) -------------------------------------------------------------------------------------------
 * A direct-light stage whose shadow rays do not grow with the light list: one per pixel whatever m_LightCount is (two with
 * HRPT_RESTIR_INITIAL_VISIBILITY). Candidates are drawn by resampled importance sampling, reused across frames through the motion plane
 * and across neighbouring pixels (pairwise MIS), and the chosen light is shaded into an image of hrpt_deferred_lighting's form; in
 * expectation it equals hrpt_deferred_lighting(HRPT_DEFERRED_SHADOWS). Defined by this project after the published algorithm (Bitterli
 * et al. 2020); parity with the RTXDI SDK is out of scope. Additive; HRPT_ABI_VERSION stays 3.
 * One source for kernels and host executors: hobbyrenderer_amd/csrc/pt_restir.h; DESIGN.md section 30 has every operation in order.
 * Surface S(x, y): the primary ray of `constants`, X = o + d * t, the surface terms of deferred lighting. Target pHat(S, i): 0 when light
 * i is culled at S, else luminance(diffuse + specular) of the unshadowed light, through p > 0 ? p : 0. A reservoir is 16 bytes per pixel;
 * light == HRPT_RESTIR_EMPTY means empty. RNG: sA = pcg_hash(y * W + x + pcg_hash(frameSeed)), sB = pcg_hash(sA), sC = pcg_hash(sB).
 * Four passes: initial (`candidates` uniform draws, W = (wSum / M) / pHat), temporal (the record of the previous pixel q = floor(p + 0.5 +
 * motion.xy), accepted on motion.w == 1, q inside, light < m_LightCount, dot(N, key.xyz) >= normalThreshold and |key.w - (depth.y +
 * motion.z)| <= depthThreshold * (depth.y + motion.z), its M clamped to maxHistory * M), spatial (`spatialSamples` neighbours in a disc of
 * spatialRadius pixels, accepted on the same normal and depth rules, combined with pairwise MIS weights) and shade (rgb = (diffuse +
 * specular) * (W * vis) + E.rgb, alpha = A.a; a miss as in deferred lighting). A pass whose flag is off runs without a partner. The temporal
 * pass is the published biased form under motion (exact for a static frame without jitter); HRPT_RESTIR_INITIAL_VISIBILITY makes the
 * spatial pass biased as well. Light indices must name the same lights between calls: a caller who reorders the list passes
 * HRPT_RESTIR_RESET. */
#define HRPT_RESTIR_SHADOWS            1u    /* the chosen light's shadow ray through hrpt_trace_rays(HRPT_RAYS_SHADOW) */
#define HRPT_RESTIR_SKY                2u    /* the atmosphere: sky at misses, sun_radiance(X) for directional lights */
#define HRPT_RESTIR_TEMPORAL           4u    /* reuse the previous call's reservoirs through the motion plane */
#define HRPT_RESTIR_SPATIAL            8u    /* reuse `spatialSamples` neighbouring reservoirs */
#define HRPT_RESTIR_INITIAL_VISIBILITY 16u   /* a second shadow ray for the initial sample; biased, opt-in */
#define HRPT_RESTIR_RESET              32u   /* ignore (and replace) the history */
#define HRPT_RESTIR_EMPTY              0xFFFFFFFFu
#define HRPT_RESTIR_LDS_MAX_LIGHTS     512   /* up to this many lights the initial pass gathers its candidates from LDS (32 KiB) */
typedef struct HrptRestirParams {
    uint32_t flags;              /* HRPT_RESTIR_* */
    uint32_t frameSeed;
    uint32_t candidates;         /* 1..32; documented default 8 */
    uint32_t spatialSamples;     /* 0..8; default 1 */
    float spatialRadius;         /* pixels, finite, in (0, 65535]; default 32 */
    float maxHistory;            /* finite, > 0; default 20 */
    float depthThreshold;        /* finite; default 0.1 */
    float normalThreshold;       /* finite; default 0.5 */
    uint32_t reserved[4];        /* 0 */
} HrptRestirParams;
typedef struct HrptRestirReservoir {
    uint32_t light;              /* index into the light list, or HRPT_RESTIR_EMPTY */
    float W;                     /* the unbiased contribution weight */
    float M;                     /* the number of candidates the record stands for */
    float pHat;                  /* the target of `light` at the surface that owns the record */
} HrptRestirReservoir;
typedef struct HrptRestirImages {
    const float *albedo, *normal, *geoNormal, *emissive, *depth;
    const float *motion;                       /* hrpt_render_motion_vectors' plane; NULL unless HRPT_RESTIR_TEMPORAL */
    const HrptRestirReservoir *reservoirIn;    /* the history: the previous call's reservoirOut, or NULL */
    const float *keyIn;                        /* ... and its keyOut (N.xyz, view depth), or NULL */
    HrptRestirReservoir *reservoirOut;         /* width * height records */
    float *keyOut;                             /* float4 image */
    float *colorOut;                           /* float4 image; must differ from every other image */
} HrptRestirImages;
/* Over the context's own planes into Output: initial -> [trace] -> temporal -> spatial -> [trace] -> shade on the context stream, each
 * trace one hrpt_trace_rays(HRPT_RAYS_SHADOW | HRPT_RAYS_DEVICE_POINTERS) of width * height records. Reservoirs, keys, ray and hit records
 * are library-owned (allocated on first use, dropped by hrpt_resize); the history is also dropped by HRPT_RESTIR_RESET. The result equals,
 * bit for bit, hrpt_restir_initial_host -> hrpt_trace_rays -> hrpt_restir_temporal_host -> hrpt_restir_spatial_host -> hrpt_trace_rays ->
 * hrpt_restir_shade_host through the public calls. Accumulation, the G-buffer, the motion plane, the other histories, exposure and
 * HrptStats are untouched. No scene: HRPT_ERR_NO_SCENE. hrpt_resize not called, a plane never requested (the message names it; the motion
 * plane with HRPT_RESTIR_TEMPORAL), m_LightCount above the scene's light count, candidates or spatialSamples out of range, a radius or
 * history that is not finite and positive, a threshold that is not finite, unknown flag bits, non-zero reserved:
 * HRPT_ERR_INVALID_ARGUMENT. An error changes nothing. */
int  hrpt_restir_lighting(HrptContext* ctx, const HrptPathTracerConstants* constants, const HrptRestirParams* params);
/* The last call's final reservoirs, width * height records (synchronises); and the device addresses of them and of their key plane (NULL
 * before the first call, after a resize). */
int  hrpt_read_restir_reservoirs(HrptContext* ctx, HrptRestirReservoir* dst, size_t bytes);
int  hrpt_get_restir_device(HrptContext* ctx, void** reservoirs, void** keys);
/* The same over caller-owned DEVICE images (16-byte aligned), with the scene, lights and ray buffers of `ctx`, every step on `stream` (a
 * hipStream_t; NULL = the default stream). The history is reservoirIn / keyIn (both NULL = none). Null or aliased images:
 * HRPT_ERR_INVALID_ARGUMENT. */
int  hrpt_restir_lighting_device(HrptContext* ctx, const HrptRestirImages* deviceImages, uint32_t width, uint32_t height,
                                 const HrptPathTracerConstants* constants, const HrptRestirParams* params, void* stream);
/* The four kernels on their own, over DEVICE arrays; the lights are the context's. initial: writes images->reservoirOut, and with
 * HRPT_RESTIR_INITIAL_VISIBILITY one HrptRay per pixel into raysOut (an empty reservoir: origin = NaN, the rest 0). temporal: reads
 * `initial`, its hit records (NULL unless HRPT_RESTIR_INITIAL_VISIBILITY), the history and images->motion, writes images->reservoirOut.
 * spatial: reads `temporal`, writes images->reservoirOut, images->keyOut and, when raysOut is not NULL, the chosen light's HrptRay.
 * shade: reads `final` and the hit records of those rays (NULL = visibility 1), writes images->colorOut. All four need a scene: its light
 * buffer, and its atmosphere tables with HRPT_RESTIR_SKY. An output must differ from every array the pass reads. */
int  hrpt_restir_initial_device(HrptContext* ctx, const HrptRestirImages* deviceImages, uint32_t width, uint32_t height,
                                const HrptPathTracerConstants* constants, const HrptRestirParams* params, HrptRay* raysOut, void* stream);
int  hrpt_restir_temporal_device(HrptContext* ctx, const HrptRestirImages* deviceImages, uint32_t width, uint32_t height,
                                 const HrptPathTracerConstants* constants, const HrptRestirParams* params, const HrptRestirReservoir* initial,
                                 const HrptRayHit* initialHits, void* stream);
int  hrpt_restir_spatial_device(HrptContext* ctx, const HrptRestirImages* deviceImages, uint32_t width, uint32_t height,
                                const HrptPathTracerConstants* constants, const HrptRestirParams* params, const HrptRestirReservoir* temporal,
                                HrptRay* raysOut, void* stream);
int  hrpt_restir_shade_device(HrptContext* ctx, const HrptRestirImages* deviceImages, uint32_t width, uint32_t height,
                              const HrptPathTracerConstants* constants, const HrptRestirParams* params, const HrptRestirReservoir* final,
                              const HrptRayHit* hits, void* stream);
/* The four passes on the host, with no GPU and no scene; same bits as the kernels. `lights` is a host array of constants->m_LightCount
 * records. sunRadiance: a float4 image, rgb = the radiance of a directional light at the pixel's X, NULL = m_Color * m_Intensity. sky: a
 * float4 image whose texel is stored at a miss, NULL = (0, 0, 0, 0). initialVisibility / visibility: float [height][width], NULL = 1. */
int  hrpt_restir_initial_host(const HrptRestirImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants,
                              const HrptGPULight* lights, const HrptRestirParams* params, const float* sunRadiance, HrptRay* raysOut, int nthreads);
int  hrpt_restir_temporal_host(const HrptRestirImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants,
                               const HrptGPULight* lights, const HrptRestirParams* params, const float* sunRadiance,
                               const HrptRestirReservoir* initial, const float* initialVisibility, int nthreads);
int  hrpt_restir_spatial_host(const HrptRestirImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants,
                              const HrptGPULight* lights, const HrptRestirParams* params, const float* sunRadiance,
                              const HrptRestirReservoir* temporal, HrptRay* raysOut, int nthreads);
int  hrpt_restir_shade_host(const HrptRestirImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants,
                            const HrptGPULight* lights, const HrptRestirParams* params, const float* sunRadiance, const float* sky,
                            const HrptRestirReservoir* final, const float* visibility, int nthreads);

/* ---- world-space hash-grid radiance cache ----------------------------------------------------------------------------------------------
 * Ends the diffuse indirect path after one segment: a sparse set of pixels (one per sparseBlock x sparseBlock block) feeds path-traced
 * radiance into a spatial hash table each frame, and every pixel then traces one cosine ray and reads the radiance at its hit point from the
 * table. The counterpart of the reference's SHARCUpdate.hlsl, SharcResolve.hlsl and SHARCQuery.hlsl; the SDK headers behind them are not in
 * the reference tree, so the stage is DEFINED by this project after the published description. Additive; HRPT_ABI_VERSION stays 3.
 * One source for kernels and host executors: hobbyrenderer_amd/csrc/pt_rcache.h; DESIGN.md section 32 has every operation in order.
 * Not here: parity with the SDK's packing and constants, cache resampling and the four-vertex back-propagation (the value stored is the path
 * tracer's full estimate along the ray, so the cache has no feedback from its own last state and no energy clamp), re-levelling entries when
 * the camera moves (entries of a changed level go stale and are rebuilt), a specular lookup, sharding the table over several GPUs, the C++
 * plugin mirror and a wavefront route for the surface query.
 *
 * Table. capacity = 2^capacityLog2 entries in three arrays: keys (uint64, 0 = empty), accumulation (HrptRcacheAccum: the integer sums of
 * one frame) and resolved (HrptRcacheEntry: the running mean; meta = samples | stale << 16). For a point p with normal n and camera c:
 * level = clamp(floor(0.5 * log2(max(|p - c|^2, FLT_MIN)) + levelBias), 1, 1023), voxel = exp2(level) / (sceneScale * exp2(levelBias)),
 * grid = floor(p / voxel) per component (17 bits each, two's complement, wrapped), key = gx | gy << 17 | gz << 34 | level << 51 |
 * octant << 61 with octant bit k = (n[k] >= 0). Its bucket is the 32 consecutive entries at (pcg(lo + pcg(hi)) mod (capacity / 32)) * 32;
 * the occupied slots of a bucket are always a prefix of it. Valid desc: capacityLog2 10..26; sceneScale and radianceScale finite and > 0;
 * levelBias in [-64, 64]; maxSamples 1..65535; staleFramesMax <= 65534; sparseBlock 1..16; roughnessThreshold finite. The reference's
 * constants: 22, 50, 0, 1e3, 60, 64, 5, 0.1. */
typedef struct HrptRcacheDesc {
    uint32_t capacityLog2;
    float sceneScale, levelBias, radianceScale;
    uint32_t maxSamples, staleFramesMax, sparseBlock;
    float roughnessThreshold;
} HrptRcacheDesc;                                                                                                          /* 32 B */
typedef struct HrptRcacheAccum { uint64_t r, g, b; uint32_t count; uint32_t pad; } HrptRcacheAccum;                       /* 32 B */
typedef struct HrptRcacheEntry { float r, g, b; uint32_t meta; } HrptRcacheEntry;                                         /* 16 B */
typedef struct HrptRcacheSample { float position[3]; float valid; float normal[3]; float pad0; float radiance[3]; float pad1; } HrptRcacheSample;   /* 48 B */
typedef struct HrptRcachePoint { float position[3]; float pad0; float normal[3]; float pad1; } HrptRcachePoint;           /* 32 B */
typedef struct HrptRcacheSurface { float position[3]; float t; float normal[3]; uint32_t hit; uint32_t rng; uint32_t pad[3]; } HrptRcacheSurface;   /* 48 B */
typedef struct HrptRcacheParams {
    uint32_t flags;              /* HRPT_RCACHE_NO_FALLBACK or 0 */
    uint32_t frameSeed;          /* of the diffuse records, as HrptIndirectParams::frameSeed */
    uint32_t reserved[2];        /* 0 */
} HrptRcacheParams;
typedef struct HrptRcache HrptRcache;
#define HRPT_RCACHE_RESET           1u   /* update / resolve: empty the table (update: before this frame's samples go in) */
#define HRPT_RCACHE_NO_FALLBACK     2u   /* indirect: pixels the cache does not serve get zeros instead of a traced path (the reference's behaviour) */
#define HRPT_RCACHE_NO_WAVE_COMBINE 4u   /* update / insert: one set of atomics per sample instead of per (wave, key); same table, the cross-check */
/* A cache on `ctx` with an empty table. Destroy it before its context. hrpt_rcache_destroy(NULL) is allowed. */
int  hrpt_rcache_create(HrptContext* ctx, const HrptRcacheDesc* desc, HrptRcache** out);
void hrpt_rcache_destroy(HrptRcache* cache);
/* One frame of filling. Per block (bx, by) of sparseBlock^2 pixels the pixel (bx * B + pcg(bx ^ by << 16 ^ frameIndex) % B, by * B +
 * pcg(by ^ bx << 16 ^ (frameIndex + 1)) % B), when inside the image, gets the diffuse record of hrpt_indirect_lighting with frameSeed =
 * frameIndex over the context's G-buffer planes (ALBEDO, NORMAL, GEO_NORMAL, DEPTH, as rendered with `constants`); it is untraced as there
 * (a miss, !(1 - metallic > 0), a direction below the surface) and also when roughness < roughnessThreshold. On those records, in order:
 * hrpt_rcache_surfaces_device, hrpt_trace_radiance(DEVICE_POINTERS | SECONDARY), the insert of (surface, L) where the ray hit and the
 * radiance has w == 1, and the resolve. The camera position of the keys is constants->m_CameraPos. Asynchronous on the context stream;
 * Accumulation, Output, every plane and history, exposure and HrptStats stay as they were. No scene: HRPT_ERR_NO_SCENE. hrpt_resize not
 * called, a plane never requested (the message names it), unknown flag bits, a camera position that is not finite, the argument errors of
 * hrpt_trace_radiance: HRPT_ERR_INVALID_ARGUMENT. An error leaves the table as it was. */
int  hrpt_rcache_update(HrptRcache* cache, const HrptPathTracerConstants* constants, uint32_t frameIndex, uint32_t flags);
/* Writes the context's indirect DIFFUSE plane (the plane and the demodulated form of hrpt_indirect_lighting(HRPT_INDIRECT_DIFFUSE), so
 * hrpt_indirect_compose, the temporal, denoise and upscale stages work on it unchanged; the specular plane is left as it is; planes that
 * do not exist at this size are allocated zeroed). In order: the full-resolution diffuse records of hrpt_indirect_rays_device for
 * params->frameSeed, hrpt_rcache_surfaces_device, the query at every hit; a pixel is SERVED when its ray hit, the key was found with
 * samples > 0 and t >= voxel (the segment spans the voxel, so no surface reads its own voxel); a served pixel's record is overwritten with
 * the untraced record and the pixel gets (cached.rgb, 1); every other record goes through hrpt_trace_radiance(SECONDARY) and the diffuse
 * resolve as in hrpt_indirect_lighting (skipped with HRPT_RCACHE_NO_FALLBACK: zeros). A second library-owned plane receives (cached.rgb, 1)
 * at served pixels and zeros elsewhere. The table is not changed. Errors as hrpt_indirect_lighting; an error changes nothing. */
int  hrpt_rcache_indirect(HrptRcache* cache, const HrptPathTracerConstants* constants, const HrptRcacheParams* params);
/* Host read-back of the served plane (synchronises; bytes = width * height * 16; before the first hrpt_rcache_indirect at this size:
 * HRPT_ERR_INVALID_ARGUMENT). */
int  hrpt_read_rcache_served(HrptContext* ctx, float* dst, size_t bytes);
/* Empties the table and zeroes the drop counter; asynchronous on the context stream. */
int  hrpt_rcache_clear(HrptRcache* cache);
/* The table: host read-back (synchronises), device pointers (valid until hrpt_rcache_destroy; dropsOut: one uint64, the samples lost to
 * full buckets since creation / clear) and hrpt_rcache_write, which installs a table (tests, baked caches; synchronises). `entries` must
 * equal the capacity; any pointer may be NULL (skipped), but write takes keys, accumulation and resolved together and refuses, with
 * HRPT_ERR_INVALID_ARGUMENT, a table in which a key sits outside its bucket or twice, an empty slot precedes an occupied one or an empty
 * slot's records are not zero. */
int  hrpt_rcache_read(HrptRcache* cache, uint64_t* keys, HrptRcacheAccum* accumulation, HrptRcacheEntry* resolved, uint64_t entries, uint64_t* dropsOut);
int  hrpt_rcache_write(HrptRcache* cache, const uint64_t* keys, const HrptRcacheAccum* accumulation, const HrptRcacheEntry* resolved, uint64_t entries);
int  hrpt_rcache_get_device(HrptRcache* cache, void** keys, void** accumulation, void** resolved, void** drops);
/* Position and geometric normal where rays land: surfacesOut[i] = (o + d * t, t, Ng facing the ray, hit 1, the advanced RNG state) for the
 * closest hit of rays[i] under the rules of hrpt_trace_rays(HRPT_RAYS_CLOSEST) (same t and rng, bit for bit), zeros with hit 0 and the
 * ray's rng at a miss or a ray that is not finite. Ng = normalize(the interpolated world normal), negated when dot(Ng, d) > 0. DEVICE arrays,
 * 16-byte aligned; asynchronous on `stream`. No scene: HRPT_ERR_NO_SCENE; more than 2^31 rays or a two-level structure deeper than the
 * thread-per-query kernels' stack: HRPT_ERR_INVALID_ARGUMENT. */
int  hrpt_rcache_surfaces_device(HrptContext* ctx, const HrptRay* rays, HrptRcacheSurface* surfacesOut, uint64_t count, void* stream);
/* The table stages alone over caller-owned arrays of 2^capacityLog2 entries: with no context (_host: host threads, nthreads <= 0 = one per
 * hardware thread up to 16) or on device memory (_device: asynchronous on `stream`). cameraPos: three finite floats in HOST memory, read before the call returns.
 * insert: per used sample (valid == 1, position and normal finite; any other sample is skipped and not counted) the bucket is walked from
 * slot 0 with a compare-and-swap on the key and stops at the first slot that was empty or holds the key; that slot's sums get
 * (uint64)min(max(L, 0) * radianceScale, 4294967040) per channel (a NaN adds 0) and its count 1. A sample that finds its bucket full adds
 * 1 to *drops and is lost. Which slot of a bucket a key lands in depends on the order of arrival; the sums do not.
 * resolve (no insert may run concurrently): per occupied entry with n = count > 0: No = min(samples, maxSamples), mean = (old * No + sum /
 * radianceScale) / (No + n), samples = min(No + n, maxSamples), stale = 0; with n == 0: stale += 1, above staleFramesMax the entry is
 * evicted. The survivors of a bucket move to its front in their old order, the accumulation is zeroed and freed slots are zeroed.
 * HRPT_RCACHE_RESET empties the table instead.
 * query: out4[i] = (resolved.rgb, 1) when the key of points[i] is present with samples > 0, else zeros; the walk ends at the first empty
 * slot; voxelOut (may be NULL) receives the voxel size at the point (0 for a point or normal that is not finite). */
int  hrpt_rcache_insert_host(const HrptRcacheDesc* desc, const float* cameraPos, uint64_t* keys, HrptRcacheAccum* accumulation, uint64_t* drops,
                             const HrptRcacheSample* samples, uint64_t count, int nthreads);
int  hrpt_rcache_insert_device(HrptContext* ctx, const HrptRcacheDesc* desc, const float* cameraPos, uint64_t* keys, HrptRcacheAccum* accumulation,
                               uint64_t* drops, const HrptRcacheSample* samples, uint64_t count, uint32_t flags, void* stream);
int  hrpt_rcache_resolve_host(const HrptRcacheDesc* desc, uint64_t* keys, HrptRcacheAccum* accumulation, HrptRcacheEntry* resolved, uint32_t flags,
                              int nthreads);
int  hrpt_rcache_resolve_device(HrptContext* ctx, const HrptRcacheDesc* desc, uint64_t* keys, HrptRcacheAccum* accumulation, HrptRcacheEntry* resolved,
                                uint32_t flags, void* stream);
int  hrpt_rcache_query_host(const HrptRcacheDesc* desc, const float* cameraPos, const uint64_t* keys, const HrptRcacheEntry* resolved,
                            const HrptRcachePoint* points, float* out4, float* voxelOut, uint64_t count, int nthreads);
int  hrpt_rcache_query_device(HrptContext* ctx, const HrptRcacheDesc* desc, const float* cameraPos, const uint64_t* keys, const HrptRcacheEntry* resolved,
                              const HrptRcachePoint* points, float* out4, float* voxelOut, uint64_t count, void* stream);

/* Intra-frame overlap: by default the shadow stage of bounce b runs on a second, library-owned stream next to the traversal of bounce
 * b + 1 (they share no buffer). That fills the tails of a context that renders one frame at a time (-3 % per frame). A host that keeps
 * two frames in flight on two contexts already fills those tails with the other frame; there the fork / join events only cost
 * (-5 % per frame with the overlap off at full size, -13 % for an eighth of the picture): pass 0. Takes effect at the next hrpt_render. */
int  hrpt_set_shadow_overlap(HrptContext* ctx, int enabled);

int  hrpt_get_stats(HrptContext* ctx, HrptStats* out);      /* synchronises; ray counters are cumulative */
int  hrpt_reset_stats(HrptContext* ctx);
/* Device self-test of the acceleration structure: *violations = number of child boxes (2-wide tree and its 4-wide collapse) that do
 * not contain the boxes / triangle vertices below them. 0 for a sound tree; anything else means missed hits. Synchronises. */
int  hrpt_selftest_bvh(HrptContext* ctx, uint64_t* violations);
/* Read-back of an acceleration structure for host-side validation (tests/bvh_reference.py): the records exactly as the kernels read them
 * (layouts: hobbyrenderer_amd/csrc/pt_scene_records.h GpuNode 64 B, GpuNode4 128 B, GpuNodeQ 64 B, GpuTri 48 B, GpuTriAttr 80 B, GpuTriTangent 48 B,
 * GpuInstance 128 B). Size query, then fill: every call writes the counts; an array pointer that is not NULL receives that array and must
 * have room for the count the query reported (nodes: nodeCount, nodes4 / nodesQ: node4Count, triangles / attributes / tangents:
 * triangleCount, instances: instanceCount). Flat structure: the 2-wide tree, its 4-wide collapse, the quantised nodes (hasNodesQ).
 * Two-level structure: nodeCount = 0, nodes4 = the instance tree ([0, instanceNodeCount), root 0 or rootLeaf) followed by the mesh trees,
 * triangles in object space (inst = mesh index). */
typedef struct HrptBvhDump {
    uint32_t structure;                     /* HRPT_ACCEL_FLAT or HRPT_ACCEL_TWO_LEVEL */
    uint32_t nodeCount, node4Count, triangleCount, instanceCount, instanceNodeCount;
    int32_t  rootLeaf;                      /* encoded leaf when the tree (two-level: the instance tree) has no node, else 0 */
    uint32_t hasNodesQ, hasTangents;
    uint32_t maxDepth, maxDepth4;           /* as reported by the builder (two-level: maxDepth4 = maxDepth4Tlas + maxDepth4Blas) */
    uint32_t maxDepth4Tlas, maxDepth4Blas;  /* two-level: LEVELS of the instance tree / of the deepest mesh tree (depth + 1; 0 = no node) */
    float    sahCost;
    uint32_t nodes4Capacity, nodesQCapacity;/* records the device allocations behind nodes4 / nodesQ hold (0: allocated to size / absent) */
    void*    nodes; void* nodes4; void* nodesQ; void* triangles; void* attributes; void* tangents; void* instances;
} HrptBvhDump;                              /* 64 B + 7 pointers */
/* The structure the kernels of `ctx` currently walk. Waits for frames in flight; changes nothing. */
int  hrpt_selftest_read_bvh(HrptContext* ctx, HrptBvhDump* dump);
/* The host builder alone, without a context or a device: builds `scene` (structure: HRPT_ACCEL_FLAT or HRPT_ACCEL_TWO_LEVEL) and
 * returns it in the same form (size query, then fill: the tree is built by every call, and is deterministic). A scene that the builder
 * refuses answers HRPT_ERR_INVALID_ARGUMENT with the reason in hrpt_last_error(NULL). */
#define HRPT_HOST_BUILD_SEPARATE_COLLAPSE 1u   /* flat only: nodes4 by collapse_bvh2_on_host over the finished 2-wide tree instead of the builder's own collapse */
int  hrpt_selftest_host_build(const HrptSceneDesc* scene, uint32_t structure, uint32_t flags, HrptBvhDump* dump);
/* Device self-test: out65536[i] = the kernels' decode of the binary16 bit pattern i (RGBA16F LUT texels). */
int  hrpt_selftest_f16_decode(HrptContext* ctx, float* out65536);
/* out512[i] = the kernels' RGBA8_UNORM channel decode of byte i (i < 256); out512[256 + i] = (float)i / 255.0f computed on the device. */
int  hrpt_selftest_unorm8(HrptContext* ctx, float* out512);
/* Device self-test of texture sampling over the uploaded scene's own texture and material tables (tests/texture_reference.py states the
 * same filtering in float64): one thread per probe calls the shader's sampling functions as they are. A probe names a material of the
 * scene, a uv, the gradients of a SampleGrad and the texture-flag mask the shader would pass. Slots are ordered albedo, roughness-metallic,
 * emissive, normal. single[k]: the slot's texture through the one-by-one path (SampleLevel at level 0) when its flag is in texFlags, else
 * zeros; batched[k]: the same four through the batched fetch of the shade kernels, batchedAccepted saying whether it took the material
 * (8-bit formats only; when 0, batched holds zeros); grad: the albedo texture through SampleGrad with ddx / ddy, whatever texFlags says
 * (zeros when the material's albedo index names no texture). probes / results are host arrays; count == 0 does nothing. Synchronises. */
typedef struct HrptTextureProbe { uint32_t material; float uv[2], ddx[2], ddy[2]; uint32_t texFlags; } HrptTextureProbe;                /* 32 B */
typedef struct HrptTextureProbeResult { float single[4][4]; float batched[4][4]; uint32_t batchedAccepted, pad[3]; float grad[4]; } HrptTextureProbeResult;   /* 160 B */
int  hrpt_selftest_sample_textures(HrptContext* ctx, const HrptTextureProbe* probes, HrptTextureProbeResult* results, uint64_t count);
/* Device self-test of the run-time atmosphere lookups over the uploaded scene's RGBA16F tables (tests/atmosphere_reference.py states the
 * same lookups in float64): one thread per probe calls the device functions the miss and sun-light code calls, as they are. cameraPos is a
 * world position in metres, viewRay and sunDir unit vectors. sky: the sky radiance along viewRay (with the sun disk when addSunDisk is
 * non-zero); sun: the sun's radiance arriving at cameraPos; transmittance: the table lookup towards the top of the atmosphere for
 * r = that position's distance from the planet's centre in km and mu = the cosine between its zenith and viewRay, both returned too
 * (the lookup is made with them as they are, also below the ground and above the atmosphere, where the addressing clamps).
 * probes / results are host arrays; count == 0 does nothing. Synchronises. */
typedef struct HrptAtmosphereProbe { float cameraPos[3], viewRay[3], sunDir[3]; float sunIntensity; uint32_t addSunDisk, pad; } HrptAtmosphereProbe;   /* 48 B */
typedef struct HrptAtmosphereProbeResult { float sky[3], sun[3], transmittance[3], r, mu, pad; } HrptAtmosphereProbeResult;                          /* 48 B */
int  hrpt_selftest_atmosphere(HrptContext* ctx, const HrptAtmosphereProbe* probes, HrptAtmosphereProbeResult* results, uint64_t count);

/* Host-side helpers of PathTracerRenderer::Render, exported so that callers in other languages
 * produce the same constants: Halton (src/Utilities.cpp:67-79) and the CB fill (:58-75). */
float hrpt_halton(uint32_t index, uint32_t base);

/* Producer of stand-ins for bin/bruneton/{transmittance,scattering,irradiance}.dat, which the reference loads
 * (src/CommonResources.cpp:519-569) but does not ship: raw float32 RGBA tables of 256*64, 256*128*32 and 64*16 texels from
 * the constants of src/shaders/Atmosphere.hlsli:41-75, following Bruneton's 2017 precomputation: transmittance, single
 * scattering, and `orders` - 1 further scattering orders (scattering density, indirect ground irradiance, multiple
 * scattering; ground albedo 0.1). irradiance may be NULL. hrpt_precompute_atmosphere computes 4 orders (Bruneton's demo value;
 * what the reference's files hold is unknown) on the current HIP device when there is one, else on host threads;
 * the _ex form chooses: orders 1..8 (1 = single scattering only, zero irradiance table), device -1 = host threads, >= 0 = that HIP
 * device, -2 = automatic. The tables are bit-identical whichever executor computed them (one __host__ __device__ source in the
 * arithmetic of hobbyrt/detmath.h). Four orders: ~0.1 s on an MI355X, ~40 s on 8 host threads. */
int  hrpt_precompute_atmosphere(float* transmittance, float* scattering, float* irradiance, int nthreads);
int  hrpt_precompute_atmosphere_ex(float* transmittance, float* scattering, float* irradiance, int orders, int nthreads, int device);
/* Test hook: texels [first, first + count) of one pass (0 transmittance, 1 direct irradiance, 2 single scattering, 3 scattering density,
 * 4 indirect irradiance, 5 multiple scattering; any other id is refused) of order `order` (passes 3 to 5) from full-size tables in host
 * memory (3 floats per texel; transmittance / scattering4: 4), by host threads (device < 0) or on HIP device `device`. Every pointer must
 * be non-null whatever the pass reads. `out` receives the texels of the pass's own table, 3 floats per texel (passes 1 and 4: 64 x 16,
 * passes 3 and 5: 256 x 128 x 32); pass 0 writes the 256 x 64 transmittance table there with 4 floats per texel and reads no table.
 * Pass 2 leaves `out` alone and writes its three outputs in place: scattering4 (rgb Rayleigh, a red Mie), deltaRayleigh and deltaMie.
 * Pass 5 also adds its texels, divided by the Rayleigh phase function, to scattering4. */
int  hrpt_atmosphere_pass(int pass, int order, uint32_t first, uint32_t count, const float* transmittance, const float* deltaIrradiance,
                          float* deltaRayleigh, float* deltaMie, const float* deltaDensity, const float* deltaMultiple,
                          float* scattering4, float* out, int nthreads, int device);

#ifdef __cplusplus
} /* extern "C" */
#endif

#if defined(__cplusplus)
static_assert(sizeof(HrptVertexQuantized) == 24, "VertexQuantized");
static_assert(sizeof(HrptMeshData) == 164, "MeshData");
static_assert(sizeof(HrptPerInstanceData) == 160, "PerInstanceData");
static_assert(sizeof(HrptMaterialConstants) == 180, "MaterialConstants");
static_assert(sizeof(HrptGPULight) == 64, "GPULight");
static_assert(sizeof(HrptPlanarViewConstants) == 704, "PlanarViewConstants");
static_assert(sizeof(HrptPathTracerConstants) == 768, "PathTracerConstants");
#else
_Static_assert(sizeof(HrptVertexQuantized) == 24, "VertexQuantized");
_Static_assert(sizeof(HrptMeshData) == 164, "MeshData");
_Static_assert(sizeof(HrptPerInstanceData) == 160, "PerInstanceData");
_Static_assert(sizeof(HrptMaterialConstants) == 180, "MaterialConstants");
_Static_assert(sizeof(HrptGPULight) == 64, "GPULight");
_Static_assert(sizeof(HrptPlanarViewConstants) == 704, "PlanarViewConstants");
_Static_assert(sizeof(HrptPathTracerConstants) == 768, "PathTracerConstants");
#endif

#endif /* HOBBYRT_PT_H */
