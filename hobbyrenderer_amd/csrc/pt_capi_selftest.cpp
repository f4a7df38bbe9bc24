// pt_capi_selftest.cpp -- the hrpt_selftest_* entry points: device decode tables, BVH checks and read-back, the host builders, texture and atmosphere probes.
#include "pt_capi_internal.h"

using namespace hrt;
using namespace hrt::capi;

int hrpt_selftest_f16_decode(HrptContext* c, float* out65536)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!out65536) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_f16_decode: null out");
    HIP_TRY(c, hipSetDevice(c->device));
    DeviceBuffer<float> d;
    HIP_TRY(c, d.alloc(65536 * sizeof(float)));
    hipError_t e = launch_f16_table(d, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out65536, d, 65536 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, HRPT_ERR_HIP, std::string("hrpt_selftest_f16_decode: ") + hipGetErrorString(e));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_selftest_f16_decode"); }

int hrpt_selftest_bvh(HrptContext* c, uint64_t* violations)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!violations) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_bvh: null out");
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, "hrpt_selftest_bvh: no scene uploaded");
    if (c->view.instances) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_bvh: not available on the two-level structure (hrpt_set_acceleration_structure)");
    HIP_TRY(c, hipSetDevice(c->device));
    DeviceBuffer<unsigned long long> d;
    HIP_TRY(c, d.alloc(sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d, 0, sizeof(unsigned long long), c->stream);
    if (e == hipSuccess) e = launch_bvh_check(c->view, d, c->stream);
    unsigned long long h = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&h, d, sizeof h, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, HRPT_ERR_HIP, std::string("hrpt_selftest_bvh: ") + hipGetErrorString(e));
    *violations = h;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_selftest_bvh"); }

int hrpt_selftest_read_bvh(HrptContext* c, HrptBvhDump* d)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!d) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_read_bvh: null dump");
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, "hrpt_selftest_read_bvh: no scene uploaded");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const SceneView& v = c->view;
    const bool twoLevel = v.instances != nullptr;
    d->structure = twoLevel ? HRPT_ACCEL_TWO_LEVEL : HRPT_ACCEL_FLAT;
    d->nodeCount = twoLevel ? 0u : v.nodeCount; d->node4Count = v.node4Count; d->triangleCount = v.triCount;
    d->instanceCount = twoLevel ? v.instanceCount : 0u; d->instanceNodeCount = twoLevel ? v.nodeCount : 0u;
    d->rootLeaf = v.rootLeaf; d->hasNodesQ = v.nodesQ ? 1u : 0u; d->hasTangents = v.tangents ? 1u : 0u;
    d->maxDepth = c->buildInfo.maxDepth; d->maxDepth4 = c->buildInfo.maxDepth4;
    d->maxDepth4Tlas = twoLevel && c->twoLevel ? c->twoLevel->maxDepth4Tlas : 0u; d->maxDepth4Blas = twoLevel && c->twoLevel ? c->twoLevel->maxDepth4Blas : 0u;
    d->sahCost = c->buildInfo.sahCost;
    d->nodes4Capacity = twoLevel ? 0u : c->nodes4Capacity; d->nodesQCapacity = v.nodesQ ? (uint32_t)(c->nodesQ.bytes() / sizeof(GpuNodeQ)) : 0u;
    auto fetch = [&](void* dst, const void* src, size_t bytes) { return (dst && src && bytes) ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess; };
    HIP_TRY(c, fetch(d->nodes, twoLevel ? nullptr : v.nodes, (size_t)d->nodeCount * sizeof(GpuNode)));
    HIP_TRY(c, fetch(d->nodes4, v.nodes4, (size_t)v.node4Count * sizeof(GpuNode4)));
    HIP_TRY(c, fetch(d->nodesQ, v.nodesQ, (size_t)v.node4Count * sizeof(GpuNodeQ)));
    HIP_TRY(c, fetch(d->triangles, v.tris, (size_t)v.triCount * sizeof(GpuTri)));
    HIP_TRY(c, fetch(d->attributes, v.attrs, (size_t)v.triCount * sizeof(GpuTriAttr)));
    HIP_TRY(c, fetch(d->tangents, v.tangents, (size_t)v.triCount * sizeof(GpuTriTangent)));
    HIP_TRY(c, fetch(d->instances, v.instances, (size_t)d->instanceCount * sizeof(GpuInstance)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_selftest_read_bvh"); }

int hrpt_selftest_host_build(const HrptSceneDesc* scene, uint32_t structure, uint32_t flags, HrptBvhDump* d)
try {
    if (!scene || !d) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_host_build: null argument");
    if ((structure != HRPT_ACCEL_FLAT && structure != HRPT_ACCEL_TWO_LEVEL) || (flags & ~HRPT_HOST_BUILD_SEPARATE_COLLAPSE) ||
        (flags && structure != HRPT_ACCEL_FLAT)) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_host_build: structure / flags");
    std::string berr;
    auto put = [](void* dst, const void* src, size_t bytes) { if (dst && bytes) memcpy(dst, src, bytes); };
    d->structure = structure; d->hasNodesQ = 0; d->nodes4Capacity = 0; d->nodesQCapacity = 0;
    if (structure == HRPT_ACCEL_FLAT) {
        BuiltBvh b;
        if (!build_scene_bvh(*scene, b, berr)) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: " + berr);
        if ((flags & HRPT_HOST_BUILD_SEPARATE_COLLAPSE) && !b.nodes.empty()) collapse_bvh2_on_host(b.nodes, b.nodes4, b.maxDepth4);
        d->nodeCount = (uint32_t)b.nodes.size(); d->node4Count = (uint32_t)b.nodes4.size(); d->triangleCount = (uint32_t)b.tris.size();
        d->instanceCount = 0; d->instanceNodeCount = 0; d->rootLeaf = b.rootLeaf; d->hasTangents = b.tangents.empty() ? 0u : 1u;
        d->maxDepth = b.maxDepth; d->maxDepth4 = b.maxDepth4; d->maxDepth4Tlas = 0; d->maxDepth4Blas = 0; d->sahCost = b.sahCost;
        put(d->nodes, b.nodes.data(), b.nodes.size() * sizeof(HostNode)); put(d->nodes4, b.nodes4.data(), b.nodes4.size() * sizeof(HostNode4));
        put(d->triangles, b.tris.data(), b.tris.size() * sizeof(HostTri)); put(d->attributes, b.attrs.data(), b.attrs.size() * sizeof(HostTriAttr));
        put(d->tangents, b.tangents.data(), b.tangents.size() * sizeof(HostTriTangent));
        return HRPT_OK;
    }
    BuiltTwoLevel b;
    if (!build_scene_two_level(*scene, b, berr)) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: " + berr);
    d->nodeCount = 0; d->node4Count = (uint32_t)b.nodes4.size(); d->triangleCount = (uint32_t)b.tris.size();
    d->instanceCount = (uint32_t)b.instances.size(); d->instanceNodeCount = b.tlasNodeCount; d->rootLeaf = b.tlasRootLeaf; d->hasTangents = b.tangents.empty() ? 0u : 1u;
    d->maxDepth = 0; d->maxDepth4 = b.maxDepth4Tlas + b.maxDepth4Blas; d->maxDepth4Tlas = b.maxDepth4Tlas; d->maxDepth4Blas = b.maxDepth4Blas; d->sahCost = 0.0f;
    put(d->nodes4, b.nodes4.data(), b.nodes4.size() * sizeof(HostNode4));
    put(d->triangles, b.tris.data(), b.tris.size() * sizeof(HostTri)); put(d->attributes, b.attrs.data(), b.attrs.size() * sizeof(HostTriAttr));
    put(d->tangents, b.tangents.data(), b.tangents.size() * sizeof(HostTriTangent)); put(d->instances, b.instances.data(), b.instances.size() * sizeof(HostInstance));
    return HRPT_OK;
} catch (...) { return caught(nullptr, "hrpt_selftest_host_build"); }

int hrpt_selftest_unorm8(HrptContext* c, float* out512)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!out512) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_unorm8: null out");
    HIP_TRY(c, hipSetDevice(c->device));
    DeviceBuffer<float> d;
    HIP_TRY(c, d.alloc(512 * sizeof(float)));
    hipError_t e = launch_unorm8_table(d, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out512, d, 512 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, HRPT_ERR_HIP, std::string("hrpt_selftest_unorm8: ") + hipGetErrorString(e));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_selftest_unorm8"); }

int hrpt_selftest_sample_textures(HrptContext* c, const HrptTextureProbe* probes, HrptTextureProbeResult* results, uint64_t count)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, "hrpt_selftest_sample_textures: no scene uploaded");
    if (count == 0) return HRPT_OK;
    if (!probes || !results) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_sample_textures: null array");
    if (count > (1ull << 24)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_sample_textures: too many probes in one call");
    const uint32_t materialCount = (uint32_t)c->keptMaterials.size();
    for (uint64_t i = 0; i < count; ++i)
        if (probes[i].material >= materialCount) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_sample_textures: material index out of range");
    HIP_TRY(c, hipSetDevice(c->device));
    DeviceBuffer<HrptTextureProbe> dProbes; DeviceBuffer<HrptTextureProbeResult> dResults;
    hipError_t e = dProbes.alloc(count * sizeof(HrptTextureProbe));
    if (e == hipSuccess) e = dResults.alloc(count * sizeof(HrptTextureProbeResult));
    if (e == hipSuccess) e = hipMemcpyAsync(dProbes, probes, count * sizeof(HrptTextureProbe), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_sample_textures(c->view, materialCount, dProbes, dResults, (uint32_t)count, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(results, dResults, count * sizeof(HrptTextureProbeResult), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, hip_status(e), std::string("hrpt_selftest_sample_textures: ") + hipGetErrorString(e));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_selftest_sample_textures"); }

int hrpt_selftest_atmosphere(HrptContext* c, const HrptAtmosphereProbe* probes, HrptAtmosphereProbeResult* results, uint64_t count)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, "hrpt_selftest_atmosphere: no scene uploaded");
    if (count == 0) return HRPT_OK;
    if (!probes || !results) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_atmosphere: null array");
    if (count > (1ull << 24)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_atmosphere: too many probes in one call");
    HIP_TRY(c, hipSetDevice(c->device));
    DeviceBuffer<HrptAtmosphereProbe> dProbes; DeviceBuffer<HrptAtmosphereProbeResult> dResults;
    hipError_t e = dProbes.alloc(count * sizeof(HrptAtmosphereProbe));
    if (e == hipSuccess) e = dResults.alloc(count * sizeof(HrptAtmosphereProbeResult));
    if (e == hipSuccess) e = hipMemcpyAsync(dProbes, probes, count * sizeof(HrptAtmosphereProbe), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_atmosphere_probes(c->view, dProbes, dResults, (uint32_t)count, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(results, dResults, count * sizeof(HrptAtmosphereProbeResult), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, hip_status(e), std::string("hrpt_selftest_atmosphere: ") + hipGetErrorString(e));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_selftest_atmosphere"); }
