// pt_capi_scene.cpp -- the scene of a context: upload (copies), the acceleration structure (flat or two-level, host or GPU builders) and the
// updates of lights, materials and instances. Per-dispatch constants are filled exactly as PathTracerRenderer::Render fills them (the
// reference's src/PathTracerRenderer.cpp:58-75).
#include <chrono>

#include "pt_capi_internal.h"
#include "pt_record_layout.h"

using namespace hrt;
using namespace hrt::capi;

// The one place a Host* array becomes the Gpu* array the kernels read (pt_record_layout.h holds the layout contract): a device copy of
// `host` owned by `owner`. G is const GpuX for a table the device only reads; a caller that asks for a writable GpuX* fills the first `skip`
// records, which are not copied, on the device itself.
template <class H, class G>
static int upload_records(HrptContext* c, const std::vector<H>& host, G** dev, DeviceAllocations* owner, size_t skip = 0)
{
    static_assert(std::is_same<typename std::remove_const<G>::type, typename GpuRecordOf<H>::type>::value, "pt_record_layout.h GpuRecordOf");
    H* d = nullptr;
    const int r = upload_writable(c, host.data(), host.size(), &d, owner, skip);
    *dev = reinterpret_cast<G*>(d);
    return r;
}

// DirectX::PackedVector::XMConvertFloatToHalf (round to nearest even), src/CommonResources.cpp:553
static uint16_t float_to_half(float f)
{
    uint32_t x; memcpy(&x, &f, 4);
    uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x47800000u) return (uint16_t)(sign | 0x7c00u | ((x > 0x7f800000u) ? (0x200u | ((x >> 13) & 0x3ffu)) : 0u));
    if (x < 0x38800000u) {
        if (x < 0x33000000u) return (uint16_t)sign;
        uint32_t shift = 126u - (x >> 23);
        uint32_t m = (x & 0x7fffffu) | 0x800000u;
        uint32_t h = m >> shift, rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1u);
        if (rem > halfway || (rem == halfway && (h & 1u))) ++h;
        return (uint16_t)(sign | h);
    }
    uint32_t r = x + 0xfffu + ((x >> 13) & 1u);
    return (uint16_t)(sign | ((r - 0x38000000u) >> 13));
}

static void free_acceleration(HrptContext* c, bool keepGpuBuilder)
{
    c->bvhAllocations.clear();
    if (!keepGpuBuilder) {
        c->gpuBuilder.reset();
        c->tlasBuilder.reset(); c->tlasBuilderInstances = 0;
        c->meshAllocations.clear();
        delete c->twoLevel; c->twoLevel = nullptr;
    }
}

void capi::free_scene(HrptContext* c)
{
    free_acceleration(c, false);
    c->perScene = PerSceneBuffers{};        // motion tables, deform staging, skin floats, previous positions; the stale flags are set again
    c->allocations.clear();
    c->nodesQ.reset();
    c->keptVertices.clear(); c->keptIndices.clear(); c->keptMeshData.clear(); c->keptInstances.clear(); c->keptMaterials.clear(); c->keptLights.clear(); c->lightCapacity = 0;
    c->haveScene = false;
    ++c->instanceEpoch;
    memset(&c->view, 0, sizeof c->view);
}

// Two-level structure: asked for, or (AUTO) large and heavily instanced
static bool two_level_wanted(const HrptContext* c, const HrptSceneDesc& s, uint64_t sceneTris)
{
    int want = c->accelStructure;
    if (const char* e = getenv("HRPT_ACCEL_STRUCTURE")) { const int v = atoi(e); if (v >= HRPT_ACCEL_AUTO && v <= HRPT_ACCEL_TWO_LEVEL) want = v; }
    if (want == HRPT_ACCEL_FLAT || s.instanceCount == 0) return false;
    if (want == HRPT_ACCEL_TWO_LEVEL) return true;
    std::vector<uint8_t> used(s.meshDataCount, 0); uint32_t distinct = 0;
    for (uint32_t i = 0; i < s.instanceCount; ++i) if (!used[s.instances[i].m_MeshDataIndex]) { used[s.instances[i].m_MeshDataIndex] = 1; ++distinct; }
    // scenes with non-opaque instances: measured cross-over against the flat structure at ~16 M world triangles (instanced alpha-tested + glass
    // meshes: 7.6 M triangles 35.5 vs 32.3 ms, 30 M 38 vs 46 ms; the two-level candidate buffer holds 4 entries with the instance next to the triangle)
    bool nonOpaque = false;
    for (uint32_t i = 0; i < s.instanceCount && !nonOpaque; ++i) nonOpaque = s.materials[s.instances[i].m_MaterialIndex].m_AlphaMode != HRPT_ALPHA_MODE_OPAQUE;
    return sceneTris >= (nonOpaque ? (16ull << 20) : (2ull << 20)) && (uint64_t)s.instanceCount >= 8ull * distinct;
}

// instancesOnly: the mesh trees of c->twoLevel are kept (hrpt_update_instances)
// kTwoLevelDoesNotFit: the scene cannot be held in this form (an instance with a singular world matrix -- a mesh flattened to a plane --, trees
// too deep): the caller builds the flat structure instead, which has no such limits
constexpr int kTwoLevelDoesNotFit = 1;
// The tree over the instances on the GPU (the reference rebuilds its TLAS on the GPU every frame, src/CommonRenderers.cpp:234-246): the
// builder's box mode over the instances' padded world boxes, then launch_tlas_fixup writes the nodes, leaves turned into instance references,
// to the front of the scene's node array. The builder and its buffers stay on the device: a rebuild (hrpt_update_instances) uploads 24 bytes
// per instance and runs the kernels. false: not built (a device error, a tree too deep): the caller builds the tree on the host instead.
static bool build_instance_tree_on_gpu(HrptContext* c, uint32_t instanceCount, const std::vector<float>& boxes, bool rebuild, bool refit, GpuNode4* dstNodes, uint32_t& depth4Levels)
{
    GpuBuildError gerr;
    if (!c->tlasBuilder || c->tlasBuilderInstances != instanceCount) {
        c->tlasBuilder = std::make_unique<GpuBvhBuilder>(); c->tlasBuilderInstances = 0;
        if (c->tlasBuilder->prepare_boxes(instanceCount, c->stream, gerr) != hipSuccess) { c->tlasBuilder.reset(); return false; }
        c->tlasBuilderInstances = instanceCount;
    }
    GpuBuiltBvh g;
    // Hierarchy: PLOC at upload, the Morton radix tree for rebuilds (hrpt_update_instances) unless a GPU builder was asked for by name. Measured on
    // 16 384 / 65 536 instances: the radix tree is built in 0.45 ms of device time against 1.9 / 2.1 ms and traverses 0 / 2 % slower, so a host that
    // moves instances every frame comes out ahead with it (update 1.8 / 4.0 ms against 3.0 / 5.5 ms), a static scene with PLOC.
    bool ploc = c->bvhBuilder == HRPT_BVH_BUILDER_GPU_PLOC || (c->bvhBuilder != HRPT_BVH_BUILDER_GPU_LBVH && !rebuild);
    if (const char* e = getenv("HRPT_TLAS_LBVH")) ploc = atoi(e) == 0;
    const hipError_t ge = (rebuild && refit && c->tlasBuilder->can_refit()) ? c->tlasBuilder->refit_boxes(boxes.data(), c->stream, g, gerr)      // hrpt_refit_instances
                                                                              : c->tlasBuilder->build_boxes(boxes.data(), ploc, kTraversalStackDepth, c->stream, g, gerr);
    if (ge != hipSuccess || g.maxDepth + 2 > kTraversalStackDepth || g.node4Count == 0 || g.node4Count > instanceCount) return false;
    if (launch_tlas_fixup(g.nodes4, g.node4Count, g.leafOrder, dstNodes, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return false;
    depth4Levels = g.maxDepth4 + 1;
    c->buildInfo.deviceBuildMs = g.deviceMs; c->buildInfo.usedBuilder = (g.ploc ? HRPT_BVH_BUILDER_GPU_PLOC : HRPT_BVH_BUILDER_GPU_LBVH) | (g.refitted ? HRPT_BVH_BUILDER_REFITTED : 0u);
    return true;
}

// The per-mesh arrays of the two-level structure into `v`: triangles, their attribute records and, where a material samples a normal map, tangents.
static int upload_triangles(HrptContext* c, const BuiltTwoLevel& b, SceneView& v, DeviceAllocations* owner)
{
    HRPT_TRY(upload_records(c, b.tris, &v.tris, owner));
    HRPT_TRY(upload_records(c, b.attrs, &v.attrs, owner));
    v.triCount = (uint32_t)b.tris.size();
    v.tangents = nullptr;
    if (!b.tangents.empty()) HRPT_TRY(upload_records(c, b.tangents, &v.tangents, owner));
    return HRPT_OK;
}

// What an instance update replaces, into `v`: the node array (the tree over the instances in front of the mesh trees), the instance records and
// their adjugate rows. The first `reservedNodes` nodes are not copied: the caller writes them on the device, through `nodes4`.
static int upload_instance_level(HrptContext* c, const BuiltTwoLevel& b, SceneView& v, uint32_t reservedNodes, GpuNode4*& nodes4)
{
    HRPT_TRY(upload_records(c, b.nodes4, &nodes4, &c->bvhAllocations, reservedNodes));
    HRPT_TRY(upload_records(c, b.instances, &v.instances, &c->bvhAllocations));
    HRPT_TRY(upload_records(c, b.instShade, &v.instShade, &c->bvhAllocations));
    v.nodes4 = nodes4; v.node4Count = (uint32_t)b.nodes4.size(); v.nodesQ = nullptr;
    v.instanceCount = (uint32_t)b.instances.size();
    return HRPT_OK;
}

static int build_two_level(HrptContext* c, const HrptSceneDesc& s, SceneView& v, bool instancesOnly, bool refit)
{
    std::string berr;
    const bool timing = getenv("HRPT_BUILD_TIMING") != nullptr; auto tp = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (!timing) return; (void)hipStreamSynchronize(c->stream); auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[two-level] %-22s %7.3f ms\n", what, std::chrono::duration<float, std::milli>(t - tp).count()); tp = t; };
    // who builds the tree over the instances: the GPU from 1024 instances on (host SAH: 2 / 6 / 16 ms for 4 096 / 16 384 / 65 536 instances, the GPU
    // ~1 ms), unless the host builder was asked for (hrpt_set_bvh_builder) or HRPT_TLAS_BUILDER says otherwise
    bool gpuTree = s.instanceCount >= 1024 && c->bvhBuilder != HRPT_BVH_BUILDER_HOST_SAH;
    if (const char* e = getenv("HRPT_TLAS_BUILDER")) gpuTree = s.instanceCount >= 8 && (strcmp(e, "gpu") == 0 || strcmp(e, "1") == 0);
    lap("(entry)");
    std::vector<float> boxes;
    std::vector<float>* wantBoxes = gpuTree ? &boxes : nullptr;      // set: the node range of the instance tree is reserved and left empty
    if (!instancesOnly) { delete c->twoLevel; c->twoLevel = new BuiltTwoLevel(); }
    if (!(instancesOnly ? rebuild_two_level_instances(s, *c->twoLevel, berr, wantBoxes) : build_scene_two_level(s, *c->twoLevel, berr, wantBoxes))) {
        if (berr.find("singular") != std::string::npos) return kTwoLevelDoesNotFit;
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: " + berr);
    }
    lap("host records");
    BuiltTwoLevel& b = *c->twoLevel;
    if (two_level_stack_need(b) > 128u) return kTwoLevelDoesNotFit;
    if (!instancesOnly) HRPT_TRY(upload_triangles(c, b, v, &c->meshAllocations));
    if (b.nodes4.size() >= kMaxStructureNodes) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: more than 2^25 nodes (32-bit node offsets in the traversal kernels)");
    // gpuTree: the reserved range at the front is written on the device (launch_tlas_fixup): only the mesh trees behind it cross PCIe
    GpuNode4* nodes4 = nullptr;
    HRPT_TRY(upload_instance_level(c, b, v, gpuTree ? b.tlasNodeCount : 0, nodes4));
    lap("uploads");
    if (gpuTree) {
        uint32_t levels = 0;
        if (build_instance_tree_on_gpu(c, s.instanceCount, boxes, instancesOnly, refit, nodes4, levels)) {
            b.maxDepth4Tlas = levels;
        } else {
            // the host builds it after all: same layout rules as ever (the reserved node range shrinks to the tree's size)
            c->bvhAllocations.clear();
            if (!rebuild_two_level_instances(s, b, berr)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: " + berr);
            HRPT_TRY(upload_instance_level(c, b, v, 0, nodes4));
            gpuTree = false;
        }
    }
    lap("instance tree (GPU)");
    if (two_level_stack_need(b) > 128u) return kTwoLevelDoesNotFit;
    v.nodes = nullptr; v.nodeCount = b.tlasNodeCount; v.rootLeaf = b.tlasRootLeaf;      // nodeCount != 0: the walk starts at node4 0 (the instance tree)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!gpuTree) c->buildInfo.usedBuilder = HRPT_BVH_BUILDER_HOST_SAH;      // (the mesh trees are the host's either way; usedBuilder names who built the tree over the instances)
    c->buildInfo.structure = HRPT_ACCEL_TWO_LEVEL;
    c->buildInfo.instanceNodeCount = b.tlasNodeCount; c->buildInfo.distinctMeshes = b.distinctMeshes;
    c->buildInfo.triangleCount = v.triCount; c->buildInfo.nodeCount = 0; c->buildInfo.node4Count = v.node4Count;
    c->buildInfo.maxDepth = 0; c->buildInfo.maxDepth4 = b.maxDepth4Tlas + b.maxDepth4Blas;
    c->bvhNodes = v.node4Count; c->bvhTris = v.triCount;
    c->traits.bvhMaxDepth = 0; c->traits.bvh4MaxDepth = b.maxDepth4Tlas + b.maxDepth4Blas; c->traits.twoLevelStackNeed = two_level_stack_need(b); c->traits.quantisedNodes = false;
    return HRPT_OK;
}

// ---- the flat structure: one route per builder, each says whether it built (a status other than HRPT_OK ends the build), then the quantised nodes ----
struct TreeDepths { uint32_t maxDepth = 0, maxDepth4 = 0; };

// experiment (HRPT_GPU_BVH_HOST_COLLAPSE): the GPU-built 2-wide tree with the host's area-greedy, depth-first 4-wide collapse
static int collapse_gpu_tree_on_host(HrptContext* c, const GpuBuiltBvh& g, SceneView& v, TreeDepths& depths)
{
    std::vector<HostNode> n2(g.nodeCount); std::vector<HostNode4> n4; uint32_t d4 = 0;
    HIP_TRY(c, hipMemcpy(n2.data(), g.nodes, n2.size() * sizeof(HostNode), hipMemcpyDeviceToHost));
    collapse_bvh2_on_host(n2, n4, d4);
    HRPT_TRY(upload_records(c, n4, &v.nodes4, &c->bvhAllocations));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    v.node4Count = (uint32_t)n4.size(); depths.maxDepth4 = d4; c->nodes4Capacity = 0;
    return HRPT_OK;
}

// The GPU builders: the whole build runs on the device; only the per-instance adjugate rows (O(instances)) are prepared on the host.
// Not built and HRPT_OK: too deep for the traversal stacks, or a device error -- the host builder takes over.
static int build_flat_on_gpu(HrptContext* c, const HrptSceneDesc& s, bool usePloc, bool refit, SceneView& v, TreeDepths& depths, bool& built)
{
    GpuBuiltBvh g; GpuBuildError gerr;
    hipError_t ge = hipSuccess;
    if (!c->gpuBuilder) {
        c->gpuBuilder = std::make_unique<GpuBvhBuilder>();
        ge = c->gpuBuilder->prepare(s, scene_needs_tangents(s), c->stream, gerr);
    }
    if (ge == hipSuccess) ge = (refit && c->gpuBuilder->can_refit()) ? c->gpuBuilder->refit(s.instances, c->stream, g, gerr)
                                                                     : c->gpuBuilder->build(s.instances, usePloc, kTraversalStackDepth, c->stream, g, gerr);
    if (ge != hipSuccess || g.maxDepth + 2 > kTraversalStackDepth) {
        c->gpuBuilder.reset();      // drop the device-side builder
        switch (gerr.reason) {
        case GpuBuildFailure::NonFinitePosition: return fail(c, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: " + gerr.message);
        case GpuBuildFailure::OutOfMemory: return fail(c, HRPT_ERR_OUT_OF_MEMORY, "acceleration structure: " + gerr.message);
        case GpuBuildFailure::DoesNotFit: case GpuBuildFailure::DeviceError: case GpuBuildFailure::None: break;      // the host builder takes over
        }
        return HRPT_OK;
    }
    v.nodes = g.nodes; v.nodeCount = g.nodeCount; v.nodes4 = g.nodes4; v.node4Count = g.node4Count; v.tris = g.tris; v.triCount = g.triCount;
    v.rootLeaf = 0; v.attrs = g.attrs; v.tangents = g.tangents;
    depths.maxDepth = g.maxDepth; depths.maxDepth4 = g.maxDepth4; built = true; c->nodes4Capacity = g.nodes4Capacity;
    if (getenv("HRPT_GPU_BVH_HOST_COLLAPSE")) HRPT_TRY(collapse_gpu_tree_on_host(c, g, v, depths));
    c->buildInfo.usedBuilder = g.ploc ? HRPT_BVH_BUILDER_GPU_PLOC : HRPT_BVH_BUILDER_GPU_LBVH; c->buildInfo.deviceBuildMs = g.deviceMs; c->buildInfo.mortonBits = g.mortonBits; c->buildInfo.sahCost = g.sahCost;
    if (g.refitted) c->buildInfo.usedBuilder |= HRPT_BVH_BUILDER_REFITTED;
    std::vector<HostInstShade> shade; build_instance_shade(s, shade);
    HRPT_TRY(upload_records(c, shade, &v.instShade, &c->bvhAllocations));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HRPT_OK;
}

// The host builder (binned SAH): always builds, or refuses the scene.
static int build_flat_on_host(HrptContext* c, const HrptSceneDesc& s, SceneView& v, TreeDepths& depths)
{
    BuiltBvh bvh; std::string berr;
    if (!build_scene_bvh(s, bvh, berr)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: " + berr);
    DeviceAllocations* own = &c->bvhAllocations;
    HRPT_TRY(upload_records(c, bvh.nodes, &v.nodes, own));
    HRPT_TRY(upload_records(c, bvh.tris, &v.tris, own));
    v.nodeCount = (uint32_t)bvh.nodes.size(); v.triCount = (uint32_t)bvh.tris.size();
    v.rootLeaf = bvh.rootLeaf;
    HRPT_TRY(upload_records(c, bvh.nodes4, &v.nodes4, own));
    v.node4Count = (uint32_t)bvh.nodes4.size();
    // The quantised vertex / index / mesh / instance buffers are consumed here: per-triangle attribute records and
    // per-instance adjugate rows replace the per-hit GetTriangleVertices + UnpackVertex + MakeAdjugateMatrix work.
    HRPT_TRY(upload_records(c, bvh.attrs, &v.attrs, own));
    HRPT_TRY(upload_records(c, bvh.instShade, &v.instShade, own));
    v.tangents = nullptr;
    if (!bvh.tangents.empty()) HRPT_TRY(upload_records(c, bvh.tangents, &v.tangents, own));
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // the BuiltBvh staging vectors die at scope exit
    depths.maxDepth = bvh.maxDepth; depths.maxDepth4 = bvh.maxDepth4;
    c->buildInfo.usedBuilder = HRPT_BVH_BUILDER_HOST_SAH; c->buildInfo.sahCost = bvh.sahCost;
    return HRPT_OK;
}

// The 64-byte quantised form of the 4-wide tree, whichever builder made it (what the wavefront kernels may read when the tree is not in LDS),
// and the choice of the form the kernels walk. quantised = false with HRPT_OK: there are no nodes (the scene fits one leaf), or the fp32 nodes are walked.
static int quantise_nodes(HrptContext* c, const HrptSceneDesc& s, SceneView& v, bool& quantised)
{
    v.nodesQ = nullptr; quantised = false;
    if (!v.node4Count) return HRPT_OK;
    size_t cap = c->nodesQ.bytes() / sizeof(GpuNodeQ);         // records the buffer holds
    if (cap <= v.node4Count) {                                  // (<=: record cap - 1 is the accumulator below, never a node)
        cap = (size_t)v.node4Count + v.node4Count / 8 + 64;
        if (c->nodesQ.alloc(cap * sizeof(GpuNodeQ)) != hipSuccess) return fail(c, HRPT_ERR_OUT_OF_MEMORY, "acceleration structure: quantised nodes");
    }
    double* dArea = reinterpret_cast<double*>(c->nodesQ + (cap - 1));       // the last (spare) record of the buffer: two doubles
    HIP_TRY(c, hipMemsetAsync(dArea, 0, 4 * sizeof(double), c->stream));
    HIP_TRY(c, launch_quantise_nodes(v.nodes4, v.node4Count, c->nodesQ, dArea, c->stream));
    double area[4] = { 0.0, 0.0, 0.0, 0.0 };
    HIP_TRY(c, hipMemcpyAsync(area, dArea, sizeof area, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    v.nodesQ = c->nodesQ;
    // Which nodes the kernels walk when the tree is in global memory. The quantised form saves three of seven 16-byte requests per lane and
    // step and pays in decode arithmetic and in looser boxes; what the looser LEAF boxes cost is triangle tests (three requests + a
    // watertight test each). Measured (MI355X, 1080p): Sponza-class scene: wf_extend 6.66 -> 6.18 ms, frame 13.8 -> 13.3 ms; glass scene
    // (18 k triangles of tessellated glass bodies): shadow-ray triangle tests x 2.4, closest-hit leaf visits + 43 %, frame +2 %.
    const float inflation = area[0] > 0.0 ? (float)(area[1] / area[0]) : 1.0f;
    if (getenv("HRPT_BVH_NODE_FORMAT_DEBUG")) fprintf(stderr, "quantised nodes: leaf area ratio %.4f (area-weighted), %.4f (mean over %.0f leaves)\n", inflation, area[3] > 0 ? area[2] / area[3] : 1.0, area[3]);
    int format = 0;
    if (const char* e = getenv("HRPT_BVH_NODE_FORMAT")) format = atoi(e);          // 1: fp32 nodes, 2: quantised nodes, else by the leaf-area ratio
    // (the leaf-area ratio is ~1.01 on BOTH scenes, so it does not tell them apart: on the glass scene it is the paths that bounce inside and between
    // the finely tessellated glass bodies that visit 40 % more leaves through the rounded boxes. Until that is understood the rule is empirical:
    // quantised nodes unless some instance is transmissive or BLEND.)
    bool glassy = false;
    for (uint32_t i = 0; i < s.instanceCount && !glassy; ++i) {
        const HrptMaterialConstants& m = s.materials[s.instances[i].m_MaterialIndex];
        glassy = m.m_TransmissionFactor > 0.0f || m.m_AlphaMode == HRPT_ALPHA_MODE_BLEND;
    }
    quantised = format == 2 || (format != 1 && inflation <= 1.10f && !glassy);
    c->buildInfo.leafAreaPermille = (uint32_t)(inflation * 1000.0f + 0.5f); c->buildInfo.nodeFormat = quantised ? 2u : 1u;
    return HRPT_OK;
}

// The acceleration structure + the records derived from instance transforms (Scene::BuildAccelerationStructures, src/Scene.cpp:67-214),
// written into `v`. First build of a scene or a rebuild after hrpt_update_instances (the GPU builder then keeps its device-resident
// geometry and buffers).
// refit (hrpt_refit_instances): where a GPU builder holds the hierarchy of the previous build, its boxes are recomputed instead of the tree rebuilt
int capi::build_acceleration(HrptContext* c, const HrptSceneDesc& s, uint64_t sceneTris, SceneView& v, bool firstBuild, bool refit)
{
    const auto t0 = std::chrono::steady_clock::now();
    c->buildInfo = HrptBuildInfo{};
    c->buildInfo.requestedBuilder = (uint32_t)c->bvhBuilder;
    c->buildInfo.structure = HRPT_ACCEL_FLAT; c->nodes4Capacity = 0;
    const bool keepMeshTrees = !firstBuild && c->twoLevel != nullptr;       // hrpt_update_instances on a two-level scene
    free_acceleration(c, !firstBuild);
    if (keepMeshTrees || (firstBuild && two_level_wanted(c, s, sceneTris))) {
        const int r = build_two_level(c, s, v, keepMeshTrees, refit);
        if (r != kTwoLevelDoesNotFit) {
            c->buildInfo.buildMs = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
            return r;
        }
        // flat after all: drop everything of the two-level form (a moved instance may have become singular: hrpt_update_instances ends up here too)
        free_acceleration(c, false);
        c->buildInfo.structure = HRPT_ACCEL_FLAT;
        firstBuild = true;
    }
    v.instances = nullptr; v.instanceCount = 0; c->traits.twoLevelStackNeed = 0;
    if (sceneTris >= kMaxStructureTriangles) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: too many triangles for the flat structure (2^32 / 48 = 89 M world-space triangles; instanced scenes can use HRPT_ACCEL_TWO_LEVEL)");
    TreeDepths depths;
    bool built = false;
    const int builder = c->bvhBuilder == HRPT_BVH_BUILDER_AUTO ? (sceneTris >= 65536 ? HRPT_BVH_BUILDER_GPU_PLOC : HRPT_BVH_BUILDER_HOST_SAH) : c->bvhBuilder;
    const bool gpuBuilder = builder == HRPT_BVH_BUILDER_GPU_LBVH || builder == HRPT_BVH_BUILDER_GPU_PLOC;
    if (!gpuBuilder) c->gpuBuilder.reset();
    if (gpuBuilder && sceneTris >= 8) HRPT_TRY(build_flat_on_gpu(c, s, builder == HRPT_BVH_BUILDER_GPU_PLOC, refit && !firstBuild, v, depths, built));
    if (!built) HRPT_TRY(build_flat_on_host(c, s, v, depths));
    if (v.node4Count >= kMaxStructureNodes) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: more than 2^25 nodes (32-bit node offsets in the traversal kernels)");
    bool quantisedNodes = false;
    HRPT_TRY(quantise_nodes(c, s, v, quantisedNodes));
    c->buildInfo.buildMs = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->buildInfo.triangleCount = v.triCount; c->buildInfo.nodeCount = v.nodeCount; c->buildInfo.node4Count = v.node4Count;
    c->buildInfo.maxDepth = depths.maxDepth; c->buildInfo.maxDepth4 = depths.maxDepth4;
    c->bvhNodes = v.nodeCount; c->bvhTris = v.triCount;
    c->traits.bvhMaxDepth = depths.maxDepth; c->traits.bvh4MaxDepth = depths.maxDepth4; c->traits.quantisedNodes = quantisedNodes;
    return HRPT_OK;
}

// What the kernels specialise on (SceneTraits), from the library's copy of instances / materials / lights; the tree depths are kept.
void capi::refresh_traits(HrptContext* c)
{
    SceneTraits t; t.bvhMaxDepth = c->traits.bvhMaxDepth; t.bvh4MaxDepth = c->traits.bvh4MaxDepth; t.twoLevelStackNeed = c->traits.twoLevelStackNeed; t.quantisedNodes = c->traits.quantisedNodes;
    for (const HrptPerInstanceData& in : c->keptInstances) {
        const HrptMaterialConstants& m = c->keptMaterials[in.m_MaterialIndex];
        // the transmission branch (PathTracer.hlsl:149-255) is entered for transmissive AND for BLEND materials (effective transmission
        // 1 - alpha), and a thick one switches the path's medium state there: that state then has to travel with the path
        if ((m.m_TransmissionFactor > 0.0f || m.m_AlphaMode == HRPT_ALPHA_MODE_BLEND) && m.m_IsThinSurface == 0) t.hasMedium = true;
        if (m.m_AlphaMode == HRPT_ALPHA_MODE_BLEND && !(m.m_TransmissionFactor > 0.0f)) t.hasStochasticAlpha = true;
        if (m.m_TextureFlags != 0) t.hasTextures = true;
        if (m.m_AlphaMode != HRPT_ALPHA_MODE_OPAQUE) t.hasNonOpaque = true;
        if (m.m_TransmissionFactor > 0.0f || m.m_AlphaMode == HRPT_ALPHA_MODE_BLEND) t.hasTransmissiveOrBlend = true;
    }
    for (const HrptGPULight& l : c->keptLights) if (l.m_Type != HRPT_LIGHT_DIRECTIONAL) t.directionalLightsOnly = false;
    c->traits = t;
}

// The descriptor table of the scene's textures: every texture's texels go to the device (the scene's allocation list), `table` is left to the caller.
static int upload_texels(HrptContext* c, const HrptSceneDesc& s, std::vector<GpuTexture>& table)
{
    int r;
    for (uint32_t i = 0; i < s.textureCount; ++i) {
        const HrptTextureDesc& td = s.textures[i];
        GpuTexture& g = table[i];
        memset(&g, 0, sizeof g);
        g.w = td.width; g.h = td.height; g.format = td.format; g.mipCount = td.mipCount ? td.mipCount : 1u;
        if (!td.texels) continue;
        if (td.width == 0 || td.height == 0) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: zero-sized texture");
        if (td.format > HRPT_TEXTURE_FORMAT_RGBA32_FLOAT) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: unknown texture format");
        if (g.mipCount > HRPT_TEXTURE_MAX_MIPS) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: more than HRPT_TEXTURE_MAX_MIPS mip levels");
        uint64_t texels = 0;
        for (uint32_t l = 0; l < g.mipCount; ++l) {
            if (l > 0 && (td.width >> l) == 0 && (td.height >> l) == 0) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: more mip levels than the texture size allows");
            g.mipOffset[l] = (uint32_t)texels;
            texels += (uint64_t)((td.width >> l) ? (td.width >> l) : 1u) * ((td.height >> l) ? (td.height >> l) : 1u);
        }
        if (texels > 0xFFFFFFFFull) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: texture too large");
        const size_t bpt = td.format <= HRPT_TEXTURE_FORMAT_RGBA8_SRGB ? 4 : (td.format == HRPT_TEXTURE_FORMAT_RGBA16_FLOAT ? 8 : 16);
        const uint8_t* d;
        if ((r = upload(c, static_cast<const uint8_t*>(td.texels), (size_t)texels * bpt, &d)) != HRPT_OK) return r;
        g.texels = d;
    }
    return HRPT_OK;
}

// Bruneton LUTs: float32 file layout -> RGBA16F (src/CommonResources.cpp:534-558)
static void convert_atmosphere_tables(const HrptSceneDesc& s, std::vector<uint16_t>& hT, std::vector<uint16_t>& hS)
{
    const size_t nT = hT.size(), nS = hS.size();
    for (size_t i = 0; i < nT; ++i) hT[i] = float_to_half(s.brunetonTransmittance[i]);
    {   // 4 M conversions: 9 ms of every upload on one thread
        const float* src = s.brunetonScattering; uint16_t* dst = hS.data();
        const unsigned threads = std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
        const size_t chunk = (nS + threads - 1) / threads;
        auto part = [src, dst, nS, chunk](size_t t) { for (size_t i = t * chunk, e = std::min(nS, i + chunk); i < e; ++i) dst[i] = float_to_half(src[i]); };
        std::vector<std::thread> pool;
        size_t started = 1;
        try { for (; started < threads; ++started) pool.emplace_back(part, started); } catch (const std::system_error&) {}
        part(0);
        for (std::thread& th : pool) th.join();
        for (size_t t = started; t < threads; ++t) part(t);       // (threads that could not be started)
    }
}

int hrpt_upload_scene(HrptContext* c, const HrptSceneDesc* s)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!s) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: null scene");
    if (!s->brunetonTransmittance || !s->brunetonScattering) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: Bruneton LUTs missing");
    if (s->textureCount && !s->textures) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: null texture table");
    HIP_TRY(c, hipSetDevice(c->device));
    std::string berr;
    uint64_t sceneTris = 0;
    if (!validate_scene(*s, sceneTris, berr, false)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: " + berr);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_scene(c);
    c->traits = SceneTraits();
    SceneView v{};
    int r;
    const bool timing = getenv("HRPT_BUILD_TIMING") != nullptr; auto tp = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (!timing) return; (void)hipStreamSynchronize(c->stream); auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[upload]    %-22s %7.3f ms\n", what, std::chrono::duration<float, std::milli>(t - tp).count()); tp = t; };
    if ((r = build_acceleration(c, *s, sceneTris, v, true)) != HRPT_OK) return r;
    lap("acceleration structure");
    if ((r = upload(c, s->materials, s->materialCount, &v.materials)) != HRPT_OK) return r;
    if ((r = upload(c, s->lights, s->lightCount, &v.lights)) != HRPT_OK) return r;
    v.lightCount = s->lightCount; c->lightCapacity = s->lightCount;
    std::vector<GpuTexture> table(s->textureCount);
    if ((r = upload_texels(c, *s, table)) != HRPT_OK) return r;
    if ((r = upload(c, table.data(), table.size(), &v.textures)) != HRPT_OK) return r;
    v.textureCount = s->textureCount;
    lap("materials, textures");

    const size_t nT = 256u * 64u * 4u, nS = 256u * 128u * 32u * 4u;
    std::vector<uint16_t> hT(nT), hS(nS);
    convert_atmosphere_tables(*s, hT, hS);
    if ((r = upload(c, hT.data(), nT, &v.lutTransmittance)) != HRPT_OK) return r;
    if ((r = upload(c, hS.data(), nS, &v.lutScattering)) != HRPT_OK) return r;
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // host staging vectors die at scope exit
    lap("atmosphere tables");

    c->view = v; c->haveScene = true;
    c->keptVertices.assign(s->vertices, s->vertices + s->vertexCount); c->keptIndices.assign(s->indices, s->indices + s->indexCount);
    c->keptMeshData.assign(s->meshData, s->meshData + s->meshDataCount); c->keptInstances.assign(s->instances, s->instances + s->instanceCount);
    c->keptMaterials.assign(s->materials, s->materials + s->materialCount);
    c->keptLights.assign(s->lights, s->lights + s->lightCount);
    refresh_traits(c);
    lap("kept copies, traits");
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_upload_scene"); }

// The scene description the rebuild paths hand to the builders, over the library's copies.
HrptSceneDesc capi::kept_scene_desc(HrptContext* c)
{
    HrptSceneDesc s{};
    s.vertices = c->keptVertices.data(); s.vertexCount = (uint32_t)c->keptVertices.size();
    s.indices = c->keptIndices.data(); s.indexCount = (uint32_t)c->keptIndices.size();
    s.meshData = c->keptMeshData.data(); s.meshDataCount = (uint32_t)c->keptMeshData.size();
    s.instances = c->keptInstances.data(); s.instanceCount = (uint32_t)c->keptInstances.size();
    s.materials = c->keptMaterials.data(); s.materialCount = (uint32_t)c->keptMaterials.size();
    static const HrptGPULight noLight{};                 // lights play no part in the build; validate_scene only wants the array to exist
    s.lights = &noLight; s.lightCount = 1;
    return s;
}
uint64_t capi::kept_triangle_count(const HrptContext* c)
{
    uint64_t n = 0;
    for (const HrptPerInstanceData& in : c->keptInstances) n += c->keptMeshData[in.m_MeshDataIndex].m_IndexCounts[0] / 3;
    return n;
}

int hrpt_update_lights(HrptContext* c, const HrptGPULight* lights, uint32_t count)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->haveScene) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_lights: no scene uploaded");
    if (!lights || count == 0) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_lights: a scene needs at least one light (the reference guarantees a directional light, src/Scene.cpp:635-666)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // frames in flight still read the old buffer
    if (count > c->lightCapacity) {
        const HrptGPULight* d; int r;
        if ((r = upload(c, lights, count, &d)) != HRPT_OK) return r;      // the old, smaller buffer stays in the scene's allocation list
        c->view.lights = d; c->lightCapacity = count;
    } else {
        HIP_TRY(c, hipMemcpyAsync(const_cast<HrptGPULight*>(c->view.lights), lights, (size_t)count * sizeof(HrptGPULight), hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->view.lightCount = count;
    c->keptLights.assign(lights, lights + count);
    refresh_traits(c);
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_update_lights"); }

int hrpt_update_materials(HrptContext* c, const HrptMaterialConstants* materials, uint32_t firstMaterial, uint32_t count)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->haveScene) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_materials: no scene uploaded");
    if (count == 0) return HRPT_OK;
    if (!materials) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_materials: null material array");
    if ((uint64_t)firstMaterial + count > c->keptMaterials.size()) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_materials: range exceeds the scene's material count");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // The acceleration structure caches two things of a material: whether its triangles are opaque (any-hit / candidate handling) and
    // whether any material needs tangent frames. A change of either needs a rebuild; everything else is a plain buffer write.
    HrptSceneDesc before = kept_scene_desc(c);
    const bool tangentsBefore = scene_needs_tangents(before);
    bool structural = false;
    for (uint32_t i = 0; i < count; ++i)
        if (triangle_flags_for_material(materials[i]) != triangle_flags_for_material(c->keptMaterials[firstMaterial + i])) structural = true;   // opacity or shading class
    std::memcpy(c->keptMaterials.data() + firstMaterial, materials, (size_t)count * sizeof(HrptMaterialConstants));
    HIP_TRY(c, hipMemcpyAsync(const_cast<HrptMaterialConstants*>(c->view.materials) + firstMaterial, materials, (size_t)count * sizeof(HrptMaterialConstants), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HrptSceneDesc s = kept_scene_desc(c);
    if (scene_needs_tangents(s) != tangentsBefore) structural = true;
    if (structural) {
        SceneView v = c->view;
        int r = build_acceleration(c, s, kept_triangle_count(c), v, true);     // from scratch: the GPU builder's resident instance table holds the opacity flags
        if (r != HRPT_OK) { c->haveScene = false; return r; }
        c->view = v;
        c->perScene.motionInstStale = true;
    }
    refresh_traits(c);
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_update_materials"); }

int capi::update_instances_impl(HrptContext* c, const HrptPerInstanceData* instances, uint32_t firstInstance, uint32_t count, bool refit)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->haveScene) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_instances: no scene uploaded");
    if (count == 0) return HRPT_OK;
    if (!instances) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_instances: null instance array");
    if ((uint64_t)firstInstance + count > c->keptInstances.size()) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_instances: range exceeds the scene's instance count");
    for (uint32_t i = 0; i < count; ++i) {
        const HrptPerInstanceData& now = instances[i]; const HrptPerInstanceData& was = c->keptInstances[firstInstance + i];
        if (now.m_MeshDataIndex != was.m_MeshDataIndex || now.m_MaterialIndex != was.m_MaterialIndex || now.m_LODIndex != was.m_LODIndex)
            return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_instances: mesh, material and LOD of an instance cannot change (upload the scene again)");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // frames in flight still traverse the old tree
    std::memcpy(c->keptInstances.data() + firstInstance, instances, (size_t)count * sizeof(HrptPerInstanceData));
    ++c->instanceEpoch;
    c->perScene.motionInstStale = true;                          // m_PrevWorld travels in these records (hrpt_render_motion_vectors)
    HrptSceneDesc s = kept_scene_desc(c);
    const uint64_t sceneTris = kept_triangle_count(c);
    SceneView v = c->view;
    int r = build_acceleration(c, s, sceneTris, v, false, refit);
    if (r != HRPT_OK) { c->haveScene = false; return r; }   // the old tree is gone: the scene has to be uploaded again
    c->view = v;
    return HRPT_OK;
}
int hrpt_update_instances(HrptContext* c, const HrptPerInstanceData* instances, uint32_t firstInstance, uint32_t count)
try { return update_instances_impl(c, instances, firstInstance, count, false); } catch (...) { return caught(c, "hrpt_update_instances"); }
int hrpt_refit_instances(HrptContext* c, const HrptPerInstanceData* instances, uint32_t firstInstance, uint32_t count)
try { return update_instances_impl(c, instances, firstInstance, count, true); } catch (...) { return caught(c, "hrpt_refit_instances"); }
