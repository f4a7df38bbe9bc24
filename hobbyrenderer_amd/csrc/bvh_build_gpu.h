// bvh_build_gpu.h -- GPU construction of the acceleration structure (see bvh_build_gpu.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <string>

#include "../../include/hobbyrt_pt.h"
#include "pt_scene_records.h"

namespace hrt {

struct GpuBuiltBvh {            // device pointers owned by the GpuBvhBuilder that produced them (valid until its next build() / destruction)
    GpuNode* nodes = nullptr; uint32_t nodeCount = 0;
    GpuNode4* nodes4 = nullptr; uint32_t node4Count = 0; uint32_t nodes4Capacity = 0;   // capacity: records the nodes4 buffer holds (>= node4Count, checked before the emission)
    GpuTri* tris = nullptr; GpuTriAttr* attrs = nullptr; GpuTriTangent* tangents = nullptr; uint32_t triCount = 0;
    uint32_t maxDepth = 0, maxDepth4 = 0;
    bool ploc = false;          // hierarchy by PLOC (nearest-neighbour clustering) rather than the Morton radix tree
    uint32_t mortonBits = 0;    // Morton bits the hierarchy used (63, or fewer when the full-code tree was too deep)
    float sahCost = 0.0f;       // surface-area-heuristic cost of the 2-wide tree (node cost 1, triangle cost 1), root area = 1
    float deviceMs = 0.0f;      // instance upload .. last kernel
    bool refitted = false;      // boxes refitted on the hierarchy of an earlier build (GpuBvhBuilder::refit)
    const uint32_t* leafOrder = nullptr;   // primitive (input index) at every position of the leaf order the leaf references count in
};

// Why a prepare / build / refit did not give a tree, as a value: the caller decides by `reason` (refuse the scene, report the allocation, or build on
// the host instead); `message` is for people (hrpt_last_error).
enum class GpuBuildFailure {
    None,
    NonFinitePosition,      // a world-space vertex position is infinite or NaN: the scene is invalid for every builder
    OutOfMemory,            // the device refused an allocation
    DoesNotFit,             // primitive count outside the builder's range, or a 4-wide tree larger than its node buffer
    DeviceError,            // a HIP call or kernel launch failed, or the builder was asked for something it was not prepared for
};
struct GpuBuildError { GpuBuildFailure reason = GpuBuildFailure::None; std::string message; };

// Keeps the scene's geometry (quantised vertices, indices) and every build buffer on the device, so that a rebuild after a transform
// change (hrpt_update_instances; the reference's per-frame TLAS rebuild, src/CommonRenderers.cpp:234-246) only uploads the instance
// table and runs the kernels: no allocation, no geometry traffic over PCIe.
class GpuBvhBuilder {
public:
    GpuBvhBuilder();
    GpuBvhBuilder(const GpuBvhBuilder&) = delete;
    GpuBvhBuilder& operator=(const GpuBvhBuilder&) = delete;
    ~GpuBvhBuilder();            // (both defined where Impl is complete)
    // `scene` must already be validated (bvh_build.h validate_scene). Triangle counts below 8 are not handled (the caller uses the
    // host builder). Copies vertices / indices to the device and sizes all buffers for this scene's triangle count.
    hipError_t prepare(const HrptSceneDesc& scene, bool needTangents, hipStream_t stream, GpuBuildError& error);
    // (Re)builds from the world matrices of `instances` (as many as at prepare(), same mesh / material indices). The tree is rebuilt
    // with fewer Morton bits until maxDepth + 2 <= maxStackDepth (the caller still checks the final depth). Synchronises `stream`.
    hipError_t build(const HrptPerInstanceData* instances, bool usePloc, uint32_t maxStackDepth, hipStream_t stream, GpuBuiltBvh& out, GpuBuildError& error);
    // Deforming meshes (hrpt_update_vertices): overwrites the records [first, first + count) of the device vertex buffer prepare() filled, from
    // host memory or (`fromDevice`) from device memory, on `stream`; the caller has checked the range against the scene's vertex count and the
    // positions for finiteness. The hierarchy of the last build stays refittable: the next build() or refit() brings everything derived after.
    hipError_t update_vertices(const HrptVertexQuantized* vertices, bool fromDevice, uint32_t first, uint32_t count, hipStream_t stream, std::string& error);
    size_t deviceBytes() const;
    // Box mode -- the tree over the instances of the two-level structure (pt_capi.cpp build_two_level): `count` boxes (6 floats each, min xyz
    // then max xyz, taken as they are), one per leaf, Morton grid over the cube of the largest extent. The result has nodes / nodes4 /
    // leafOrder only; a leaf reference ~(k << 2) names box leafOrder[k].
    hipError_t prepare_boxes(uint32_t count, hipStream_t stream, GpuBuildError& error);
    hipError_t build_boxes(const float* boxes, bool usePloc, uint32_t maxStackDepth, hipStream_t stream, GpuBuiltBvh& out, GpuBuildError& error);
    // New boxes on the hierarchy of the last successful build() / build_boxes() (same primitives, moved): no sort, no hierarchy construction.
    // The tree stays valid whatever the motion (every box is recomputed bottom-up); its quality is that of the old topology on the new positions.
    bool can_refit() const;
    hipError_t refit(const HrptPerInstanceData* instances, hipStream_t stream, GpuBuiltBvh& out, GpuBuildError& error);
    hipError_t refit_boxes(const float* boxes, hipStream_t stream, GpuBuiltBvh& out, GpuBuildError& error);
private:
    hipError_t allocate(uint32_t n, const HrptSceneDesc* scene, bool needTangents, hipStream_t stream, GpuBuildError& error);
    struct Impl;
    std::unique_ptr<Impl> p;
};
// copies the `count` 4-wide nodes of a tree built in box mode to `dst`, leaves rewritten as two-level instance references ~(instance << 2)
hipError_t launch_tlas_fixup(const GpuNode4* src, uint32_t count, const uint32_t* leafOrder, GpuNode4* dst, hipStream_t stream);

} // namespace hrt
