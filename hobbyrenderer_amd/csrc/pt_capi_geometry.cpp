// pt_capi_geometry.cpp -- geometry that changes after the upload: keyframe animation (hrpt_animate), deforming meshes (hrpt_update_vertices*),
// skinning and morph targets in front of them, and their context-less host companions.
#include <chrono>

#include "pt_capi_internal.h"
#include "pt_deform.h"
#include "pt_skin.h"

using namespace hrt;
using namespace hrt::capi;

// ---- keyframe animation on the device: hrpt_animate and its companions (csrc/pt_anim.h has the definition) ----
static AnimDeviceCopy* find_animation_copy(HrptContext* c, const HrptAnimation* anim)
{
    for (AnimDeviceCopy& a : c->animations) if (a.anim == anim && a.serial == anim->serial) return &a;
    return nullptr;
}

// Uploads the resolved tables and seeds the state: once per (context, animation).
static int upload_animation(HrptContext* c, const HrptAnimation* anim, AnimDeviceCopy*& out)
{
    for (size_t i = 0; i < c->animations.size(); ++i)          // an address reused by a newer animation: the old copy is dead
        if (c->animations[i].anim == anim) { c->animations.erase(c->animations.begin() + (long)i); break; }
    AnimDeviceCopy a;
    a.anim = anim; a.serial = anim->serial;
    int r = HRPT_OK;
    auto put = [&](const auto& v, auto*& dev) {
        using T = typename std::remove_reference<decltype(v)>::type::value_type;
        const T* d = nullptr;
        if (r == HRPT_OK) r = upload(c, v.data(), v.size(), &d, &a.allocations);
        dev = const_cast<T*>(d);
    };
    HrptAnimSampler* samplers; float* keyTimes; float* keyValues; HrptAnimChannel* channels; uint32_t* targets; uint32_t* order; int32_t* orderParent;
    uint32_t* rangeNode; uint32_t* jointNode; float* inverseBind;
    put(anim->samplers, samplers); put(anim->keyTimes, keyTimes); put(anim->keyValues, keyValues); put(anim->channels, channels); put(anim->targets, targets);
    put(anim->order, order); put(anim->orderParent, orderParent); put(anim->rangeNode, rangeNode); put(anim->jointNode, jointNode); put(anim->inverseBind, inverseBind);
    put(anim->groupFirst, a.groupFirst); put(anim->times, a.times); put(anim->baseTrs, a.trs); put(anim->baseWorlds, a.worlds);
    const std::vector<float> zeroWeights(anim->morphWeightCount, 0.0f), zeroPalette(12 * anim->jointNode.size(), 0.0f);
    put(zeroWeights, a.weights); put(zeroPalette, a.palette);
    const std::vector<HrptPerInstanceData> zeroRecords(anim->rangeNode.size());
    put(zeroRecords, a.records);
    if (r == HRPT_OK && hipStreamSynchronize(c->stream) != hipSuccess) r = fail(c, HRPT_ERR_HIP, "hrpt_animate: table upload failed");   // the staging vectors above die here
    if (r != HRPT_OK) return r;                                 // (`a` frees what it holds)
    a.tables = anim->tables();
    a.tables.samplers = samplers; a.tables.keyTimes = keyTimes; a.tables.keyValues = keyValues; a.tables.channels = channels; a.tables.targets = targets;
    a.tables.order = order; a.tables.orderParent = orderParent; a.tables.rangeNode = rangeNode; a.tables.jointNode = jointNode; a.tables.inverseBind = inverseBind;
    c->animations.push_back(std::move(a));
    out = &c->animations.back();
    return HRPT_OK;
}

int hrpt_animate(HrptContext* c, const HrptAnimation* anim, uint32_t flags)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!anim) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animate: null animation");
    if (flags & ~(uint32_t)(HRPT_ANIMATE_REFIT | HRPT_ANIMATE_NO_COMMIT)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animate: unknown flag bits");
    const bool evaluateInstances = (flags & HRPT_ANIMATE_NO_COMMIT) == 0;
    if (evaluateInstances) {
        if (!c->haveScene) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animate: no scene uploaded");
        if (anim->instanceNeed > c->keptInstances.size()) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animate: an instance index of the animation exceeds the scene's instance count");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    AnimDeviceCopy* a = find_animation_copy(c, anim);
    if (!a) HRPT_TRY(upload_animation(c, anim, a));
    const uint32_t range = (uint32_t)anim->rangeNode.size();
    const bool commit = evaluateInstances && range > 0;
    if (!anim->times.empty()) HIP_TRY(c, hipMemcpyAsync(a->times, anim->times.data(), anim->times.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (commit && a->recordsEpoch != c->instanceEpoch) {       // something else wrote the instances since this copy was made
        HIP_TRY(c, hipMemcpyAsync(a->records, c->keptInstances.data() + anim->instanceFirst, (size_t)range * sizeof(HrptPerInstanceData), hipMemcpyHostToDevice, c->stream));
        a->recordsEpoch = 0;
    }
    // HRPT_ANIM_TIMING (scripts/anim_bench.py): device time of the kernels between events, host time of the read-back and of the commit, on stderr
    const bool timing = getenv("HRPT_ANIM_TIMING") != nullptr;
    if (timing) HIP_TRY(c, hipEventRecord(c->evStart, c->stream));
    HIP_TRY(c, launch_animate(a->tables, a->times, a->groupFirst, anim->groupFirst.data(), (uint32_t)anim->groupFirst.size() - 1u, a->trs, a->worlds, a->weights, a->palette,
                              commit ? a->records : nullptr, c->stream));
    float kernelMs = 0.0f;
    if (timing) {
        HIP_TRY(c, hipEventRecord(c->evStop, c->stream));
        HIP_TRY(c, hipEventSynchronize(c->evStop));
        HIP_TRY(c, hipEventElapsedTime(&kernelMs, c->evStart, c->evStop));
        if (!commit) fprintf(stderr, "[animate] kernels %.4f ms\n", kernelMs);
    }
    if (!commit) return HRPT_OK;                                // evaluation only, or no instance hangs under a composed node: nothing to commit, nothing to build
    const auto t0 = std::chrono::steady_clock::now();
    // the commit of hrpt_update_instances: the evaluated range comes back into the host copy, the rest of the roll is host work
    std::vector<HrptPerInstanceData> evaluated(range);
    HIP_TRY(c, hipMemcpyAsync(evaluated.data(), a->records, (size_t)range * sizeof(HrptPerInstanceData), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < c->keptInstances.size(); ++i)
        if (i < anim->instanceFirst || i - anim->instanceFirst >= range) std::memcpy(c->keptInstances[i].m_PrevWorld, c->keptInstances[i].m_World, sizeof(float) * 16);
    const auto t1 = std::chrono::steady_clock::now();
    const int r = update_instances_impl(c, evaluated.data(), anim->instanceFirst, range, (flags & HRPT_ANIMATE_REFIT) != 0);
    if (timing) fprintf(stderr, "[animate] kernels %.4f ms read-back and roll %.4f ms commit %.4f ms\n", kernelMs, std::chrono::duration<float, std::milli>(t1 - t0).count(),
                        std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t1).count());
    a = find_animation_copy(c, anim);
    if (a) a->recordsEpoch = r == HRPT_OK ? c->instanceEpoch : 0;
    return r;
} catch (...) { return caught(c, "hrpt_animate"); }

static int animation_pointers(HrptContext* c, const char* what, const HrptAnimation* anim, AnimDeviceCopy*& a)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!anim) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null animation");
    a = find_animation_copy(c, anim);
    if (!a) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": hrpt_animate has not run for this animation on this context");
    return HRPT_OK;
}
int hrpt_get_animation_device(HrptContext* c, const HrptAnimation* anim, void** palette, void** weights, void** nodeWorlds)
try {
    AnimDeviceCopy* a = nullptr;
    HRPT_TRY(animation_pointers(c, "hrpt_get_animation_device", anim, a));
    if (palette) *palette = anim->jointNode.empty() ? nullptr : a->palette;
    if (weights) *weights = anim->morphWeightCount ? a->weights : nullptr;
    if (nodeWorlds) *nodeWorlds = anim->nodes.empty() ? nullptr : a->worlds;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_get_animation_device"); }
int hrpt_read_animation(HrptContext* c, const HrptAnimation* anim, float* palette, float* weights, float* nodeWorlds)
try {
    AnimDeviceCopy* a = nullptr;
    HRPT_TRY(animation_pointers(c, "hrpt_read_animation", anim, a));
    HIP_TRY(c, hipSetDevice(c->device));
    if (palette && !anim->jointNode.empty()) HIP_TRY(c, hipMemcpyAsync(palette, a->palette, anim->jointNode.size() * 12 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (weights && anim->morphWeightCount) HIP_TRY(c, hipMemcpyAsync(weights, a->weights, anim->morphWeightCount * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (nodeWorlds && !anim->nodes.empty()) HIP_TRY(c, hipMemcpyAsync(nodeWorlds, a->worlds, anim->nodes.size() * 16 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_read_animation"); }
int hrpt_animation_release(HrptContext* c, const HrptAnimation* anim)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!anim) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animation_release: null animation");
    HIP_TRY(c, hipSetDevice(c->device));
    for (size_t i = 0; i < c->animations.size(); ++i)
        if (c->animations[i].anim == anim) {
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            c->animations.erase(c->animations.begin() + (long)i);
            break;
        }
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_animation_release"); }

// ---- deforming meshes: hrpt_update_vertices / hrpt_update_vertices_device (include/hobbyrt_pt.h has the contract) ----
constexpr uint32_t kVertexUpdateFlags = HRPT_VERTICES_REFIT | HRPT_VERTICES_SAME_FRAME;

// The argument checks both variants share (the answer without a scene is hrpt_update_instances').
static int check_vertex_update(HrptContext* c, const char* what, const void* vertices, uint32_t firstVertex, uint32_t count, uint32_t flags)
{
    if (!c->haveScene) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": no scene uploaded");
    if (flags & ~kVertexUpdateFlags) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": unknown flag bits");
    if (!vertices && count > 0) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null vertex array");
    if ((uint64_t)firstVertex + count > c->keptVertices.size()) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": range exceeds the scene's vertex count");
    return HRPT_OK;
}

// The previous-position protocol: a call without HRPT_VERTICES_SAME_FRAME starts a frame (previous = current everywhere), every call records
// the positions it is about to replace. While no call has recorded anything the table stays empty, which stands for previous == current.
static void roll_previous_positions(HrptContext* c, uint32_t firstVertex, uint32_t count, uint32_t flags)
{
    const bool newFrame = (flags & HRPT_VERTICES_SAME_FRAME) == 0;
    if (count == 0) {
        if (newFrame && !c->perScene.keptPrevPositions.empty()) { c->perScene.keptPrevPositions.clear(); c->perScene.motionPositionsStale = true; }
        return;
    }
    if (newFrame || c->perScene.keptPrevPositions.empty()) {
        c->perScene.keptPrevPositions.resize(c->keptVertices.size() * 3);
        for (size_t i = 0; i < c->keptVertices.size(); ++i) std::memcpy(&c->perScene.keptPrevPositions[3 * i], c->keptVertices[i].m_Pos, 12);
    } else {
        for (size_t i = firstVertex; i < (size_t)firstVertex + count; ++i) std::memcpy(&c->perScene.keptPrevPositions[3 * i], c->keptVertices[i].m_Pos, 12);
    }
    c->perScene.motionPositionsStale = true;
}

// Installs validated vertices: `quantised` (host, count records) goes into the kept copy; a flat structure's GPU builder gets its device
// buffer patched from `deviceQuantised` when the records are already on the device, from the host array otherwise; then the structure follows.
static int commit_vertices(HrptContext* c, const char* what, const HrptVertexQuantized* quantised, const HrptVertexQuantized* deviceQuantised,
                           uint32_t firstVertex, uint32_t count, uint32_t flags)
{
    roll_previous_positions(c, firstVertex, count, flags);
    std::memcpy(c->keptVertices.data() + firstVertex, quantised, (size_t)count * sizeof(HrptVertexQuantized));
    const bool twoLevel = c->twoLevel != nullptr;
    if (!twoLevel && c->gpuBuilder) {
        std::string gerr;
        const hipError_t e = c->gpuBuilder->update_vertices(deviceQuantised ? deviceQuantised : quantised, deviceQuantised != nullptr, firstVertex, count, c->stream, gerr);
        if (e != hipSuccess) { c->haveScene = false; return fail(c, HRPT_ERR_HIP, std::string(what) + ": " + gerr + ": " + hipGetErrorString(e)); }
    }
    HrptSceneDesc s = kept_scene_desc(c);
    SceneView v = c->view;
    // flat: a rebuild like hrpt_update_instances' (the GPU builder keeps its buffers; the host builder starts from the kept copy). Two-level: the
    // mesh trees hold the old vertices, so the whole structure is built again along the first-build path.
    const int r = build_acceleration(c, s, kept_triangle_count(c), v, twoLevel, (flags & HRPT_VERTICES_REFIT) != 0);
    if (r != HRPT_OK) { c->haveScene = false; return r; }   // the old tree is gone: the scene has to be uploaded again
    c->view = v;
    return HRPT_OK;
}

int hrpt_update_vertices(HrptContext* c, const HrptVertexQuantized* vertices, uint32_t firstVertex, uint32_t count, uint32_t flags)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(check_vertex_update(c, "hrpt_update_vertices", vertices, firstVertex, count, flags));
    for (uint32_t i = 0; i < count; ++i)
        if (!deform::position_finite(vertices[i].m_Pos)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_vertices: non-finite vertex position");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // frames in flight still traverse the old tree and read the old motion tables
    if (count == 0) { roll_previous_positions(c, 0, 0, flags); return HRPT_OK; }
    return commit_vertices(c, "hrpt_update_vertices", vertices, nullptr, firstVertex, count, flags);
} catch (...) { return caught(c, "hrpt_update_vertices"); }

// What hrpt_update_vertices_device and hrpt_update_vertices_skinned share once their arguments are checked: `launch(staged, dStatus2)` puts
// a kernel on the context's stream that writes `count` quantised records into the staging buffer and raises the two status words behind
// them (word 0: a position that is not finite; word 1: a joint index out of range); nothing is committed before both are known to be clear.
template <class Launch>
static int update_vertices_staged(HrptContext* c, const std::string& what, uint32_t firstVertex, uint32_t count, uint32_t flags, hipStream_t stream, Launch launch)
{
    constexpr size_t kStatusBytes = 2 * sizeof(uint32_t);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (count == 0) { roll_previous_positions(c, 0, 0, flags); return HRPT_OK; }
    HIP_TRY(c, hipStreamSynchronize(stream));           // whatever writes the caller's arrays has to be done before the kernel below reads them
    const size_t recordBytes = (size_t)count * sizeof(HrptVertexQuantized);
    HIP_TRY(c, c->perScene.dDeformStaging.reserve(c->keptVertices.size() * sizeof(HrptVertexQuantized) + kStatusBytes));      // once per scene: room for the whole vertex buffer + the status words
    if (recordBytes + kStatusBytes > c->perScene.dDeformStaging.bytes()) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": range exceeds the staging buffer");
    HrptVertexQuantized* staged = static_cast<HrptVertexQuantized*>(c->perScene.dDeformStaging.get());
    uint32_t* dStatus = reinterpret_cast<uint32_t*>(static_cast<char*>(c->perScene.dDeformStaging.get()) + recordBytes);
    HIP_TRY(c, hipMemsetAsync(dStatus, 0, kStatusBytes, c->stream));
    HIP_TRY(c, launch(staged, dStatus));
    // the copy-back that keeps the host copy current also brings the status words
    std::vector<HrptVertexQuantized> host((recordBytes + kStatusBytes + sizeof(HrptVertexQuantized) - 1) / sizeof(HrptVertexQuantized));
    HIP_TRY(c, hipMemcpyAsync(host.data(), staged, recordBytes + kStatusBytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint32_t status[2] = { 0, 0 };
    std::memcpy(status, reinterpret_cast<const char*>(host.data()) + recordBytes, sizeof status);
    if (status[1]) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": joint index out of range");
    if (status[0]) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": non-finite vertex position");
    return commit_vertices(c, what.c_str(), host.data(), staged, firstVertex, count, flags);
}

int hrpt_update_vertices_device(HrptContext* c, const HrptVertexFloat* deviceVertices, uint32_t firstVertex, uint32_t count, uint32_t flags, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(check_vertex_update(c, "hrpt_update_vertices_device", deviceVertices, firstVertex, count, flags));
    if (reinterpret_cast<uintptr_t>(deviceVertices) & 15u) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_vertices_device: deviceVertices must be 16-byte aligned");
    return update_vertices_staged(c, "hrpt_update_vertices_device", firstVertex, count, flags, static_cast<hipStream_t>(stream), [&](HrptVertexQuantized* staged, uint32_t* dStatus) {
        return launch_quantise_vertices(deviceVertices, count, staged, dStatus, c->stream);
    });
} catch (...) { return caught(c, "hrpt_update_vertices_device"); }

// ---- the producer in front: hrpt_skin_vertices_host / _device, hrpt_update_vertices_skinned (csrc/pt_skin.h has the definition) ----
// The argument checks all three share.
static int skin_args_check(HrptContext* c, const char* what, const HrptSkinArgs* a)
{
    const std::string w(what);
    auto misaligned = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (!a) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": null args");
    if (a->reserved != 0) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": reserved must be 0");
    if (misaligned(a->base, 15) || misaligned(a->joints, 7) || misaligned(a->weights, 15) || misaligned(a->jointMatrices, 15) || misaligned(a->deltas, 3) ||
        misaligned(a->morphWeights, 3))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": base, weights and jointMatrices must be 16-byte aligned, joints 8-byte, deltas and morphWeights 4-byte");
    if (a->joints && (!a->weights || !a->jointMatrices || a->jointCount == 0)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": joints need weights, jointMatrices and a jointCount > 0");
    if (a->targetCount > 0 && (!a->deltas || !a->morphWeights)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": targetCount > 0 needs deltas and morphWeights");
    if (!a->base && a->count > 0) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": null base");
    return HRPT_OK;
}

// HRPT_SKIN_PALETTE=1: gather every palette from global memory (the A/B of scripts/skin_bench.py); anything else: by joint count
static int skin_palette_mode() { const char* e = getenv("HRPT_SKIN_PALETTE"); return e ? atoi(e) : 0; }

int hrpt_update_vertices_skinned(HrptContext* c, const HrptSkinArgs* args, uint32_t firstVertex, uint32_t flags, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(skin_args_check(c, "hrpt_update_vertices_skinned", args));
    HRPT_TRY(check_vertex_update(c, "hrpt_update_vertices_skinned", args->base, firstVertex, args->count, flags));
    // Two kernels on the context's stream, the skinned floats in a buffer of the context between them. A kernel that quantised in
    // registers instead was measured no faster than this and is not kept.
    return update_vertices_staged(c, "hrpt_update_vertices_skinned", firstVertex, args->count, flags, static_cast<hipStream_t>(stream), [&](HrptVertexQuantized* staged, uint32_t* dStatus) {
        if (!c->perScene.dSkinFloats) {                          // once per scene: room for the whole vertex buffer
            const hipError_t e = c->perScene.dSkinFloats.alloc(c->keptVertices.size() * sizeof(HrptVertexFloat));
            if (e != hipSuccess) return e;
        }
        const hipError_t e = launch_skin_vertices(*args, c->perScene.dSkinFloats, dStatus, skin_palette_mode(), c->stream);
        return e != hipSuccess ? e : launch_quantise_vertices(c->perScene.dSkinFloats, args->count, staged, dStatus, c->stream);
    });
} catch (...) { return caught(c, "hrpt_update_vertices_skinned"); }

int hrpt_skin_vertices_device(HrptContext* c, const HrptSkinArgs* args, HrptVertexFloat* deviceOut, uint32_t* deviceStatus2, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(skin_args_check(c, "hrpt_skin_vertices_device", args));
    if (args->count == 0) return HRPT_OK;
    if (!deviceOut || (reinterpret_cast<uintptr_t>(deviceOut) & 15u) || (reinterpret_cast<uintptr_t>(deviceStatus2) & 3u))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_skin_vertices_device: deviceOut must be 16-byte aligned and not NULL, deviceStatus2 4-byte aligned");
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(args->base), out0 = reinterpret_cast<uintptr_t>(deviceOut), bytes = (uintptr_t)args->count * sizeof(HrptVertexFloat);
    if (in0 < out0 + bytes && out0 < in0 + bytes) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_skin_vertices_device: deviceOut overlaps base");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_skin_vertices(*args, deviceOut, deviceStatus2, skin_palette_mode(), static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_skin_vertices_device"); }
int hrpt_quantize_vertices_device(HrptContext* c, const HrptVertexFloat* deviceIn, uint32_t count, HrptVertexQuantized* deviceOut, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (count == 0) return HRPT_OK;
    if (!deviceIn || !deviceOut) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_quantize_vertices_device: null array");
    if ((reinterpret_cast<uintptr_t>(deviceIn) & 15u) || (reinterpret_cast<uintptr_t>(deviceOut) & 3u))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_quantize_vertices_device: deviceIn must be 16-byte aligned, deviceOut 4-byte aligned");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_quantise_vertices(deviceIn, count, deviceOut, nullptr, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_quantize_vertices_device"); }

int hrpt_quantize_vertices_host(const HrptVertexFloat* in, uint32_t count, HrptVertexQuantized* out, int nthreads)
{
    if (count == 0) return HRPT_OK;
    if (!in || !out) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_quantize_vertices_host: null array");
    return run_host("hrpt_quantize_vertices_host", [&] { (void)quantize_vertices_host(in, count, out, host_threads(nthreads)); });
}
// ---- keyframe animation without a context: the tables, the clock and the host executor (csrc/pt_anim_host.cpp) ----
int hrpt_animation_create(const HrptAnimationDesc* desc, HrptAnimation** out)
{
    if (!out) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animation_create: null out");
    *out = nullptr;
    if (!desc) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animation_create: null desc");
    std::string err;
    HRPT_TRY(run_host("hrpt_animation_create", [&] { *out = animation_create(*desc, err); }));
    return *out ? HRPT_OK : fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animation_create: " + err);
}
void hrpt_animation_destroy(HrptAnimation* anim) { delete anim; }
int hrpt_animation_advance(HrptAnimation* anim, float dt)
{
    if (!anim) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animation_advance: null animation");
    animation_advance(*anim, dt);
    return HRPT_OK;
}
int hrpt_animation_set_times(HrptAnimation* anim, const float* times, uint32_t count)
{
    if (!anim || count != anim->times.size() || (count && !times)) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animation_set_times: null argument, or count is not the animation count");
    for (uint32_t i = 0; i < count; ++i) anim->times[i] = times[i];
    return HRPT_OK;
}
int hrpt_animation_get_times(const HrptAnimation* anim, float* times, float* durations, uint32_t count)
{
    if (!anim || count != anim->times.size()) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animation_get_times: null animation, or count is not the animation count");
    for (uint32_t i = 0; i < count; ++i) { if (times) times[i] = anim->times[i]; if (durations) durations[i] = anim->durations[i]; }
    return HRPT_OK;
}
int hrpt_animate_host(const HrptAnimation* anim, const HrptPerInstanceData* prevInstances, HrptPerInstanceData* instancesInOut, uint32_t instanceCount,
                      float* paletteOut, float* weightsOut, float* nodeWorldsOut, int nthreads)
{
    if (!anim) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animate_host: null animation");
    if (instancesInOut && anim->instanceNeed > instanceCount) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animate_host: an instance index of the animation exceeds instanceCount");
    return run_host("hrpt_animate_host", [&] {
        if (instancesInOut && prevInstances && prevInstances != instancesInOut) std::memmove(instancesInOut, prevInstances, (size_t)instanceCount * sizeof(HrptPerInstanceData));
        animate_host(*anim, instancesInOut, instancesInOut ? instanceCount : 0u, paletteOut, weightsOut, nodeWorldsOut, host_threads(nthreads));
    });
}

int hrpt_skin_vertices_host(const HrptSkinArgs* args, HrptVertexFloat* out, int nthreads)
{
    HRPT_TRY(skin_args_check(nullptr, "hrpt_skin_vertices_host", args));
    if (args->count == 0) return HRPT_OK;
    if (!out) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_skin_vertices_host: null out");
    uint32_t status = 0;
    HRPT_TRY(run_host("hrpt_skin_vertices_host", [&] { status = skin_vertices_host(*args, out, host_threads(nthreads)); }));
    if (status & skin::kJointOutOfRange) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_skin_vertices_host: joint index out of range");
    return HRPT_OK;
}
