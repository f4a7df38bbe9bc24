// pt_capi_render.cpp -- what traces rays: hrpt_render, the first-hit G-buffer and motion vectors, hrpt_trace_rays, hrpt_trace_radiance, the
// resolves and hrpt_allgather.
#include "pt_capi_internal.h"

using namespace hrt;
using namespace hrt::capi;

// The checks every frame shares, in this order: the viewport against hrpt_resize, the stripe, the tile rectangle (all zero = the whole
// image). Fills `rect`.
static int frame_rect(HrptContext* c, const std::string& what, const HrptFrameParams& p, TileRect& rect)
{
    const uint32_t vw = (uint32_t)p.constants.m_View.m_ViewportSize[0], vh = (uint32_t)p.constants.m_View.m_ViewportSize[1];
    if (vw != c->width || vh != c->height) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": m_ViewportSize does not match hrpt_resize");
    rect.x0 = p.tileX0; rect.y0 = p.tileY0; rect.x1 = p.tileX1; rect.y1 = p.tileY1;
    rect.stripeCount = p.stripeCount ? p.stripeCount : 1u; rect.stripeIndex = p.stripeIndex;
    if (rect.stripeIndex >= rect.stripeCount) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": stripeIndex must be below stripeCount");
    if (rect.x0 == 0 && rect.y0 == 0 && rect.x1 == 0 && rect.y1 == 0) { rect.x1 = c->width; rect.y1 = c->height; }
    if (rect.x1 > c->width || rect.y1 > c->height || rect.x0 > rect.x1 || rect.y0 > rect.y1)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": tile rectangle outside the image");
    return HRPT_OK;
}

int hrpt_render(HrptContext* c, const HrptFrameParams* p)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_render: null params");
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, "hrpt_render: no scene uploaded");
    if (!c->perSize.dAccum) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_render: hrpt_resize not called");
    if (p->accumCount == 0) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_render: accumCount == 0");
    if (p->constants.m_MaxBounces > 64u) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_render: m_MaxBounces above 64 (the reference's UI stops at 12, src/ImGuiLayer.cpp:760; one kernel sequence is launched per bounce)");
    if (p->constants.m_LightCount > c->view.lightCount) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_render: m_LightCount exceeds the scene's light buffer");
    TileRect rect;
    HRPT_TRY(frame_rect(c, "hrpt_render", *p, rect));
    HIP_TRY(c, hipSetDevice(c->device));

    bool wavefront = (p->flags & HRPT_FRAME_MEGAKERNEL) == 0 && wavefront_supports(c->view, p->constants);
    if (!wavefront && c->view.instances && exceeds_private_stack(c->traits))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_render: this two-level structure is deeper than the validation megakernel's 64-entry stack");
    if (!wavefront && (p->flags & HRPT_FRAME_MEGAKERNEL) == 0) c->megakernelFallbacks++;
    HIP_TRY(c, hipEventRecord(c->evStart, c->stream));
    if (wavefront) {
        std::string werr;
        c->wf.profile = (p->flags & HRPT_FRAME_PROFILE) != 0;
        c->wf.shadeInstances = (uint32_t)c->keptInstances.size(); c->wf.shadeMaterials = (uint32_t)c->keptMaterials.size();    // as uploaded / last updated
        hipError_t e = wavefront_render(c->wf, c->view, c->traits, p->constants, p->accumCount, c->perSize.dAccum, c->perSize.dOutput, c->width, c->height, rect,
                                        c->perContext.dCounters, c->stream, werr);
        if (e != hipSuccess) return fail(c, hip_status(e), "wavefront_render: " + werr + ": " + hipGetErrorString(e));
    } else {
        for (uint32_t k = 0; k < p->accumCount; ++k) {
            HrptPathTracerConstants cb = p->constants;
            cb.m_AccumulationIndex = p->constants.m_AccumulationIndex + k;                 // PathTracerRenderer.cpp:62,:105
            cb.m_Jitter[0] = hrpt_halton(cb.m_AccumulationIndex + 1, 2) - 0.5f;            // :65
            cb.m_Jitter[1] = hrpt_halton(cb.m_AccumulationIndex + 1, 3) - 0.5f;
            HIP_TRY(c, launch_megakernel(c->view, cb, c->perSize.dAccum, c->perSize.dOutput, c->width, rect, c->perContext.dCounters, c->stream));
        }
    }
    HIP_TRY(c, hipEventRecord(c->evStop, c->stream));
    c->timed = true;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_render"); }

// The device tables of hrpt_render_motion_vectors, (re)built from the kept copies where a flag says they are stale: the instance records after
// every upload / instance update / rebuild, indices after an upload only, positions after an upload and after hrpt_update_vertices (12 bytes
// per vertex from the kept copy, and as much again for the previous positions while a deformation lasts). A context that never asks for
// motion never gets here.
static int refresh_motion_tables(HrptContext* c)
{
    if (!c->perScene.motionInstStale && !c->perScene.motionGeometryStale && !c->perScene.motionPositionsStale) return HRPT_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // motion calls in flight still read the old tables
    std::vector<float> positions;
    const size_t pb = c->keptVertices.size() * 3 * sizeof(float);
    if (c->perScene.motionGeometryStale) {
        c->perScene.dMotionPositions.reset(); c->perScene.dMotionPrevPositions.reset(); c->perScene.dMotionIndices.reset();   // all three go before anything is allocated
        const size_t ib = c->keptIndices.size() * sizeof(uint32_t);
        HIP_TRY(c, c->perScene.dMotionPositions.alloc(pb ? pb : 16));
        HIP_TRY(c, c->perScene.dMotionIndices.alloc(ib ? ib : 16));
        if (ib) HIP_TRY(c, hipMemcpyAsync(c->perScene.dMotionIndices, c->keptIndices.data(), ib, hipMemcpyHostToDevice, c->stream));
        c->perScene.motionPositionsStale = true;
    }
    if (c->perScene.motionPositionsStale) {
        positions.resize(c->keptVertices.size() * 3);
        for (size_t i = 0; i < c->keptVertices.size(); ++i) std::memcpy(&positions[3 * i], c->keptVertices[i].m_Pos, 12);
        if (pb) HIP_TRY(c, hipMemcpyAsync(c->perScene.dMotionPositions, positions.data(), pb, hipMemcpyHostToDevice, c->stream));
        if (!c->perScene.keptPrevPositions.empty()) {            // (same size as `positions`: hrpt_update_vertices fills it for all vertices)
            if (!c->perScene.dMotionPrevPositions) HIP_TRY(c, c->perScene.dMotionPrevPositions.alloc(pb ? pb : 16));
            if (pb) HIP_TRY(c, hipMemcpyAsync(c->perScene.dMotionPrevPositions, c->perScene.keptPrevPositions.data(), pb, hipMemcpyHostToDevice, c->stream));
        }
    }
    std::vector<MotionInst> records(c->keptInstances.size());
    for (size_t i = 0; i < records.size(); ++i) {
        const HrptPerInstanceData& in = c->keptInstances[i];
        MotionInst& r = records[i];
        for (int row = 0; row < 4; ++row) for (int k = 0; k < 3; ++k) r.prevWorld[row * 3 + k] = in.m_PrevWorld[row * 4 + k];
        r.firstIndex = c->keptMeshData[in.m_MeshDataIndex].m_IndexOffsets[0];         // LOD 0 (PathTracer.hlsl:102-103)
        r.pad[0] = r.pad[1] = r.pad[2] = 0;
    }
    HIP_TRY(c, c->perScene.dMotionInst.reserve(records.empty() ? 64 : records.size() * sizeof(MotionInst)));
    if (!records.empty()) HIP_TRY(c, hipMemcpyAsync(c->perScene.dMotionInst, records.data(), records.size() * sizeof(MotionInst), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // the staging vectors die at scope exit
    c->perScene.motionInstStale = c->perScene.motionGeometryStale = c->perScene.motionPositionsStale = false;
    return HRPT_OK;
}

// First-hit G-buffer: the checks of hrpt_render that apply (no bounces, no lights), then one of the two kernel paths. No events, no counters, no
// fallback count: HrptStats keeps describing renders. hrpt_render_motion_vectors (`motion`) is the same pass with the motion plane written too
// and a planeMask that may be 0.
static int render_gbuffer_impl(HrptContext* c, const HrptFrameParams* p, uint32_t planeMask, bool motion, const HrptPlanarViewConstants* prevView)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    const std::string what = motion ? "hrpt_render_motion_vectors" : "hrpt_render_gbuffer";
    if (!p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": null params");
    if (motion && !prevView) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": null prevView (pass the current view for a camera that did not move)");
    if ((planeMask == 0 && !motion) || (planeMask >> HRPT_GB_PLANES) != 0)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + (motion ? ": planeMask names G-buffer planes (bits 0..5) only" : ": planeMask must name at least one of the HRPT_GB_PLANES planes and no other bit"));
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, what + ": no scene uploaded");
    if (!c->perSize.dAccum) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": hrpt_resize not called");
    if (p->accumCount != 1) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": accumCount must be 1 (the planes describe path vertex 0 of ONE accumulation index)");
    TileRect rect;
    HRPT_TRY(frame_rect(c, what, *p, rect));
    HIP_TRY(c, hipSetDevice(c->device));
    const bool wavefront = (p->flags & HRPT_FRAME_MEGAKERNEL) == 0;
    if (!wavefront && c->view.instances && exceeds_private_stack(c->traits))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": this two-level structure is deeper than the validation kernel's 64-entry stack");
    const size_t bytes = (size_t)c->width * c->height * sizeof(float4);
    for (uint32_t k = 0; k < HRPT_GB_PLANES; ++k) {
        if ((planeMask & (1u << k)) && !c->perSize.dGBuffer[k]) HRPT_TRY(realloc_image(c, c->perSize.dGBuffer[k], bytes));
    }
    float4* planes[HRPT_GB_PLANES];             // what the kernels take: the plain pointers
    for (uint32_t k = 0; k < HRPT_GB_PLANES; ++k) planes[k] = c->perSize.dGBuffer[k];
    MotionArgs m{};
    if (motion) {
        if (!c->perSize.dMotion) HRPT_TRY(realloc_image(c, c->perSize.dMotion, bytes));
        int r = refresh_motion_tables(c);
        if (r != HRPT_OK) return r;
        m.inst = c->perScene.dMotionInst; m.positions = c->perScene.dMotionPositions; m.prevPositions = c->perScene.keptPrevPositions.empty() ? c->perScene.dMotionPositions : c->perScene.dMotionPrevPositions; m.indices = c->perScene.dMotionIndices; m.plane = c->perSize.dMotion;
        std::memcpy(m.prevWorldToClip, prevView->m_MatWorldToClip, sizeof m.prevWorldToClip);
        m.prevScale[0] = prevView->m_ClipToWindowScale[0]; m.prevScale[1] = prevView->m_ClipToWindowScale[1];
        m.prevBias[0] = prevView->m_ClipToWindowBias[0]; m.prevBias[1] = prevView->m_ClipToWindowBias[1];
    }
    if (wavefront) {
        std::string werr;
        hipError_t e = wavefront_gbuffer(c->wf, c->view, c->traits, p->constants, planes, planeMask, c->width, rect, c->stream, werr, motion ? &m : nullptr);
        if (e != hipSuccess) return fail(c, hip_status(e), "wavefront_gbuffer: " + werr + ": " + hipGetErrorString(e));
    } else if (motion) HIP_TRY(c, launch_motion_megakernel(c->view, p->constants, planes, planeMask, m, c->width, rect, c->stream));
    else HIP_TRY(c, launch_gbuffer_megakernel(c->view, p->constants, planes, planeMask, c->width, rect, c->stream));
    return HRPT_OK;
}
int hrpt_render_gbuffer(HrptContext* c, const HrptFrameParams* p, uint32_t planeMask)
try { return render_gbuffer_impl(c, p, planeMask, false, nullptr); } catch (...) { return caught(c, "hrpt_render_gbuffer"); }
int hrpt_render_motion_vectors(HrptContext* c, const HrptFrameParams* p, const HrptPlanarViewConstants* prevView, uint32_t planeMask)
try { return render_gbuffer_impl(c, p, planeMask, true, prevView); } catch (...) { return caught(c, "hrpt_render_motion_vectors"); }
int hrpt_read_motion_vectors(HrptContext* c, float* dst, size_t bytes)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->perSize.dMotion) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_read_motion_vectors: the motion plane was never requested from hrpt_render_motion_vectors");
    return read_image(c, c->perSize.dMotion, dst, bytes, "hrpt_read_motion_vectors");
} catch (...) { return caught(c, "hrpt_read_motion_vectors"); }
int hrpt_get_motion_vectors_device(HrptContext* c, void** devicePtr)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!devicePtr) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_motion_vectors_device: null out");
    *devicePtr = c->perSize.dMotion;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_get_motion_vectors_device"); }
int hrpt_read_gbuffer(HrptContext* c, uint32_t plane, void* dst, size_t bytes)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (plane >= HRPT_GB_PLANES) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_read_gbuffer: unknown plane");
    if (!c->perSize.dGBuffer[plane]) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_read_gbuffer: plane " + std::to_string(plane) + " was never requested from hrpt_render_gbuffer");
    return read_image(c, c->perSize.dGBuffer[plane], static_cast<float*>(dst), bytes, "hrpt_read_gbuffer");
} catch (...) { return caught(c, "hrpt_read_gbuffer"); }
int hrpt_get_gbuffer_device(HrptContext* c, uint32_t plane, void** devicePtr)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (plane >= HRPT_GB_PLANES || !devicePtr) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_gbuffer_device: unknown plane or null out");
    *devicePtr = c->perSize.dGBuffer[plane];
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_get_gbuffer_device"); }

int hrpt_resolve_output(HrptContext* c)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->perSize.dAccum) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_resolve_output: hrpt_resize not called");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_resolve(c->perSize.dAccum, c->perSize.dOutput, c->width * c->height, c->stream));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_resolve_output"); }

int hrpt_resolve_device(HrptContext* c, const float* accumulationDevice, float* outputDevice, uint64_t pixelCount, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!accumulationDevice || !outputDevice) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_resolve_device: null image");
    if (pixelCount == 0) return HRPT_OK;
    if (pixelCount > 0xFFFFFFFFull) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_resolve_device: image too large");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_resolve(reinterpret_cast<const float4*>(accumulationDevice), reinterpret_cast<float4*>(outputDevice), (uint32_t)pixelCount,
                              static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_resolve_device"); }

int hrpt_allgather(HrptContext* const* ranks, int n)
try {
    if (!ranks || n <= 0) return HRPT_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; ++i) if (!ranks[i]) return HRPT_ERR_INVALID_ARGUMENT;
    HrptContext* c0 = ranks[0];
    const uint32_t W = c0->width, H = c0->height;
    if (!c0->perSize.dAccum || W == 0 || H == 0) return fail(c0, HRPT_ERR_INVALID_ARGUMENT, "hrpt_allgather: hrpt_resize not called");
    if (H % (uint32_t)n != 0) return fail(c0, HRPT_ERR_INVALID_ARGUMENT, "hrpt_allgather: image height must be a multiple of the number of ranks");
    for (int i = 0; i < n; ++i) {
        if (ranks[i]->width != W || ranks[i]->height != H || !ranks[i]->perSize.dAccum) return fail(c0, HRPT_ERR_INVALID_ARGUMENT, "hrpt_allgather: contexts differ in image size");
        for (int j = 0; j < i; ++j) if (ranks[j] == ranks[i]) return fail(c0, HRPT_ERR_INVALID_ARGUMENT, "hrpt_allgather: the same context appears twice");
    }
    const size_t rows = H / (uint32_t)n, bandBytes = rows * (size_t)W * sizeof(float4);
    std::vector<hipEvent_t> sent((size_t)n, nullptr);
    auto cleanup = [&]() { for (hipEvent_t e : sent) if (e) (void)hipEventDestroy(e); };
    // every rank pushes its band to all the others on its own stream, then marks the point where its sends are enqueued
    for (int i = 0; i < n; ++i) {
        HrptContext* src = ranks[i];
        hipError_t e = hipSetDevice(src->device);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sent[(size_t)i], hipEventDisableTiming);
        const size_t off = (size_t)i * rows * W;
        for (int j = 0; j < n && e == hipSuccess; ++j) {
            if (j == i) continue;
            HrptContext* dst = ranks[j];
            // the destination band must not be in use by the destination's earlier work (e.g. its previous resolve): order behind it
            hipEvent_t ready = nullptr;
            e = hipSetDevice(dst->device);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ready, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventRecord(ready, dst->stream);
            if (e == hipSuccess) e = hipSetDevice(src->device);
            if (e == hipSuccess) e = hipStreamWaitEvent(src->stream, ready, 0);
            if (e == hipSuccess) e = hipMemcpyPeerAsync(dst->perSize.dAccum + off, dst->device, src->perSize.dAccum + off, src->device, bandBytes, src->stream);
            if (ready) (void)hipEventDestroy(ready);
        }
        if (e == hipSuccess) e = hipEventRecord(sent[(size_t)i], src->stream);
        if (e != hipSuccess) { cleanup(); return fail(c0, HRPT_ERR_HIP, std::string("hrpt_allgather (send): ") + hipGetErrorString(e)); }
    }
    // every rank waits for all senders, then resolves its now complete image
    for (int j = 0; j < n; ++j) {
        HrptContext* dst = ranks[j];
        hipError_t e = hipSetDevice(dst->device);
        for (int i = 0; i < n && e == hipSuccess; ++i) if (i != j) e = hipStreamWaitEvent(dst->stream, sent[(size_t)i], 0);
        if (e == hipSuccess) e = launch_resolve(dst->perSize.dAccum, dst->perSize.dOutput, W * H, dst->stream);
        if (e != hipSuccess) { cleanup(); return fail(c0, HRPT_ERR_HIP, std::string("hrpt_allgather (receive): ") + hipGetErrorString(e)); }
    }
    cleanup();      // destroying a recorded event is deferred by the runtime until the waits that reference it have run
    return HRPT_OK;
} catch (...) { return caught(ranks && n > 0 ? ranks[0] : nullptr, "hrpt_allgather"); }

int hrpt_trace_rays(HrptContext* c, const HrptRay* rays, HrptRayHit* hits, uint64_t count, uint32_t flags)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->haveScene) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_trace_rays: no scene uploaded");
    if (count == 0) return HRPT_OK;
    if (!rays || !hits) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_trace_rays: null array");
    if ((flags & 0xFFu) > HRPT_RAYS_SHADOW || (flags & ~(0xFFu | HRPT_RAYS_DEVICE_POINTERS | HRPT_RAYS_THREAD_PER_RAY))) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_trace_rays: unknown flags");
    if (count > (1ull << 31)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_trace_rays: too many rays in one call");
    if (c->view.instances && ((flags & HRPT_RAYS_THREAD_PER_RAY) || !wavefront_trace_rays_supported(c->traits)) && exceeds_private_stack(c->traits))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_trace_rays: this two-level structure is deeper than the thread-per-ray kernel's 64-entry stack");
    HIP_TRY(c, hipSetDevice(c->device));
    const bool shadow = (flags & 0xFFu) == HRPT_RAYS_SHADOW;
    // the persistent refilling traversal kernel (pt_wf_extend.h wf_trace_rays); the thread-per-ray kernel stays as the fallback for trees
    // deeper than its stacks allow and as the cross-check (HRPT_RAYS_THREAD_PER_RAY)
    const bool persistent = !(flags & HRPT_RAYS_THREAD_PER_RAY) && wavefront_trace_rays_supported(c->traits) && c->view.node4Count > 0;
    auto trace = [&](const HrptRay* dr, HrptRayHit* dh) -> hipError_t {
        if (!persistent) return launch_trace_rays(c->view, dr, dh, count, shadow, c->stream);
        std::string werr;
        hipError_t te = wavefront_trace_rays(c->wf, c->view, c->traits, dr, dh, count, shadow, c->stream, werr);
        if (te != hipSuccess) c->err = "hrpt_trace_rays: " + werr;
        return te;
    };
    if (flags & HRPT_RAYS_DEVICE_POINTERS) {
        HIP_TRY(c, trace(rays, hits));
        return HRPT_OK;
    }
    DeviceBuffer<HrptRay> dRays; DeviceBuffer<HrptRayHit> dHits;
    hipError_t e = dRays.alloc(count * sizeof(HrptRay));
    if (e == hipSuccess) e = dHits.alloc(count * sizeof(HrptRayHit));
    if (e == hipSuccess) e = hipMemcpyAsync(dRays, rays, count * sizeof(HrptRay), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = trace(dRays, dHits);
    if (e == hipSuccess) e = hipMemcpyAsync(hits, dHits, count * sizeof(HrptRayHit), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, hip_status(e), std::string("hrpt_trace_rays: ") + hipGetErrorString(e));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_trace_rays"); }

// Path-traced radiance along the caller's rays: the checks of hrpt_render that apply (bounces, lights), then the wavefront pipeline between
// wf_raygen_rays and wf_store_radiance, or one thread per ray. No events, no counters, no fallback count: HrptStats keeps describing renders.
int hrpt_trace_radiance(HrptContext* c, const HrptRay* rays, float* radiance4, uint64_t count, const HrptPathTracerConstants* constants, uint32_t flags)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, "hrpt_trace_radiance: no scene uploaded");
    if (!constants) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_trace_radiance: null constants");
    if (flags & ~(HRPT_RADIANCE_DEVICE_POINTERS | HRPT_RADIANCE_THREAD_PER_RAY | HRPT_RADIANCE_ACCUMULATE | HRPT_RADIANCE_SECONDARY)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_trace_radiance: unknown flags");
    if (constants->m_MaxBounces > 64u) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_trace_radiance: m_MaxBounces above 64 (one kernel sequence is launched per bounce)");
    if (constants->m_LightCount > c->view.lightCount) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_trace_radiance: m_LightCount exceeds the scene's light buffer");
    if (count == 0) return HRPT_OK;
    if (!rays || !radiance4) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_trace_radiance: null array");
    if (count > (1ull << 31)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_trace_radiance: too many rays in one call");
    const bool wavefront = !(flags & HRPT_RADIANCE_THREAD_PER_RAY) && wavefront_supports(c->view, *constants);
    if (!wavefront && c->view.instances && exceeds_private_stack(c->traits))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_trace_radiance: this two-level structure is deeper than the thread-per-ray kernel's 64-entry stack");
    HIP_TRY(c, hipSetDevice(c->device));
    const bool accumulate = (flags & HRPT_RADIANCE_ACCUMULATE) != 0, secondary = (flags & HRPT_RADIANCE_SECONDARY) != 0;
    auto trace = [&](const HrptRay* dr, float4* dl) -> hipError_t {
        if (!wavefront) return launch_radiance_rays(c->view, *constants, dr, dl, count, accumulate, secondary, c->stream);
        std::string werr;
        c->wf.shadeInstances = (uint32_t)c->keptInstances.size(); c->wf.shadeMaterials = (uint32_t)c->keptMaterials.size();    // as hrpt_render sets them
        hipError_t te = wavefront_radiance(c->wf, c->view, c->traits, *constants, dr, dl, count, accumulate, secondary, c->stream, werr);
        if (te != hipSuccess) c->err = "hrpt_trace_radiance: " + werr;
        return te;
    };
    if (flags & HRPT_RADIANCE_DEVICE_POINTERS) {
        HIP_TRY(c, trace(rays, reinterpret_cast<float4*>(radiance4)));
        return HRPT_OK;
    }
    DeviceBuffer<HrptRay> dRays; DeviceBuffer<float4> dRadiance;
    hipError_t e = dRays.alloc(count * sizeof(HrptRay));
    if (e == hipSuccess) e = dRadiance.alloc(count * sizeof(float4));
    if (e == hipSuccess) e = hipMemcpyAsync(dRays, rays, count * sizeof(HrptRay), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && accumulate) e = hipMemcpyAsync(dRadiance, radiance4, count * sizeof(float4), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = trace(dRays, dRadiance);
    if (e == hipSuccess) e = hipMemcpyAsync(radiance4, dRadiance, count * sizeof(float4), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, hip_status(e), std::string("hrpt_trace_radiance: ") + hipGetErrorString(e));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_trace_radiance"); }

int hrpt_resolve_columns_device(HrptContext* c, const float* shardsDevice, float* accumulationDevice, float* outputDevice, uint32_t width, uint32_t height, uint32_t ranks, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!shardsDevice || !outputDevice) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_resolve_columns_device: null image");
    if (ranks == 0 || width == 0 || height == 0 || width % (8u * ranks) != 0) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_resolve_columns_device: width must be a positive multiple of 8 * ranks");
    if ((uint64_t)width * height > 0xFFFFFFFFull) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_resolve_columns_device: image too large");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_resolve_columns(reinterpret_cast<const float4*>(shardsDevice), reinterpret_cast<float4*>(accumulationDevice), reinterpret_cast<float4*>(outputDevice),
                                      width, height, ranks, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_resolve_columns_device"); }
