// pt_wavefront.hip -- the production path: a persistent-threads wavefront path tracer for gfx950.
//
// One hrpt_render = all requested accumulation indices ("spp") of a tile at once:
//   wf_raygen -> per bounce { wf_extend -> wf_shade -> wf_shadow } -> wf_resolve
// replacing the single PathTracer_CSMain dispatch per index of the reference
// (/root/reference/src/shaders/PathTracer.hlsl:53-340, src/PathTracerRenderer.cpp:96-103).
//
// Data layout in HBM (one pool, SoA of float4, all streams coalesced 16 B/lane):
//   path queues A/B (ping-pong per bounce): rayO{o.xyz,tmin} rayD{d.xyz,rng} thr{T.xyz,sample} [med0{sigmaA,ior} med1{sigmaS,inVolume}]
//   hit records of the current queue:       hit{t,u,v,triangle}  (triangle = leaf-order index, 0xFFFFFFFF = miss)
//   NEE / shadow queue (dense):             sh0{origin,sample} sh1{N,roughness} sh2{V,metallic} sh3{baseColor,ior} sh4{T,count}
//                                           + per light sample shL{ux,uy,light}: direction, visibility and the BRDF x radiance
//                                           evaluation are done by wf_shadow, where every lane has NEE work and occluded
//                                           samples skip the evaluation
//   sampleRadiance[sample] (rgb): one slot per (pixel, accumulation index); emissive / NEE / sky are added in path order,
//                                 wf_resolve then folds the indices in order exactly like progressive accumulation (:332-339).
// Queues are SEGMENTED: a segment is 1024 consecutive samples owned by ONE wave at a time. The owning wave
// compacts survivors inside its segment with __ballot + popcount prefix (no global atomics, no block barriers,
// deterministic layout, pixel tiles stay together), and writes the segment's live count. Every kernel is a fixed
// grid of persistent waves striding over segments; each wave reaches its exit when the segment index runs out.
// The BVH (nodes + world-space triangles) is copied to LDS when it fits, and the traversal stack lives in LDS,
// one column per lane (conflict-free), sized from the builder's maximum depth.
#define HRPT_PHASE_TU 1
#include "pt_wavefront.h"

#include <mutex>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "bvh_build.h"
#include "pt_gbuffer.h"
#include "pt_motion.h"
#include "pt_path.h"

#ifdef HRPT_PHASE_PROFILE
__device__ unsigned long long g_phaseCounters[128];
#endif
#ifdef HRPT_SKY_DEBUG       // diagnostic build: what the miss branch of wf_shade fed into / got out of the sky lookup, first 2048 samples x 16 floats
__device__ float g_skyDebug[2048 * 16];
#endif

namespace hrt {

namespace {

#include "pt_wf_common.h"      // the device code, one piece per stage, in this order
#include "pt_wf_raygen.h"
#include "pt_wf_extend.h"
#include "pt_wf_shade.h"
#include "pt_wf_shadow.h"
#include "pt_wf_gbuffer.h"

// ------------------------------------------------------------------ host side
// What is launched, on which grid and with how much LDS is decided in pt_wavefront_plan.h; here the plan meets the kernels.
// The persistent kernels divide their segments evenly among the waves of the grid (seg = wave, wave + waves, ...), so a grid that is not a
// whole number of ROUNDS of what a CU holds of that kernel finishes late: with six resident blocks per CU a grid of 16 per CU takes three
// rounds of 1/16 of the work each, 12 takes two of 1/12 (measured: LDS-tree wf_extend +8 % at 16, global-tree wf_extend +20 % at 7 against 6).
// launch_rounds trims the requested grid to whole rounds of the kernel's own occupancy (hipOccupancyMaxActiveBlocksPerMultiprocessor: its
// registers, its LDS bytes), asked once per kernel and LDS size. Used for the closest-hit traversal kernels (wf_extend, wf_trace_rays), where
// the effect is large and consistent; the other kernels launch the grid asked for: trimmed, the any-hit pass of the glass config lost 12 %
// (one round of its five resident blocks instead of eight blocks per CU) and the buffered shadow kernel 3 %, the rest did not move.
static int resident_blocks_per_cu(const void* kernel, size_t ldsBytes)
{
    static std::mutex mu; static std::unordered_map<uint64_t, int> cache;
    const uint64_t key = (uint64_t)(uintptr_t)kernel * 0x9E3779B97F4A7C15ull ^ (uint64_t)ldsBytes;
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, (int)kBlock, ldsBytes) != hipSuccess) { (void)hipGetLastError(); n = 0; }
    cache.emplace(key, n);
    return n;
}
template <class K, class... Args> static void launch_rounds(uint32_t cus, K kernel, dim3 g, size_t ldsBytes, hipStream_t st, Args... args)
{
    const int resident = cus ? resident_blocks_per_cu(reinterpret_cast<const void*>(kernel), ldsBytes) : 0;
    const uint32_t perRound = cus * (uint32_t)(resident > 0 ? resident : 0);
    if (perRound && g.x > perRound) g.x = (g.x / perRound) * perRound;
    hipLaunchKernelGGL(kernel, g, dim3(kBlock), ldsBytes, st, args...);
}

// The template arguments <LDS_BVH, DEPTH, W, TL> of the traversal kernel a Variant stands for, as compile-time constants: calls
// f(bool_constant<L>, integral_constant<int, D>, integral_constant<int, W>, integral_constant<int, TL>) with one of
//   flat 2-wide tree       L in { false, true }   D in { 8, 16, 32, 64 }   W = 2                     TL = 0
//   flat 4-wide tree       L in { false, true }   D in { 16, 32, 64 }      W = 4                     TL = 0
//   ... quantised nodes    L = false              D in { 16, 32, 64 }      W = kQuantisedTree        TL = 0
//   two-level structure    L = false              D in { 16, 32, 64 }      W = 4                     TL = 1 (every instance opaque), 2
// and no other combination, so a kernel is instantiated only where f names it for one of these.
template <int N> using int_c = std::integral_constant<int, N>;
template <class F> void dispatch_variant(const Variant& v, F&& f)
{
    auto depth = [&](auto L, auto W, auto TL) {
        if constexpr (W() == 2) if (v.depth <= 8) return f(L, int_c<8>(), W, TL);
        if (v.depth <= 16) return f(L, int_c<16>(), W, TL);
        if (v.depth <= 32) return f(L, int_c<32>(), W, TL);
        return f(L, int_c<64>(), W, TL);
    };
    if (v.twoLevel) { if (v.twoLevelCandidates) depth(std::false_type(), int_c<4>(), int_c<2>()); else depth(std::false_type(), int_c<4>(), int_c<1>()); }
    else if (v.width == 2) { if (v.lds) depth(std::true_type(), int_c<2>(), int_c<0>()); else depth(std::false_type(), int_c<2>(), int_c<0>()); }
    else if (v.lds) depth(std::true_type(), int_c<4>(), int_c<0>());
    else if (v.quantised) depth(std::false_type(), int_c<kQuantisedTree>(), int_c<0>());
    else depth(std::false_type(), int_c<4>(), int_c<0>());
}

// wf_extend: closest hits (trimmed to whole rounds) or, anyHit, the visibility pass of the resolve schedule over the shadow-ray queue
void launch_extend(const Variant& v, uint32_t cus, dim3 g, hipStream_t st, const WfArgs& a, uint32_t parity, bool anyHit = false)
{
    dispatch_variant(v, [&](auto L, auto D, auto W, auto TL) {
        constexpr bool l = L(); constexpr int d = D(), w = W(), tl = TL();
        auto closest = [&](auto kernel) { launch_rounds(cus, kernel, g, v.ldsBytes, st, a, parity); };
        if constexpr (tl != 0) {       // closest hits only (plan_render keeps the any-hit pass off for two-level scenes)
            if (a.primary) closest(wf_extend<false, d, 4, false, tl, true>);
            else closest(wf_extend<false, d, 4, false, tl, false>);
        } else if (anyHit) hipLaunchKernelGGL((wf_extend<l, d, w, true>), g, dim3(kBlock), v.ldsBytes + kCandidateLdsBytes, st, a, parity);
        else if constexpr (w == 2) closest(wf_extend<l, d, w, false>);
        else if (a.primary) { if (a.allOpaque) closest(wf_extend<l, d, w, false, 0, true, true>); else closest(wf_extend<l, d, w, false, 0, true>); }
        else { if (a.allOpaque) closest(wf_extend<l, d, w, false, 0, false, true>); else closest(wf_extend<l, d, w, false>); }
    });
}
// wf_shadow in one of the kShadow* modes; two-level scenes: kShadowOpaque or kShadowSlim, candidates by Variant::twoLevelCandidates
void launch_shadow(const Variant& v, dim3 g, hipStream_t st, const WfArgs& a, const HrptPathTracerConstants& cb, int bounce, bool dirOnly, int mode)
{
    dispatch_variant(v, [&](auto L, auto D, auto W, auto TL) {
        constexpr bool l = L(); constexpr int d = D(), w = W(), tl = TL();
        auto launch = [&](auto kernel, size_t extraLds) { hipLaunchKernelGGL(kernel, g, dim3(kBlock), v.ldsBytes + extraLds, st, a, cb, bounce); };
        if constexpr (tl != 0) {
            const size_t cand = tl == 2 ? (size_t)kTwoLevelCandidates * 3 * kBlock * 4 : 0;      // candidate columns of the buffered two-level shadow query
            if (mode == kShadowSlim) launch(wf_shadow<false, d, 4, true, kShadowSlim, tl>, cand);
            else if (dirOnly) launch(wf_shadow<false, d, 4, true, kShadowOpaque, tl>, cand);
            else launch(wf_shadow<false, d, 4, false, kShadowOpaque, tl>, cand);
        } else if (mode == kShadowResolve) launch(wf_shadow<l, d, w, false, kShadowResolve>, 0);
        // general variant (all light types) + candidate buffer
        // (not trimmed to whole rounds: measured, the buffered variant -- three resident blocks per CU, long uneven entries -- is 3 % slower
        // with 15 or 6 blocks per CU than with the 16 or 8 asked for)
        else if (mode == kShadowBuffered) launch(wf_shadow<l, d, w, false, kShadowBuffered>, kCandidateLdsBytes);
        else if (mode == kShadowSlim) launch(wf_shadow<l, d, w, true, kShadowSlim>, 0);
        else if (dirOnly) launch(wf_shadow<l, d, w, true, kShadowOpaque>, 0);
        else launch(wf_shadow<l, d, w, false, kShadowOpaque>, 0);
    });
}
// wf_trace_rays: visibility (shadow) or closest hits over a caller's rays
void launch_wf_trace_rays(const Variant& v, uint32_t cus, dim3 g, hipStream_t st, const WfTraceArgs& a, bool shadow)
{
    dispatch_variant(v, [&](auto L, auto D, auto W, auto TL) {
        constexpr bool l = L(), tl = TL() != 0; constexpr int d = D(), w = W();
        if constexpr (w != 2) {        // (4-wide trees only: plan_trace_rays)
            // (two-level: no candidate columns: visibility queries over non-opaque instances re-trace behind every candidate)
            if (shadow) launch_rounds(cus, wf_trace_rays<l, d, w, true, tl>, g, v.ldsBytes + (tl ? 0 : kCandidateLdsBytes), st, a);
            else launch_rounds(cus, wf_trace_rays<l, d, w, false, tl>, g, v.ldsBytes, st, a);
        }
    });
}
// NEE visibility + accumulation of one bounce on stream `sst`. With non-opaque geometry in the scene: ray generation, the opaque any-hit pass in
// the refilling traversal kernel, then wf_shadow for the contributions and the (few) rays that crossed non-opaque triangles.
void shadow_stage(const RenderPlan& plan, const SceneTraits& traits, uint32_t cus, dim3 grid, hipStream_t sst, WfArgs& a, const HrptPathTracerConstants& cb, int bounce, uint32_t parity)
{
    a.shadowParity = parity;
    if (plan.shadowMode == kShadowResolve) {
        if (traits.directionalLightsOnly) hipLaunchKernelGGL((wf_shadow_rays<true>), grid, dim3(kBlock), 0, sst, a, cb);
        else hipLaunchKernelGGL((wf_shadow_rays<false>), grid, dim3(kBlock), 0, sst, a, cb);
        launch_extend(plan.vA, cus, grid, sst, a, 0u, true);
    }
    launch_shadow(plan.vS, grid, sst, a, cb, bounce, traits.directionalLightsOnly, plan.shadowMode);
}
// The shading of one bounce: wf_bounce0 (fusedBounce0: trace + shade of bounce 0, by the depth of vE) or the wf_shade / wf_shade_lt the plan and a.primary name
void launch_shade(const RenderPlan& plan, bool fusedBounce0, dim3 g, hipStream_t st, const WfArgs& a, const HrptPathTracerConstants& cb, uint32_t parity, int bounce, int last)
{
    const size_t sortLds = (size_t)(kBlock / 64) * ((size_t)5 * a.segSize);      // per wave: two uint16 permutations (segments A, B) + uint8 class keys
    auto bounce0 = [&](auto kernel) { hipLaunchKernelGGL(kernel, g, dim3(kBlock), plan.bounce0LdsBytes, st, a, cb, last); };
    auto shade = [&](auto kernel, size_t ldsBytes) { hipLaunchKernelGGL(kernel, g, dim3(kBlock), ldsBytes, st, a, cb, parity, bounce, last); };
    if (fusedBounce0) {
        if (plan.vE.depth <= 16) bounce0(wf_bounce0<16>);
        else if (plan.vE.depth <= 32) bounce0(wf_bounce0<32>);
        else bounce0(wf_bounce0<64>);
    }
    else if (plan.maxLights > kMaxLights) shade(wf_shade<0, false>, sortLds);
    else if (plan.maxLights > 1) shade(wf_shade<(int)kMaxLights, false>, sortLds);
    else if (plan.simpleScene && plan.shadeLdsTables && a.primary) shade(wf_shade_lt<1, true, true>, plan.shadeLdsBytes);
    else if (plan.simpleScene && plan.shadeLdsTables) shade(wf_shade_lt<1, true>, plan.shadeLdsBytes);
    else if (plan.simpleScene && a.primary) shade(wf_shade<1, true, true>, plan.shadeLdsBytes);
    else if (plan.simpleScene) shade(wf_shade<1, true>, plan.shadeLdsBytes);
    else shade(wf_shade<1, false>, sortLds);
}

TreeCounts tree_counts(const SceneView& scene) { return { scene.nodeCount, scene.node4Count, scene.triCount, scene.nodesQ != nullptr, scene.instances != nullptr, 0u, 0u }; }

// CUs of the context's device, asked once per context (a context stays on the device it was created for)
hipError_t device_cus(WavefrontState& st, uint32_t& cus, std::string& error)
{
    if (!st.cus) {
        hipError_t e; int dev = 0; hipDeviceProp_t prop;
        if ((e = hipGetDevice(&dev)) != hipSuccess || (e = hipGetDeviceProperties(&prop, dev)) != hipSuccess) { error = "hipGetDeviceProperties"; return e; }
        st.cus = (uint32_t)prop.multiProcessorCount;
    }
    cus = st.cus;
    return hipSuccess;
}

// Grows `buf` to at least `bytes`. Work in flight on the context's streams may still use the old allocation, so both are waited for before
// it goes. After a failure the buffer is empty.
hipError_t grow_buffer(WavefrontState& st, hipStream_t stream, DeviceBuffer<void>& buf, size_t bytes)
{
    if (bytes <= buf.bytes()) return hipSuccess;
    if (buf) { (void)hipStreamSynchronize(stream); if (st.auxStream) (void)hipStreamSynchronize(st.auxStream); }
    return buf.alloc(bytes);
}
// The traversal-stack overflow columns of a render or G-buffer plan: two sets (wf_extend and wf_shadow run concurrently) of `entries` ints
// each (threads x entries per thread; 0 = the tree fits the LDS stack). A G-buffer call sizes them as a render does: the next render keeps the buffer.
hipError_t reserve_spill(WavefrontState& st, hipStream_t stream, size_t entries, WfArgs& a, std::string& error)
{
    if (!entries) return hipSuccess;
    const hipError_t e = grow_buffer(st, stream, st.spill, 2 * entries * 4);
    if (e != hipSuccess) { error = "hipMalloc(traversal stack overflow)"; return e; }
    a.spill[0] = static_cast<int32_t*>(st.spill.get()); a.spill[1] = a.spill[0] + entries;
    return hipSuccess;
}

} // namespace

hipError_t wavefront_trace_rays(WavefrontState& st, const SceneView& scene, const SceneTraits& traits, const HrptRay* rays, HrptRayHit* hits, uint64_t count,
                                bool shadow, hipStream_t stream, std::string& error)
{
    if (count == 0) return hipSuccess;
    hipError_t e; uint32_t cus = 0;
    if ((e = device_cus(st, cus, error)) != hipSuccess) return e;
    const TraceRaysPlan p = plan_trace_rays(traits, tree_counts(scene), count, shadow, cus, st.knobs);
    WfTraceArgs a{};
    a.scene = scene; a.rays = rays; a.hits = hits; a.count = count;
    a.refillMin = p.refillMin; a.nodeLoopMin = p.nodeLoopMin; a.quantised = p.v.quantised;
    if (p.spillEntries) {
        // own overflow columns (a render may be in flight on the context's buffers only in stream order, but sizes differ)
        if ((e = grow_buffer(st, stream, st.traceSpill, p.spillThreads * p.spillEntries * 4)) != hipSuccess) { error = "hipMalloc(traversal stack overflow)"; return e; }
        a.spill = static_cast<int32_t*>(st.traceSpill.get());
    }
    launch_wf_trace_rays(p.v, cus, dim3(p.grid), stream, a, shadow);
    if ((e = hipGetLastError()) != hipSuccess) { error = "kernel launch"; return e; }
    return hipSuccess;
}

bool wavefront_supports(const SceneView& scene, const HrptPathTracerConstants& cb)
{
    (void)scene;
    return cb.m_MaxBounces >= 1;       // any number of lights: up to kMaxLights buffered per lane, beyond that streamed (wf_shade<0>)
}

void wavefront_release(WavefrontState& st)
{
    st.pool.reset(); st.spill.reset(); st.traceSpill.reset(); st.gbPool.reset(); st.radPool.reset();
    for (auto* events : { &st.events, &st.forkEvents, &st.joinEvents }) { for (hipEvent_t e : *events) (void)hipEventDestroy(e); events->clear(); }
    st.eventsUsed = 0;
    if (st.auxStream) (void)hipStreamDestroy(st.auxStream);
    st.auxStream = nullptr;
}

void wavefront_collect_timing(WavefrontState& st)
{
    for (uint32_t i = 0; i + 1 < st.eventsUsed; i += 2) {
        float t = 0.0f;
        if (hipEventElapsedTime(&t, st.events[i], st.events[i + 1]) == hipSuccess) { st.kernelMs[st.kind[i / 2]] += t; st.kernelLaunches[st.kind[i / 2]]++; }
    }
    st.eventsUsed = 0;
}

#ifdef HRPT_SKY_DEBUG
extern "C" int hrpt_sky_debug_read(float* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_skyDebug), sizeof(float) * 2048 * 16) == hipSuccess ? 0 : -3; }
#endif
#ifdef HRPT_PHASE_PROFILE
// reads (and zeroes) the phase counters of this library build
extern "C" int hrpt_phase_profile_read(unsigned long long* out128)
{
    if (hipMemcpyFromSymbol(out128, HIP_SYMBOL(g_phaseCounters), 128 * sizeof(unsigned long long)) != hipSuccess) return -3;
    static const unsigned long long zero[128] = { 0 };
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_phaseCounters), zero, sizeof zero) != hipSuccess) return -3;
    return 0;
}
#endif

void wavefront_reset_timing(WavefrontState& st)
{
    st.eventsUsed = 0;
    for (int k = 0; k < kKernelClasses; ++k) { st.kernelMs[k] = 0.0f; st.kernelLaunches[k] = 0; }
    st.raygenBytes = 0; st.resolveBytes = 0;
}

// Record sizes (the SoA streams of WfBuffers, 16 B per float4 stream):
//   path record   rayO + rayD + thr (+ med0 + med1)              48 (80) B       hit record  16 B
//   shadow entry  sh0 + sh1 + sh4 always read, sh2 + sh3 only for an entry with an unoccluded sample; + shL 16 B per light sample
//   radiance      one float4 read-modify-write                    32 B
// Any-hit schedule (kShadowResolve): per shadow ray sqO + sqD + sqId written and read (2 x 36 B), shVis written and read per light slot.
void wavefront_queue_bytes(const WavefrontState& st, const DeviceCounters& c, uint64_t& trace, uint64_t& shade, uint64_t& shadow)
{
    const uint64_t path = st.plan.pathRecordBytes, survivors = c.closestRays > c.paths ? c.closestRays - c.paths : 0;
    trace = c.closestRays * (32 + 16);
    shade = c.closestRays * (path + 16) + survivors * path + c.neeEntries * 80 + c.neeSamples * 16 + c.radianceShade * 32;
    shadow = c.neeEntries * 48 + c.neeSamples * 16 + c.radianceShadow * (32 + 32);
    if (st.plan.shadowMode == kShadowSlim) {     // 32-byte entries; wf_shadow re-reads rayD (always) and thr (unoccluded samples) of the path's input record
        shade = c.closestRays * (path + 16) + survivors * path + c.neeEntries * 32 + c.radianceShade * 32;
        shadow = c.neeEntries * (32 + 16) + c.radianceShadow * (16 + 32);
    }
    if (st.plan.shadowMode == kShadowResolve) shadow += c.neeEntries * 32 + c.neeSamples * 16 + c.shadowRays * 72 + c.neeEntries * st.plan.maxLights * 8;
    if (st.plan.fusedPrimary) {      // bounce 0 reads no path records: wf_extend only writes hits, wf_shade reads them and stores the first radiance term
        trace -= c.paths * 16;                               // no record read, {direction, seed} written
        shade = shade - c.paths * (path - 16) + c.paths * 16;     // 16 of the 48 record bytes read; first radiance term stored
        shadow -= c.skipped16 * 16;
        // wf_bounce0: neither record is written by the trace or read by the shading; a {direction, seed} record is stored per shadow-queue entry
        trace -= c.fusedPaths * 32;
        shade = shade - c.fusedPaths * 32 + c.fusedEntries * 16;
    }
}

namespace {
// records an event; pairs are (begin, end) around one launch of kernel class `kind`
bool timing_mark(WavefrontState& st, hipStream_t stream, KernelClass kind, bool begin)
{
    if (st.eventsUsed >= 4096) return true;   // a single render never needs more; stop timing rather than grow unbounded
    if (st.eventsUsed + 1 > st.events.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return false;
        st.events.push_back(e);
    }
    if (begin) { if (st.kind.size() < st.eventsUsed / 2 + 1) st.kind.resize(st.eventsUsed / 2 + 1); st.kind[st.eventsUsed / 2] = (uint8_t)kind; }
    (void)hipEventRecord(st.events[st.eventsUsed], stream);
    st.eventsUsed++;
    return true;
}
// Lays the streams of a queue pool down: each at a 256-byte aligned offset from `base`, in call order; a stream the scene does not have
// (present = false) points at the base and takes no room. Run against a null base for the size (`off`), then against the allocation.
struct PoolCarver {
    char* base; size_t off = 0;
    template <class T> void operator()(T*& stream, size_t bytes, bool present = true)
    {
        stream = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + (present ? off : 0));
        if (present) off += (bytes + 255) & ~(size_t)255;
    }
};
size_t counter_bytes(uint64_t capacity) { return (size_t)(capacity / 64) * 4; }      // one count per segment, sized for the smallest segment (64 samples)
// What every pool starts with: the first `queues` path queues, the hit records and, on two-level scenes, the hit's instance (else hitInst: null)
void carve_paths_and_hits(PoolCarver& carve, WfBuffers& b, int queues, uint64_t capacity, bool hasMedium, bool hasInstances)
{
    for (int p = 0; p < queues; ++p) {
        carve(b.rayO[p], capacity * 16); carve(b.rayD[p], capacity * 16); carve(b.thr[p], capacity * 16);
        carve(b.med0[p], capacity * 16, hasMedium); carve(b.med1[p], capacity * 16, hasMedium);
        carve(b.pathCnt[p], counter_bytes(capacity));
    }
    carve(b.hit, capacity * 16);
    carve(b.hitInst, capacity * 4, hasInstances); if (!hasInstances) b.hitInst = nullptr;
}
// Queue pool of a render: every stream of WfBuffers (and the PrimaryArgs copy), in this order; returns the bytes used.
size_t carve_pool(char* base, WfArgs& a, uint64_t capacity, uint32_t maxLights, const SceneTraits& traits, bool hasInstances)
{
    const bool hasShadowRayQueue = traits.hasNonOpaque || maxLights > 1;
    PoolCarver carve{ base };
    WfBuffers& b = a.b;
    carve_paths_and_hits(carve, b, 2, capacity, traits.hasMedium, hasInstances);
    carve(a.primaryArgs, sizeof(PrimaryArgs));
    carve(b.sh0, capacity * 16); carve(b.sh1, capacity * 16); carve(b.sh2, capacity * 16); carve(b.sh3, capacity * 16); carve(b.sh4, capacity * 16);
    carve(b.shL, capacity * 16 * maxLights);
    carve(b.shadowCnt, counter_bytes(capacity)); carve(b.radiance, capacity * 16);
    // (the shadow mode is the plan's; the arrays are small next to the path queues)
    carve(b.sqO, capacity * 16 * maxLights, hasShadowRayQueue); carve(b.sqD, capacity * 16 * maxLights, hasShadowRayQueue); carve(b.sqId, capacity * 4 * maxLights, hasShadowRayQueue);
    carve(b.sqCnt, counter_bytes(capacity), hasShadowRayQueue); carve(b.shVis, capacity * 4 * maxLights, hasShadowRayQueue); carve(b.sqCand, capacity * 8 * kShadowCandidates * maxLights, hasShadowRayQueue);
    return carve.off;
}
// Queue pool of a G-buffer call: path queue 0, hit records, the radiance slots wf_raygen zeroes and a scratch counter block (the front end counts
// rays and paths; HrptStats describes renders, so these counts go nowhere).
size_t carve_gbuffer_pool(char* base, WfArgs& a, uint64_t capacity, bool hasMedium, bool hasInstances)
{
    PoolCarver carve{ base };
    carve_paths_and_hits(carve, a.b, 1, capacity, hasMedium, hasInstances);
    carve(a.b.radiance, capacity * 16);
    carve(a.counters, sizeof(DeviceCounters) * kCounterShards);
    return carve.off;
}
// The part of WfArgs that scene, traits, rectangle and knobs decide; what a plan decides is the caller's (everything else stays zero)
void fill_scene_args(WfArgs& a, const WavefrontState& st, const SceneView& scene, const SceneTraits& traits, TileRect rect, uint32_t width)
{
    a.scene = scene;
    a.tilesX = rect.columns(); a.tilesY = (rect.y1 - rect.y0 + 7) / 8; a.rect = rect; a.imageWidth = width; a.pixelsPadded = a.tilesX * a.tilesY * 64;
    a.hasMedium = traits.hasMedium ? 1u : 0u; a.hasStochasticAlpha = traits.hasStochasticAlpha ? 1u : 0u; a.allOpaque = traits.hasNonOpaque ? 0u : 1u;
    a.refillMin = st.knobs.refillMin ? st.knobs.refillMin : kRefillMinDefault; a.streamSegments = st.knobs.drainSegments ? 0u : 1u;
}
// Step 1 of a render: the accumulation indices per batch, so that one batch stays below maxSamples AND its queue pool below a byte budget,
// and the queue pool of such a batch (again with half the indices per batch when the device refuses the allocation), carved into `a`.
hipError_t size_batch_and_pool(WavefrontState& st, const RenderPlan& plan, const SceneTraits& traits, bool hasInstances, uint64_t pixelsPadded, uint32_t accumCount,
                               hipStream_t stream, WfArgs& a, uint32_t& sppPerBatch, std::string& error)
{
    sppPerBatch = accumCount < kMaxSppPerBatch ? accumCount : kMaxSppPerBatch;
    uint64_t maxSamples = 64ull << 20;
    if (pixelsPadded * sppPerBatch * plan.bytesPerSample > st.pool.bytes()) {
        // the pool has to grow: keep it within half of what the device has free (other contexts -- a second frame in flight -- need theirs)
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) == hipSuccess) {
            const uint64_t budget = (uint64_t)(freeB + st.pool.bytes()) / 2;
            if (budget / plan.bytesPerSample < maxSamples) maxSamples = budget / plan.bytesPerSample;
        }
    }
    if (maxSamples * plan.maxLights > 0xFFFFFFFFull) maxSamples = 0xFFFFFFFFull / plan.maxLights;      // (entry, light) slot ids are 32-bit
    while (sppPerBatch > 1 && pixelsPadded * sppPerBatch > maxSamples) --sppPerBatch;
    for (;;) {
        const uint64_t capacity = ((pixelsPadded * sppPerBatch + kMaxSegment - 1) / kMaxSegment) * kMaxSegment;
        if (capacity >= (1ull << 31)) { error = "tile too large for one batch"; return hipErrorInvalidValue; }
        const size_t bytes = carve_pool(nullptr, a, capacity, plan.maxLights, traits, hasInstances);
        const hipError_t e = grow_buffer(st, stream, st.pool, bytes);
        if (e == hipSuccess) { carve_pool(static_cast<char*>(st.pool.get()), a, capacity, plan.maxLights, traits, hasInstances); return hipSuccess; }
        (void)hipGetLastError();
        if (sppPerBatch == 1) {       // nothing left to halve
            error = "hipMalloc(queue pool, " + std::to_string(bytes >> 20) + " MiB for " + std::to_string(capacity) + " samples; render a smaller tile)";
            return e;
        }
        sppPerBatch = (sppPerBatch + 1) / 2;
    }
}
// The second stream and one fork and one join event per bounce, made at first use. false: the runtime refused one; this render runs serially
bool prepare_overlap(WavefrontState& st, int maxBounces)
{
    if (!st.auxStream && hipStreamCreateWithFlags(&st.auxStream, hipStreamNonBlocking) != hipSuccess) { st.auxStream = nullptr; return false; }
    while (st.forkEvents.size() < (size_t)maxBounces) {
        hipEvent_t f, j;
        if (hipEventCreateWithFlags(&f, hipEventDisableTiming) != hipSuccess) return false;
        if (hipEventCreateWithFlags(&j, hipEventDisableTiming) != hipSuccess) { (void)hipEventDestroy(f); return false; }
        st.forkEvents.push_back(f); st.joinEvents.push_back(j);
    }
    return true;
}
// The bounces of one batch whose path queue 0 is filled (or, plan.fusedPrimary, derived by the bounce-0 kernels): per bounce wf_extend, wf_shade and the
// shadow stage, for renders and hrpt_trace_radiance alike. `profile`: HIP events around every launch (renders with HRPT_FRAME_PROFILE).
// `firstBounce`: the path segment the queue holds (0, or 1 with HRPT_RADIANCE_SECONDARY). The kernels take the true bounce index; the queue and
// shadow parities and the fork / join events follow bounce - firstBounce, so path queue 0 is the input of the first bounce that runs.
hipError_t run_bounces(WavefrontState& st, const RenderPlan& plan, const SceneTraits& traits, uint32_t cus, const BatchPlan& batch, hipStream_t stream,
                       WfArgs& a, const HrptPathTracerConstants& cb, bool profile, std::string& error, int firstBounce = 0)
{
    hipError_t e;
    const dim3 grid(batch.grid);
    const int maxBounces = (int)cb.m_MaxBounces;
    // wf_shadow(b) only reads the shadow queue of shade(b) and adds into sampleRadiance; wf_extend(b+1) reads the path queue and
    // writes hit records: no shared buffer, so the two run concurrently (fork after shade(b), join before shade(b+1), which both
    // rewrites the shadow queue and adds the next radiance term -- the per-sample order of additions is unchanged).
    // Per-launch timing (HRPT_FRAME_PROFILE) needs stream order, so profiling renders serially.
    const bool overlap = !profile && !st.knobs.serialShadow && maxBounces - firstBounce > 1 && prepare_overlap(st, maxBounces - firstBounce);
    bool pendingJoin = false;
    for (int bounce = firstBounce; bounce < maxBounces; ++bounce) {
        const size_t step = (size_t)(bounce - firstBounce);
        const uint32_t parity = (uint32_t)step & 1u;
        const bool timed = profile && st.eventsUsed + 8 <= 4096;
        a.primary = (plan.fusedPrimary && bounce == 0) ? 1u : 0u;
        const bool fusedBounce0 = plan.fusedBounce0 && bounce == 0;      // wf_bounce0 in place of the pair below, on the shade grid, timed as wf_shade
        if (timed && !fusedBounce0) timing_mark(st, stream, kKernelExtend, true);
        if (!fusedBounce0) launch_extend(plan.vE, cus, dim3(batch.gridExtend), stream, a, parity);
        if (timed) { if (!fusedBounce0) timing_mark(st, stream, kKernelExtend, false); timing_mark(st, stream, kKernelShade, true); }
        if (pendingJoin) { if ((e = hipStreamWaitEvent(stream, st.joinEvents[step - 1], 0)) != hipSuccess) { error = "hipStreamWaitEvent(join)"; return e; } pendingJoin = false; }
        launch_shade(plan, fusedBounce0, grid, stream, a, cb, parity, bounce, bounce + 1 == maxBounces ? 1 : 0);
        if (timed) { timing_mark(st, stream, kKernelShade, false); timing_mark(st, stream, kKernelShadow, true); }
        if (overlap) {
            if ((e = hipEventRecord(st.forkEvents[step], stream)) != hipSuccess ||
                (e = hipStreamWaitEvent(st.auxStream, st.forkEvents[step], 0)) != hipSuccess) { error = "fork to the shadow stream"; return e; }
            shadow_stage(plan, traits, cus, grid, st.auxStream, a, cb, bounce, parity);
            if ((e = hipEventRecord(st.joinEvents[step], st.auxStream)) != hipSuccess) { error = "hipEventRecord(join)"; return e; }
            pendingJoin = true;
        } else {
            shadow_stage(plan, traits, cus, grid, stream, a, cb, bounce, parity);
        }
        if (timed) timing_mark(st, stream, kKernelShadow, false);
    }
    if (pendingJoin && (e = hipStreamWaitEvent(stream, st.joinEvents[(size_t)(maxBounces - firstBounce) - 1], 0)) != hipSuccess) { error = "hipStreamWaitEvent(join)"; return e; }
    return hipSuccess;
}
}

hipError_t wavefront_render(WavefrontState& st, const SceneView& scene, const SceneTraits& traits, const HrptPathTracerConstants& constants,
                            uint32_t accumCount, float4* accumulation, float4* output, uint32_t width, uint32_t height, TileRect rect,
                            DeviceCounters* counters, hipStream_t stream, std::string& error)
{
    (void)height;
    if (rect.x1 <= rect.x0 || rect.y1 <= rect.y0 || rect.columns() == 0) return hipSuccess;
    hipError_t e; uint32_t cus = 0;
    if ((e = device_cus(st, cus, error)) != hipSuccess) return e;
    TreeCounts tree = tree_counts(scene);
    tree.instanceCount = st.shadeInstances; tree.materialCount = st.shadeMaterials;
    const RenderPlan& plan = st.plan = plan_render(traits, tree, constants.m_LightCount, cus, st.knobs);
    // ---- 1. the batch size, the queue pool and the overflow columns
    WfArgs a{};
    fill_scene_args(a, st, scene, traits, rect, width);
    const uint64_t pixelsPadded = (uint64_t)a.tilesX * a.tilesY * 64;
    uint32_t sppPerBatch = 0;
    if ((e = size_batch_and_pool(st, plan, traits, scene.instances != nullptr, pixelsPadded, accumCount, stream, a, sppPerBatch, error)) != hipSuccess) return e;
    if ((e = reserve_spill(st, stream, plan.spillThreads * plan.spillEntries, a, error)) != hipSuccess) return e;
    // ---- 2. the arguments the plan decides
    a.maxLights = plan.maxLights; a.sortShade = plan.sortShade; a.nodeLoopMin = plan.nodeLoopMin; a.slimShadow = plan.slim ? 1u : 0u; a.counters = counters;
    a.shadeInstances = tree.instanceCount; a.shadeMaterials = tree.materialCount;       // the counts the plan sized the LDS tables from
    // ---- 3. per batch: raygen, the bounces (wf_shadow of one overlapping wf_extend of the next), resolve
    for (uint32_t first = 0; first < accumCount; first += sppPerBatch) {
        const uint32_t spp = (accumCount - first) < sppPerBatch ? (accumCount - first) : sppPerBatch;
        a.spp = spp; a.numSamples = (uint32_t)(pixelsPadded * spp);
        const BatchPlan batch = plan_batch(plan, st.knobs, a.numSamples);
        a.segSize = batch.segSize; a.numSegments = batch.numSegments;
        const dim3 grid(batch.grid);

        HrptPathTracerConstants cb = constants;
        cb.m_AccumulationIndex = constants.m_AccumulationIndex + first;
        JitterTable jt;
        for (uint32_t k = 0; k < spp; ++k) {   // PathTracerRenderer.cpp:65
            jt.j[k].x = hrpt_halton(cb.m_AccumulationIndex + k + 1, 2) - 0.5f;
            jt.j[k].y = hrpt_halton(cb.m_AccumulationIndex + k + 1, 3) - 0.5f;
        }
        PrimaryArgs pr{};
        if (plan.fusedPrimary) {
            for (int i = 0; i < 16; ++i) pr.clipToWorld[i] = cb.m_View.m_MatClipToWorldNoOffset[i];
            for (int i = 0; i < 3; ++i) pr.cam[i] = cb.m_CameraPos[i];
            pr.invW = cb.m_View.m_ViewportSizeInv[0]; pr.invH = cb.m_View.m_ViewportSizeInv[1]; pr.accumIndex = cb.m_AccumulationIndex;
            for (uint32_t k = 0; k < spp; ++k) pr.j[k] = jt.j[k];
            hipLaunchKernelGGL(wf_store_primary, dim3(1), dim3(64), 0, stream, pr, const_cast<PrimaryArgs*>(a.primaryArgs));
        }
        const bool timedEnds = st.profile && st.eventsUsed + 4 <= 4096;
        if (!plan.fusedPrimary) {
            if (timedEnds) timing_mark(st, stream, kKernelRaygen, true);
            hipLaunchKernelGGL(wf_raygen, grid, dim3(kBlock), 0, stream, a, cb, jt);
            if (timedEnds) timing_mark(st, stream, kKernelRaygen, false);
        }
        {   // raygen: sampleRadiance zeroed + one path record per pixel of the rectangle and index; resolve: sampleRadiance read, Accumulation
            // read (when resuming) and written, Output written
            const uint64_t w = (uint64_t)rect.columns() * 8u, px = (w < rect.x1 - rect.x0 ? w : (uint64_t)rect.x1 - rect.x0) * (rect.y1 - rect.y0);
            if (!plan.fusedPrimary) st.raygenBytes += (uint64_t)a.numSamples * 16 + px * spp * st.plan.pathRecordBytes;
            st.resolveBytes += px * ((uint64_t)spp * 16 + 32 + (cb.m_AccumulationIndex > 0 ? 16 : 0));
        }
        if ((e = run_bounces(st, plan, traits, cus, batch, stream, a, cb, st.profile, error)) != hipSuccess) return e;
        uint32_t rgrid = (uint32_t)((pixelsPadded + kBlock - 1) / kBlock); if (rgrid > cus * 8) rgrid = cus * 8;
        if (timedEnds) timing_mark(st, stream, kKernelResolve, true);
        hipLaunchKernelGGL(wf_resolve, dim3(rgrid), dim3(kBlock), 0, stream, a, accumulation, output, cb.m_AccumulationIndex);
        if (timedEnds) timing_mark(st, stream, kKernelResolve, false);
        if ((e = hipGetLastError()) != hipSuccess) { error = "kernel launch"; return e; }
    }
    return hipSuccess;
}

// hrpt_render_gbuffer, wavefront path: wf_raygen + the render's closest-hit kernel over one sample per pixel of `rect` (plan_gbuffer), then
// wf_gbuffer -- or, for hrpt_render_motion_vectors (`motion` given), wf_gbuffer_motion. Touches neither st.plan nor the byte / timing accounting of renders; works in the render's queue pool when that is large enough,
// otherwise in a pool of its own (HrptStats::queuePoolBytes keeps describing renders).
hipError_t wavefront_gbuffer(WavefrontState& st, const SceneView& scene, const SceneTraits& traits, const HrptPathTracerConstants& constants,
                             float4* const* planes, uint32_t planeMask, uint32_t width, TileRect rect, hipStream_t stream, std::string& error, const MotionArgs* motion)
{
    if (rect.x1 <= rect.x0 || rect.y1 <= rect.y0 || rect.columns() == 0) return hipSuccess;
    hipError_t e; uint32_t cus = 0;
    if ((e = device_cus(st, cus, error)) != hipSuccess) return e;
    WfArgs a{};
    fill_scene_args(a, st, scene, traits, rect, width);
    const uint64_t pixelsPadded = (uint64_t)a.tilesX * a.tilesY * 64;
    const uint64_t capacity = ((pixelsPadded + kMaxSegment - 1) / kMaxSegment) * kMaxSegment;
    if (capacity >= (1ull << 31)) { error = "tile too large for one batch"; return hipErrorInvalidValue; }
    const GBufferPlan plan = plan_gbuffer(traits, tree_counts(scene), cus, st.knobs, (uint32_t)pixelsPadded);
    const size_t bytes = carve_gbuffer_pool(nullptr, a, capacity, traits.hasMedium, scene.instances != nullptr);
    char* pool = static_cast<char*>(st.pool.get());
    if (bytes > st.pool.bytes()) {
        if ((e = grow_buffer(st, stream, st.gbPool, bytes)) != hipSuccess) { error = "hipMalloc(G-buffer queue pool, " + std::to_string(bytes >> 20) + " MiB)"; return e; }
        pool = static_cast<char*>(st.gbPool.get());
    }
    carve_gbuffer_pool(pool, a, capacity, traits.hasMedium, scene.instances != nullptr);
    if ((e = reserve_spill(st, stream, plan.spillThreads * plan.spillEntries, a, error)) != hipSuccess) return e;
    // one sample per pixel, one light slot, rays from the path queue; no shading-class sort and no slim shadow entries (both stay zero)
    a.maxLights = 1; a.spp = 1; a.primary = 0u; a.nodeLoopMin = plan.nodeLoopMin;
    a.numSamples = (uint32_t)pixelsPadded; a.segSize = plan.batch.segSize; a.numSegments = plan.batch.numSegments;
    JitterTable jt{};
    jt.j[0].x = constants.m_Jitter[0]; jt.j[0].y = constants.m_Jitter[1];      // the caller's jitter, not the Halton point of the index (pass 0 for pixel centres)
    GBufferPlanes g; for (uint32_t k = 0; k < kGbPlanes; ++k) g.plane[k] = planes[k];
    const dim3 grid(plan.batch.grid);
    hipLaunchKernelGGL(wf_raygen, grid, dim3(kBlock), 0, stream, a, constants, jt);
    launch_extend(plan.vE, cus, dim3(plan.batch.gridExtend), stream, a, 0u);
    if (motion && planeMask != 0u) hipLaunchKernelGGL(wf_gbuffer_motion<true>, grid, dim3(kBlock), 0, stream, a, constants, g, planeMask, *motion);
    else if (motion) hipLaunchKernelGGL(wf_gbuffer_motion<false>, grid, dim3(kBlock), 0, stream, a, constants, g, planeMask, *motion);
    else hipLaunchKernelGGL(wf_gbuffer, grid, dim3(kBlock), 0, stream, a, constants, g, planeMask);
    if ((e = hipGetLastError()) != hipSuccess) { error = "kernel launch"; return e; }
    return hipSuccess;
}

// hrpt_trace_radiance, wavefront path: wf_raygen_rays, the render's bounces (run_bounces with plan_radiance's plan; from bounce 1 with `secondary`), wf_store_radiance, in batches of
// radiance_batch_rays. Like wavefront_gbuffer it touches neither st.plan nor the byte / timing accounting of renders and counts into a scratch
// counter block; it works in the render's queue pool when that holds a batch, otherwise in a pool of its own.
hipError_t wavefront_radiance(WavefrontState& st, const SceneView& scene, const SceneTraits& traits, const HrptPathTracerConstants& constants,
                              const HrptRay* rays, float4* radiance, uint64_t count, bool accumulate, bool secondary, hipStream_t stream, std::string& error)
{
    if (count == 0) return hipSuccess;
    hipError_t e; uint32_t cus = 0;
    if ((e = device_cus(st, cus, error)) != hipSuccess) return e;
    TreeCounts tree = tree_counts(scene);
    tree.instanceCount = st.shadeInstances; tree.materialCount = st.shadeMaterials;
    const RenderPlan plan = plan_radiance(traits, tree, constants.m_LightCount, cus, st.knobs);
    WfArgs a{};
    fill_scene_args(a, st, scene, traits, TileRect{}, 0u);     // (no rectangle: nothing between raygen and resolve reads one)
    // ---- 1. the batch size and the queue pool: a render's streams and, behind them, the scratch counters
    const bool hasInstances = scene.instances != nullptr;
    auto carve = [&](char* base, uint64_t capacity) {
        const size_t bytes = carve_pool(base, a, capacity, plan.maxLights, traits, hasInstances);
        a.counters = reinterpret_cast<DeviceCounters*>(reinterpret_cast<uintptr_t>(base) + bytes);
        return bytes + sizeof(DeviceCounters) * kCounterShards;
    };
    uint64_t batchRays = radiance_batch_rays(count, plan, 0, st.knobs);
    size_t bytes = carve(nullptr, radiance_capacity(batchRays));
    char* pool = static_cast<char*>(st.pool.get());
    if (bytes > st.pool.bytes()) {
        if (bytes > st.radPool.bytes()) {     // the pool has to grow: within half of what the device has free, as a render's
            size_t freeB = 0, totalB = 0;
            if (hipMemGetInfo(&freeB, &totalB) == hipSuccess) batchRays = radiance_batch_rays(count, plan, (uint64_t)(freeB + st.radPool.bytes()) / 2, st.knobs);
        }
        for (;;) {
            bytes = carve(nullptr, radiance_capacity(batchRays));
            if ((e = grow_buffer(st, stream, st.radPool, bytes)) == hipSuccess) break;
            (void)hipGetLastError();
            if (batchRays <= kMaxSegment) { error = "hipMalloc(radiance queue pool, " + std::to_string(bytes >> 20) + " MiB)"; return e; }
            batchRays = (batchRays + 1) / 2;
        }
        pool = static_cast<char*>(st.radPool.get());
    }
    carve(pool, radiance_capacity(batchRays));
    if ((e = reserve_spill(st, stream, plan.spillThreads * plan.spillEntries, a, error)) != hipSuccess) return e;
    // ---- 2. the arguments the plan decides (one sample per ray; a.primary stays 0: every bounce reads the path queue)
    a.maxLights = plan.maxLights; a.sortShade = plan.sortShade; a.nodeLoopMin = plan.nodeLoopMin; a.slimShadow = plan.slim ? 1u : 0u; a.spp = 1;
    a.shadeInstances = tree.instanceCount; a.shadeMaterials = tree.materialCount;
    // ---- 3. per batch: the rays into path queue 0, the bounces, sampleRadiance out
    for (uint64_t first = 0; first < count; first += batchRays) {
        a.numSamples = (uint32_t)((count - first) < batchRays ? (count - first) : batchRays);
        const BatchPlan batch = plan_batch(plan, st.knobs, a.numSamples);
        a.segSize = batch.segSize; a.numSegments = batch.numSegments;
        hipLaunchKernelGGL(wf_raygen_rays, dim3(batch.grid), dim3(kBlock), 0, stream, a, reinterpret_cast<const float4*>(rays + first));
        if ((e = run_bounces(st, plan, traits, cus, batch, stream, a, constants, false, error, secondary ? 1 : 0)) != hipSuccess) return e;
        uint32_t sgrid = (a.numSamples + kBlock - 1) / kBlock; if (sgrid > cus * 8) sgrid = cus * 8;
        hipLaunchKernelGGL(wf_store_radiance, dim3(sgrid), dim3(kBlock), 0, stream, a, radiance + first, accumulate ? 1u : 0u);
        if ((e = hipGetLastError()) != hipSuccess) { error = "kernel launch"; return e; }
    }
    return hipSuccess;
}

} // namespace hrt
