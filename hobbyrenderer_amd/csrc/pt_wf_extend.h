// pt_wf_extend.h -- the persistent refilling traversal: the waves-per-SIMD settings of the traversal and shading kernels with the measurements
// behind them, wf_extend (closest hits of a path queue, the any-hit pass over the shadow-ray queue, the bounce-0 instantiations that derive
// their rays from the sample index) and wf_trace_rays with its WfTraceArgs (hrpt_trace_rays over a caller's rays through the same loop).
// A piece of pt_wavefront.hip, included there after pt_wf_common.h: no stand-alone header.
// ------------------------------------------------------------------ extend (closest hit)
// Persistent while-while traversal with lane refill: a wave keeps up to 64 rays of its segment in flight; whenever
// at least kRefillMin lanes have finished their ray, they fetch the next rays of the segment (ballot + prefix rank),
// so the traversal loop runs with full lanes instead of waiting for the slowest ray of a 64-ray batch.
// Waves per SIMD the kernels are compiled for (amdgpu_waves_per_eu; measured on MI355X, built without the SLP vectoriser -- csrc/Makefile):
//   wf_extend, tree in LDS      6   80 VGPRs without spills; the <PRIMARY> instantiation gives up 10 registers for it (-1.5 %)
//   wf_extend, tree in global   6   80-82 VGPRs since nodes and triangles are addressed by 32-bit offsets (84 and +2 % at 6 waves before): config 4 -2 %
//   wf_extend<TL>               5   100-117 VGPRs: a few spilled registers buy the fifth wave (-4 %); with the SLP vectoriser on the same
//                                   setting doubled the kernel's time (128 VGPRs wanted)
//   wf_shade, any variant       4   general single-light variant: 121-129 VGPRs wanted, -14 % against 3 waves. The same setting produced wrong sky
//                                   radiance while the SLP vectoriser was on (138 VGPRs wanted). Root cause (round 3, profiles/r03_wrong_sky_isa_evidence.txt):
//                                   a backend bug under register pressure -- the hoisted constant of mie_phase was kept alive through a live-range-split
//                                   copy placed in ONE arm of a divergent if/else, so the lanes of the other arm restored garbage. The guards: the random
//                                   trait scenes of the GPU suite (seed 1 fails on that build) and tests/test_kernel_resources.py (no scratch, <= 128
//                                   VGPRs). Re-check both whenever this kernel, the flags or the compiler change. 5 waves on <SIMPLE>: no gain
constexpr int kWavesExtendLds = 6, kWavesExtendGlobal = 6, kWavesExtendTwoLevel = 5, kWavesShade = 4;
#ifndef HRPT_WAVES_EXTEND_LDS_OPAQUE
#define HRPT_WAVES_EXTEND_LDS_OPAQUE 6
#endif
constexpr int kWavesExtendLdsOpaque = HRPT_WAVES_EXTEND_LDS_OPAQUE;
constexpr uint32_t kNoPathRecord = 0xFFFFFFFEu;     // hit-record code of a slot without a path (wf_extend<PRIMARY>; 0xFFFFFFFF = miss)

// ANYHIT: the same persistent loop over the shadow-ray queue (sqO / sqD / sqId, sqCnt rays per segment): the first hit on an opaque
// triangle ends the ray (kVisBlocked); otherwise the ray is clear or, if it crossed non-opaque triangles, left to wf_shadow's candidate
// pass (kVisCandidates). Shadow rays get the lane refill closest-hit rays have: 3.8 -> 8 Grays/s on the glass config.
// TL: the two-level structure of instanced scenes (pt_traverse.h "two-level traversal"): tree in global memory, closest hits only, every
// instance opaque; the hit's instance goes to its own stream (hitInst) next to the hit record.
// PRIMARY: bounce 0 of a batch without a raygen pass (WfArgs::primary): the refill derives the ray from the sample index. A separate instantiation:
// as a run-time branch the extra live state cost the kernel 6 VGPRs and 3 % on EVERY bounce.
// TL: 0 flat tree, 1 two-level structure with ForceOpaque instances only, 2 two-level with non-opaque instances (candidate re-trace compiled in)
// OPQ: no instance of the scene is ForceNonOpaque (closest-hit launches of the flat structure): the candidate rules of TraceRayStandard (lower
// bound of a re-trace, stochastic-alpha draws) are compiled out -- every hit is committed.
template <bool LDS_BVH, int DEPTH, int W, bool ANYHIT, int TL = 0, bool PRIMARY = false, bool OPQ = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(TL ? kWavesExtendTwoLevel : (LDS_BVH ? (OPQ ? kWavesExtendLdsOpaque : kWavesExtendLds) : kWavesExtendGlobal)))) void wf_extend(WfArgs a, uint32_t parity)
{
    static_assert(!OPQ || (!ANYHIT && !TL), "OPQ: closest hits over the flat structure");
    static_assert(!TL || (!LDS_BVH && !ANYHIT && W == 4), "two-level traversal: global 4-wide tree, closest hit");
    static_assert(!PRIMARY || !ANYHIT, "primary rays are closest-hit rays");
    static_assert(W != kQuantisedTree || (!LDS_BVH && !TL), "quantised nodes: flat tree in global memory");
    extern __shared__ __attribute__((aligned(128))) char smem[];
    LdsStack<DEPTH, kExtendLdsStack> stack; LdsBvh<W> lbvh;
    constexpr size_t candBytes = ANYHIT ? (size_t)kShadowCandidates * 2 * kBlock * 4 : 0;
    setup_lds<LDS_BVH, DEPTH, W>(smem, a.scene, stack, lbvh, candBytes);
    LdsCandidates cand; cand.base = reinterpret_cast<int32_t*>(smem + (size_t)LdsStack<DEPTH, kExtendLdsStack>::kRows * kBlock * 4) + threadIdx.x;
    if (DEPTH > kExtendLdsStack) { stack.spill = a.spill[ANYHIT ? 1 : 0] + blockIdx.x * kBlock + threadIdx.x; stack.spillStride = gridDim.x * kBlock; }
    typename GlobalBvhOf<(TL ? kTwoLevelTree : W)>::type gbvh = GlobalBvhOf<(TL ? kTwoLevelTree : W)>::make(a.scene);
    const SceneView& s = a.scene;

    const uint32_t wavesPerBlock = kBlock / 64;
    const uint32_t gw = uniform(blockIdx.x * wavesPerBlock + (threadIdx.x >> 6)), totalWaves = gridDim.x * wavesPerBlock;
    const float4* __restrict__ rayO = ANYHIT ? a.b.sqO : a.b.rayO[parity];
    float4* __restrict__ rayD = ANYHIT ? a.b.sqD : a.b.rayD[parity];
    const uint32_t* __restrict__ segCount = ANYHIT ? a.b.sqCnt : a.b.pathCnt[parity];
    const uint32_t slotsPerSample = ANYHIT ? a.maxLights : 1u;
    unsigned int nRays = 0;
    const bool emptyScene = s.nodeCount == 0 && s.rootLeaf == 0;

    // The wave streams through its segments (gw, gw + totalWaves, ...) without draining between them: when one segment has been
    // handed out completely the idle lanes refill from the next one, so only the very end of the wave's work runs with few lanes.
    {
        uint32_t seg = gw, cnt = 0, segBase = 0, next = 0;      // wave-uniform cursor: next ray of the current segment to hand out
        bool haveSeg = false;
        auto open_segment = [&]() {                             // first non-empty segment at or after `seg`
            haveSeg = false; cnt = 0; next = 0;
            for (; seg < a.numSegments; seg += totalWaves) {
                cnt = uniform(PRIMARY ? path_count(a, 0u, seg) : segCount[seg]);
                if (cnt) { segBase = (seg * a.segSize) * slotsPerSample; haveSeg = true; break; }
            }
        };
        open_segment();
        // per-lane traversal state
        bool active = false;
        Ray r; r.o = mk3(0.0f, 0.0f, 0.0f); r.d = mk3(0.0f, 0.0f, 1.0f); r.tmin = 0.0f; r.tmax = 1e10f;
        RayShear sh = make_shear(r.d); f3 inv = mk3(0.0f, 0.0f, 0.0f), noi = mk3(0.0f, 0.0f, 0.0f);
        TlCull tl; tl.inv = inv; tl.noi = noi; tl.noiF = noi; tl.inst = -1;      // TL only (dead otherwise)
        HitKey lower; lower.have = false; lower.t = 0.0f; lower.inst = 0; lower.prim = 0;
        Hit best; best.valid = false; best.t = 0.0f; best.inst = 0; best.prim = 0; best.u = 0.0f; best.v = 0.0f; best.opaque = 0; best.tri = 0;
        int32_t cur = kTraversalDone; int sp = 0; uint32_t slot = 0, rng = 0, rng0 = 0; float tlim = 0.0f;
        bool blocked = false, candOverflow = false; int candCount = 0;
        for (;;) {
            if (haveSeg && next >= cnt && (a.streamSegments || __ballot(active) == 0ull)) { seg += totalWaves; open_segment(); }
            // ---- refill idle lanes
            unsigned long long mIdle = __ballot(!active);
            uint32_t nIdle = (uint32_t)__popcll(mIdle);
            if (active) HRT_PHASE(ANYHIT ? PH_ANY_ITER : PH_EXT_ITER);
            if (haveSeg && (nIdle >= a.refillMin || nIdle == 64u)) {
                const uint32_t idx = next + prefix_rank(mIdle);
                bool take = !active && idx < cnt;
                if constexpr (PRIMARY) {                // bounce 0, rays from the sample index (false: padding pixel of an 8 x 8 tile)
                    if (take) {
                        slot = segBase + idx; take = primary_ray(a, *a.primaryArgs, slot, r.o, r.d, rng); r.tmin = 0.0f; r.tmax = 1e10f; rng0 = rng;
                        if (take) rayD[slot] = make_float4(r.d.x, r.d.y, r.d.z, __uint_as_float(rng));      // for wf_shade(0) / wf_shadow(0): direction + RNG seed
                        else a.b.hit[slot] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(kNoPathRecord));   // padding pixel of an 8 x 8 tile: wf_shade skips the slot
                    }
                }
                if (take) {
                    HRT_PHASE(ANYHIT ? PH_ANY_REFILL : PH_EXT_REFILL);
                    if constexpr (!PRIMARY) {
                        slot = segBase + idx;
                        float4 o = rayO[slot], d = rayD[slot];
                        r.o = mk3(o.x, o.y, o.z); r.d = mk3(d.x, d.y, d.z); r.tmin = o.w; r.tmax = ANYHIT ? d.w : 1e10f;
                        rng = __float_as_uint(d.w); rng0 = rng;
                    }
                    blocked = false; candOverflow = false; candCount = 0;
                    lower.have = false;
                    best.valid = false; tlim = r.tmax; sp = 0;
                    bool finite = (r.d.x == r.d.x && r.d.y == r.d.y && r.d.z == r.d.z);
                    sh = make_shear(r.d);
                    if constexpr (TL) tl_world(tl, r); else { inv = traversal_rcp(r.d); noi = slab_origin_term(r.o, inv); }
                    cur = (emptyScene || !finite) ? kTraversalDone : (s.nodeCount == 0 ? s.rootLeaf : 0);
                    active = true; ++nRays;
                }
                next += nIdle;
            }
            if (__ballot(active) == 0ull) { if (haveSeg) continue; break; }
            if (active) {
                // ---- descend inner nodes until this lane holds a leaf (or its stack ran out)
                // (the descent is cut short once fewer than nodeLoopMin lanes are still at inner nodes: the rest of the wave holds leaves and
                // would only wait; the lanes cut off keep their node and go on in the next round. Thresholded while-while.)
                if constexpr (TL) {
                    while (cur >= 0 && cur != kExitBlas) {
                        cur = inner_step(gbvh, cur, tl.noi, tl.noiF, tl.inv, r.tmin, tlim, stack, sp);
                        if ((uint32_t)__popcll(__ballot(cur >= 0 && cur != kExitBlas)) < a.nodeLoopMin) break;
                    }
                    // leaving an instance / entering one: the lane continues with the next tree in the next round
                    if (cur == kExitBlas || (cur < 0 && cur != kTraversalDone && tl.inst < 0)) cur = tl_switch(gbvh, cur, tl, r, stack, sp);
                    else if (cur < 0 && cur != kTraversalDone) {
                        const GpuInstance& I = s.instances[tl.inst];
                        const uint32_t enc = (uint32_t)(~cur), first = enc >> 2, count = (enc & 3u) + 1u;
                        const uint32_t inst = (uint32_t)tl.inst, iflags = I.flags & 7u;
                        for (uint32_t i = 0; i < count; ++i) {
                            float4 ta, tb, tc; gbvh.tri(first + i, ta, tb, tc);
                            f3 p0, p1, p2; tl_world_triangle(I, ta, tb, tc, p0, p1, p2);
                            float t, u, v;
                            const bool hitTri = tri_test(p0, p1, p2, r, sh, t, u, v);
                            const uint32_t prim = __float_as_uint(tb.w);
                            // Written as selects on one flag (every closest-hit loop of the library is). As `if (take) { best.t = t; ... }` this loop was
                            // compiled (ROCm 7.2, gfx950) to code that, on a tie in t won by (instance, primitive), took the new key but kept the OLD
                            // barycentrics: hits on an edge shared by two triangles then shaded with the other triangle's (u, v).
                            // tests/test_two_level_gpu.py::test_two_level_full_frame holds such a pixel; the select form is also 1 % faster.
                            const bool ok = TL != 2 || !lower.have || key_less(lower.t, lower.inst, lower.prim, t, inst, prim);       // behind a rejected non-opaque candidate
                            const bool take = hitTri && ok && (!best.valid || key_less(t, inst, prim, best.t, best.inst, best.prim));
                            best.t = take ? t : best.t; best.u = take ? u : best.u; best.v = take ? v : best.v;
                            best.inst = take ? inst : best.inst; best.prim = take ? prim : best.prim; best.tri = take ? first + i : best.tri;
                            best.opaque = take ? iflags : best.opaque;
                            best.valid = best.valid || take;
                            tlim = take ? t : tlim;
                        }
                        cur = stack.pop(--sp);      // the exit marker is below every entry pushed inside an instance
                    }
                } else {
                while (cur >= 0) {
                    HRT_PHASE(ANYHIT ? PH_ANY_NODE : PH_EXT_NODE);
                    if (LDS_BVH) cur = inner_step(lbvh, cur, noi, inv, r.tmin, tlim, stack, sp);
                    else cur = inner_step(gbvh, cur, noi, inv, r.tmin, tlim, stack, sp);
                    if ((uint32_t)__popcll(__ballot(cur >= 0)) < a.nodeLoopMin) break;
                }
                }
                // ---- intersect the leaf
                if (!TL && cur < 0 && cur != kTraversalDone) {
                    uint32_t enc = (uint32_t)(~cur);
                    uint32_t first = enc >> 2, count = (enc & 3u) + 1u;
                    HRT_PHASE(ANYHIT ? PH_ANY_LEAF : PH_EXT_LEAF);
                    for (uint32_t i = 0; i < count; ++i) {
                        HRT_PHASE(ANYHIT ? PH_ANY_TRI : PH_EXT_TRI);
                        float4 ta, tb, tc;
                        if (LDS_BVH) lbvh.tri(first + i, ta, tb, tc); else gbvh.tri(first + i, ta, tb, tc);
                        float t, u, v;
                        if (tri_test(mk3(ta.x, ta.y, ta.z), mk3(tb.x, tb.y, tb.z), mk3(tc.x, tc.y, tc.z), r, sh, t, u, v)) {
                            if (ANYHIT) {
                                if (__float_as_uint(tc.w) & 1u) { blocked = true; break; }     // opaque instance: committed, whatever lies in front of it
                                if (LDS_BVH) candidate_insert<kShadowCandidates>(lbvh, cand, candCount, candOverflow, t, first + i, __float_as_uint(ta.w), __float_as_uint(tb.w));
                                else candidate_insert<kShadowCandidates>(gbvh, cand, candCount, candOverflow, t, first + i, __float_as_uint(ta.w), __float_as_uint(tb.w));
                                continue;
                            }
                            uint32_t inst = __float_as_uint(ta.w), prim = __float_as_uint(tb.w);
                            const bool ok = OPQ || !lower.have || key_less(lower.t, lower.inst, lower.prim, t, inst, prim);
                            const bool take = ok && (!best.valid || key_less(t, inst, prim, best.t, best.inst, best.prim));      // selects: see the two-level loop above
                            best.t = take ? t : best.t; best.u = take ? u : best.u; best.v = take ? v : best.v;
                            best.inst = take ? inst : best.inst; best.prim = take ? prim : best.prim; best.tri = take ? first + i : best.tri;
                            best.opaque = take ? (__float_as_uint(tc.w) & 7u) : best.opaque;     // bit 0 opaque, bits 1-2 shading class
                            best.valid = best.valid || take;
                            tlim = take ? t : tlim;
                        }
                    }
                    cur = (blocked || sp == 0) ? kTraversalDone : stack.pop(--sp);
                }
                // ---- traversal finished: candidate resolution (TraceRayStandard) and hit record
                if (ANYHIT) {
                    if (cur == kTraversalDone) {
                        HRT_PHASE(PH_ANY_FINISH);
                        const uint32_t id = a.b.sqId[slot];
                        uint32_t code = blocked ? kVisBlocked : kVisClear;
                        if (!blocked && candCount > 0) {
                            uint2* out = a.b.sqCand + (size_t)id * kShadowCandidates;
                            for (int k = 0; k < candCount; ++k) { float ct; uint32_t ctri; cand.key(k, ct, ctri); out[k] = make_uint2(__float_as_uint(ct), ctri); }
                            code = kVisCandidates | ((uint32_t)candCount << 8) | (candOverflow ? 1u << 16 : 0u);
                        }
                        a.b.shVis[id] = code;
                        active = false;
                    }
                } else if (cur == kTraversalDone) {
                    bool done = true;
                    HRT_PHASE(PH_EXT_FINISH);
                    if (!OPQ && TL != 1 && best.valid && !(best.opaque & 1u)) HRT_PHASE(PH_EXT_CANDIDATE);
                    if (!OPQ && TL != 1 && best.valid && !(best.opaque & 1u) && !candidate_commits(s, best, rng)) {
                        // rejected non-opaque candidate: it becomes the exclusive lower bound of a new closest-hit query
                        lower.have = true; lower.t = best.t; lower.inst = best.inst; lower.prim = best.prim;
                        best.valid = false; tlim = r.tmax; sp = 0;
                        cur = s.nodeCount == 0 ? s.rootLeaf : 0;
                        if constexpr (TL) tl_world(tl, r);
                        done = false;
                    }
                    if (done) {
                        if (!OPQ && a.hasStochasticAlpha && rng != rng0) { float4 d = rayD[slot]; d.w = __uint_as_float(rng); rayD[slot] = d; }
                        // hit record: triangle (< 2^29: leaf references hold first << 2) | shading class << 29; 0xFFFFFFFF = miss
                        a.b.hit[slot] = make_float4(best.t, best.u, best.v, __uint_as_float(best.valid ? (best.tri | ((best.opaque >> 1) << 29)) : 0xFFFFFFFFu));
                        if constexpr (TL) a.b.hitInst[slot] = best.inst;
                        active = false;
                    }
                }
            }
        }
    }
    if (!ANYHIT) block_count_add(&a.counters->closestRays, 0, nRays);      // shadow rays are counted by wf_shadow
    if (PRIMARY) { __syncthreads(); block_count_add(&a.counters->closestRays, 2, nRays); }      // ... and the paths wf_raygen would have counted
}

// ------------------------------------------------------------------ stand-alone ray queries (hrpt_trace_rays) through the same persistent loop
// TraceRayStandard (RaytracingCommon.hlsli:138-198) / CalculateRTShadow<true> (CommonLighting.hlsli:380-496) for the reference's other inline-RT
// passes (DDGI ProbeTraceCS.hlsl:60-61,108-109, RT shadows, BrdfRayTracing.hlsl:138-140): a caller's array of HrptRay instead of the path queue,
// HrptRayHit records instead of hit records. A wave owns chunks of 256 consecutive rays and refills idle lanes exactly like wf_extend; the
// thread-per-ray kernel of round 1 (pt_megakernel.hip) was 1.8x slower on the same rays. SHADOW: the any-hit traversal gathers the non-opaque
// triangles a ray crosses in per-lane LDS columns; when the ray ends unblocked they are resolved front to back right there.
struct WfTraceArgs {
    SceneView scene; const HrptRay* rays; HrptRayHit* hits; uint64_t count;
    int32_t* spill; uint32_t refillMin, nodeLoopMin;
    bool quantised;         // host-side only: the launch picks the instantiation that walks SceneView::nodesQ
};
constexpr uint32_t kTraceChunkShift = 8;
template <bool LDS_BVH, int DEPTH, int W, bool SHADOW, bool TL = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(SHADOW ? 1 : (TL ? kWavesExtendTwoLevel : (LDS_BVH ? kWavesExtendLds : kWavesExtendGlobal))))) void wf_trace_rays(WfTraceArgs a)
{
    static_assert(!TL || (!LDS_BVH && W == 4), "two-level structure: global 4-wide trees (every instance opaque: a shadow ray ends at its first hit)");
    static_assert(W != kQuantisedTree || (!LDS_BVH && !TL), "quantised nodes: flat tree in global memory");
    extern __shared__ __attribute__((aligned(128))) char smem[];
    LdsStack<DEPTH, kExtendLdsStack> stack; LdsBvh<W> lbvh;
    constexpr size_t candBytes = SHADOW ? (size_t)kShadowCandidates * 2 * kBlock * 4 : 0;
    setup_lds<LDS_BVH, DEPTH, W>(smem, a.scene, stack, lbvh, candBytes);
    LdsCandidates cand; cand.base = reinterpret_cast<int32_t*>(smem + (size_t)LdsStack<DEPTH, kExtendLdsStack>::kRows * kBlock * 4) + threadIdx.x;
    if (DEPTH > kExtendLdsStack) { stack.spill = a.spill + blockIdx.x * kBlock + threadIdx.x; stack.spillStride = gridDim.x * kBlock; }
    typename GlobalBvhOf<(TL ? kTwoLevelTree : W)>::type gbvh = GlobalBvhOf<(TL ? kTwoLevelTree : W)>::make(a.scene);
    const SceneView& s = a.scene;
    const uint32_t wavesPerBlock = kBlock / 64;
    const uint32_t gw = uniform(blockIdx.x * wavesPerBlock + (threadIdx.x >> 6)), totalWaves = gridDim.x * wavesPerBlock;
    TlCull tl; tl.inv = mk3(0.0f, 0.0f, 0.0f); tl.noi = tl.inv; tl.noiF = tl.inv; tl.inst = -1;      // TL only
    const uint64_t numChunks = (a.count + (1u << kTraceChunkShift) - 1) >> kTraceChunkShift;
    const bool emptyScene = s.nodeCount == 0 && s.rootLeaf == 0;

    uint64_t chunk = gw; uint32_t cnt = 0, next = 0; uint64_t chunkBase = 0; bool haveChunk = false;
    auto open_chunk = [&]() {
        haveChunk = chunk < numChunks; next = 0;
        if (haveChunk) { chunkBase = chunk << kTraceChunkShift; const uint64_t left = a.count - chunkBase; cnt = left < (1u << kTraceChunkShift) ? (uint32_t)left : (1u << kTraceChunkShift); }
    };
    open_chunk();
    bool active = false;
    Ray r; r.o = mk3(0.0f, 0.0f, 0.0f); r.d = mk3(0.0f, 0.0f, 1.0f); r.tmin = 0.0f; r.tmax = 1e10f;
    RayShear sh = make_shear(r.d); f3 inv = mk3(0.0f, 0.0f, 0.0f), noi = mk3(0.0f, 0.0f, 0.0f);
    HitKey lower; lower.have = false; lower.t = 0.0f; lower.inst = 0; lower.prim = 0;
    Hit best; best.valid = false; best.t = 0.0f; best.inst = 0; best.prim = 0; best.u = 0.0f; best.v = 0.0f; best.opaque = 0; best.tri = 0;
    int32_t cur = kTraversalDone; int sp = 0; uint64_t slot = 0; uint32_t rng = 0; float tlim = 0.0f;
    bool blocked = false, candOverflow = false, finite = true; int candCount = 0;
    for (;;) {
        if (haveChunk && next >= cnt) { chunk += totalWaves; open_chunk(); }
        const unsigned long long mIdle = __ballot(!active);
        const uint32_t nIdle = (uint32_t)__popcll(mIdle);
        if (haveChunk && (nIdle >= a.refillMin || nIdle == 64u)) {
            const uint32_t idx = next + prefix_rank(mIdle);
            if (!active && idx < cnt) {
                slot = chunkBase + idx;
                const float4* rp = reinterpret_cast<const float4*>(a.rays + slot);           // 48-byte records: three 16-byte loads
                const float4 q0 = rp[0], q1 = rp[1]; const uint32_t rr = reinterpret_cast<const uint32_t*>(rp + 2)[0];
                const f3 o = mk3(q0.x, q0.y, q0.z), d = mk3(q1.x, q1.y, q1.z);
                finite = all_finite(o, d);
                if (SHADOW) r = shadow_ray(o, d, q1.w);                                        // the query applies its own bias; tmax = distance to the light
                else { r.o = o; r.d = d; r.tmin = q0.w; r.tmax = q1.w; }
                rng = rr; blocked = false; candOverflow = false; candCount = 0; lower.have = false; best.valid = false; tlim = r.tmax; sp = 0;
                sh = make_shear(r.d);
                if constexpr (TL) tl_world(tl, r); else { inv = traversal_rcp(r.d); noi = slab_origin_term(r.o, inv); }
                cur = (emptyScene || !finite) ? kTraversalDone : (s.nodeCount == 0 ? s.rootLeaf : 0);
                active = true;
            }
            next += nIdle;
        }
        if (__ballot(active) == 0ull) { if (haveChunk) continue; break; }
        if (active) {
            if constexpr (TL) {
                while (cur >= 0 && cur != kExitBlas) {
                    cur = inner_step(gbvh, cur, tl.noi, tl.noiF, tl.inv, r.tmin, tlim, stack, sp);
                    if ((uint32_t)__popcll(__ballot(cur >= 0 && cur != kExitBlas)) < a.nodeLoopMin) break;
                }
                if (cur == kExitBlas || (cur < 0 && cur != kTraversalDone && tl.inst < 0)) cur = tl_switch(gbvh, cur, tl, r, stack, sp);
                else if (cur < 0 && cur != kTraversalDone) {
                    const GpuInstance& I = s.instances[tl.inst];
                    const uint32_t enc = (uint32_t)(~cur), first = enc >> 2, count = (enc & 3u) + 1u, inst = (uint32_t)tl.inst;
                    for (uint32_t i = 0; i < count; ++i) {
                        float4 ta, tb, tc; gbvh.tri(first + i, ta, tb, tc);
                        f3 p0, p1, p2; tl_world_triangle(I, ta, tb, tc, p0, p1, p2);
                        float t, u, v;
                        const bool hitTri = tri_test(p0, p1, p2, r, sh, t, u, v);
                        if (SHADOW) { if (hitTri) { if (I.flags & 1u) { blocked = true; break; } candCount = 1; } continue; }      // candCount: "crossed a non-opaque instance"
                        const uint32_t prim = __float_as_uint(tb.w);
                        const bool ok = !lower.have || key_less(lower.t, lower.inst, lower.prim, t, inst, prim);
                        const bool take = hitTri && ok && (!best.valid || key_less(t, inst, prim, best.t, best.inst, best.prim));      // selects: see wf_extend<TL>
                        best.t = take ? t : best.t; best.u = take ? u : best.u; best.v = take ? v : best.v;
                        best.inst = take ? inst : best.inst; best.prim = take ? prim : best.prim; best.tri = take ? first + i : best.tri;
                        best.valid = best.valid || take; best.opaque = take ? (I.flags & 1u) : best.opaque;
                        tlim = take ? t : tlim;
                    }
                    cur = blocked ? kTraversalDone : stack.pop(--sp);
                }
            } else {
            while (cur >= 0) {
                if (LDS_BVH) cur = inner_step(lbvh, cur, noi, inv, r.tmin, tlim, stack, sp);
                else cur = inner_step(gbvh, cur, noi, inv, r.tmin, tlim, stack, sp);
                if ((uint32_t)__popcll(__ballot(cur >= 0)) < a.nodeLoopMin) break;
            }
            if (cur < 0 && cur != kTraversalDone) {
                const uint32_t enc = (uint32_t)(~cur), first = enc >> 2, count = (enc & 3u) + 1u;
                for (uint32_t i = 0; i < count; ++i) {
                    float4 ta, tb, tc;
                    if (LDS_BVH) lbvh.tri(first + i, ta, tb, tc); else gbvh.tri(first + i, ta, tb, tc);
                    float t, u, v;
                    if (tri_test(mk3(ta.x, ta.y, ta.z), mk3(tb.x, tb.y, tb.z), mk3(tc.x, tc.y, tc.z), r, sh, t, u, v)) {
                        if (SHADOW) {
                            if (__float_as_uint(tc.w) & 1u) { blocked = true; break; }
                            if (LDS_BVH) candidate_insert<kShadowCandidates>(lbvh, cand, candCount, candOverflow, t, first + i, __float_as_uint(ta.w), __float_as_uint(tb.w));
                            else candidate_insert<kShadowCandidates>(gbvh, cand, candCount, candOverflow, t, first + i, __float_as_uint(ta.w), __float_as_uint(tb.w));
                            continue;
                        }
                        const uint32_t inst = __float_as_uint(ta.w), prim = __float_as_uint(tb.w);
                        const bool ok = !lower.have || key_less(lower.t, lower.inst, lower.prim, t, inst, prim);
                        const bool take = ok && (!best.valid || key_less(t, inst, prim, best.t, best.inst, best.prim));      // selects: see wf_extend
                        best.t = take ? t : best.t; best.u = take ? u : best.u; best.v = take ? v : best.v;
                        best.inst = take ? inst : best.inst; best.prim = take ? prim : best.prim; best.tri = take ? first + i : best.tri;
                        best.opaque = take ? (__float_as_uint(tc.w) & 1u) : best.opaque;
                        best.valid = best.valid || take;
                        tlim = take ? t : tlim;
                    }
                }
                cur = (blocked || sp == 0) ? kTraversalDone : stack.pop(--sp);
            }
            }
            if (cur == kTraversalDone) {
                HrptRayHit out; out.t = 0.0f; out.u = 0.0f; out.v = 0.0f; out.instance = 0; out.primitive = 0; out.hit = 0; out.rng = rng; out.pad = 0;
                bool done = true;
                if (SHADOW) {
                    float vis = 1.0f;
                    if (finite) {
                        if (blocked) vis = 0.0f;
                        else if (candCount > 0) {
                            if constexpr (TL) vis = shadow_retrace(s, gbvh, r, stack);
                            else if (LDS_BVH) vis = shadow_resolve_candidates(s, lbvh, r, sh, candCount, candOverflow, cand, stack);
                            else vis = shadow_resolve_candidates(s, gbvh, r, sh, candCount, candOverflow, cand, stack);
                        }
                    }
                    out.t = vis; out.hit = vis < 1.0f ? 1u : 0u;
                } else if (best.valid && !best.opaque && !candidate_commits(s, best, rng)) {
                    lower.have = true; lower.t = best.t; lower.inst = best.inst; lower.prim = best.prim;
                    best.valid = false; tlim = r.tmax; sp = 0;
                    cur = s.nodeCount == 0 ? s.rootLeaf : 0;
                    if constexpr (TL) tl_world(tl, r);
                    done = false;
                } else if (best.valid) { out.t = best.t; out.u = best.u; out.v = best.v; out.instance = best.inst; out.primitive = best.prim; out.hit = 1u; out.rng = rng; }
                if (done) {
                    out.rng = rng;
                    float4* hp = reinterpret_cast<float4*>(a.hits + slot);
                    hp[0] = make_float4(out.t, out.u, out.v, __uint_as_float(out.instance));
                    hp[1] = make_float4(__uint_as_float(out.primitive), __uint_as_float(out.hit), __uint_as_float(out.rng), 0.0f);
                    active = false;
                }
            }
        }
    }
}
