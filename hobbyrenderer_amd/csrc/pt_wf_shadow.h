// pt_wf_shadow.h -- the NEE visibility stage: wf_shadow_rays (one compacted ray per valid light sample, for the any-hit pass of scenes with
// non-opaque geometry) and wf_shadow (visibility of every shadow-queue entry in one of the kShadow* modes, BRDF x radiance of the unoccluded
// samples, added into sampleRadiance). A piece of pt_wavefront.hip, included there after pt_wf_common.h: no stand-alone header.
// ------------------------------------------------------------------ shadow rays (scenes with non-opaque geometry)
// One ray per valid light sample of every shadow-queue entry, compacted per segment, for the any-hit pass of wf_extend<ANYHIT>.
// nee_direction is evaluated here and again in wf_shadow (same inputs, same bits) rather than stored: 40 B per sample less traffic.
template <bool DIRONLY>
__global__ __launch_bounds__(kBlock) void wf_shadow_rays(WfArgs a, HrptPathTracerConstants cb)
{
    const SceneView& s = a.scene;
    const f3 sunDir = mk3(cb.m_SunDirection[0], cb.m_SunDirection[1], cb.m_SunDirection[2]);
    const uint32_t wavesPerBlock = kBlock / 64, lane = lane_id();
    const uint32_t gw = uniform(blockIdx.x * wavesPerBlock + (threadIdx.x >> 6)), totalWaves = gridDim.x * wavesPerBlock;
    for (uint32_t seg = gw; seg < a.numSegments; seg += totalWaves) {
        const uint32_t cnt = uniform(a.b.shadowCnt[seg]), segBase = seg * a.segSize, items = cnt * a.maxLights;
        uint32_t outCount = 0;
        for (uint32_t i0 = 0; i0 < items; i0 += 64) {
            const uint32_t i = i0 + lane;
            bool valid = false; Ray ray; uint32_t id = 0;
            if (i < items) {
                HRT_PHASE(PH_SHADOW_RAYS_ITEM);
                const uint32_t el = i / a.maxLights, j = i - el * a.maxLights, e = segBase + el;
                id = e * a.maxLights + j;
                float4 h4 = a.b.sh4[e];
                if (j < __float_as_uint(h4.w)) {
                    float4 h0 = a.b.sh0[e], h1 = a.b.sh1[e], ls = a.b.shL[(size_t)e * a.maxLights + j];
                    HrptGPULight l = load_light(s, __float_as_uint(ls.z));
                    f3 L; float maxDist;
                    if (nee_direction<DIRONLY>(l, mk3(h1.x, h1.y, h1.z), mk3(h0.x, h0.y, h0.z), sunDir, cb.m_CosSunAngularRadius, ls.x, ls.y, L, maxDist)) {
                        ray = shadow_ray(mk3(h0.x, h0.y, h0.z), L, maxDist);
                        valid = true;
                    }
                }
                if (!valid) a.b.shVis[id] = kVisNoRay;
            }
            const unsigned long long m = __ballot(valid);
            if (valid) {
                const uint32_t o = segBase * a.maxLights + outCount + prefix_rank(m);
                a.b.sqO[o] = make_float4(ray.o.x, ray.o.y, ray.o.z, ray.tmin);
                a.b.sqD[o] = make_float4(ray.d.x, ray.d.y, ray.d.z, ray.tmax);
                a.b.sqId[o] = id;
            }
            outCount += (uint32_t)__popcll(m);
        }
        if (lane == 0) a.b.sqCnt[seg] = outCount;
    }
}

// ------------------------------------------------------------------ shadow (NEE visibility + accumulation)
// MODE: kShadowOpaque / kShadowBuffered / kShadowResolve / kShadowSlim (pt_wavefront_plan.h)
// Waves per SIMD (built without the SLP vectoriser, csrc/Makefile): the buffered variant is held at 3 -- the gradient-sampled alpha test of
// mip-mapped MASK textures, a rare path, would otherwise cost every scene with alpha-tested geometry a wave (145-152 VGPRs; at 4 waves config 4's
// shadow stage is 6 % SLOWER: it traverses, and spills hurt its loops); the resolve variant runs at 4 (146-150 VGPRs wanted, 128 given: it waits
// on its queue reads for 71 % of its cycles and only walks candidate lists: glass config shadow stage -6 %); the two-level variants at 3
// (scenes with non-opaque instances -16 % shadow time). Forced budgets are re-checked with the random trait scenes (scripts/parity_campaign.sh:
// HRPT_WF_SHADOW_PATH=1 / 2 and the two-level scenes), because one has broken wf_shade's general variant before.
template <bool LDS_BVH, int DEPTH, int W, bool DIRONLY, int MODE, int TL = 0>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(MODE == 2 && TL == 0 ? 4 : ((MODE == 1 || TL != 0) ? 3 : 1)))) void wf_shadow(WfArgs a, HrptPathTracerConstants cb, int bounce)
{
    static_assert(!TL || (!LDS_BVH && W == 4 && (MODE == kShadowOpaque || MODE == kShadowSlim)), "two-level structure: the opaque / slim modes over the global tree (any-hit query, or with TL == 2 the buffered candidate query)");
    static_assert(W != kQuantisedTree || (!LDS_BVH && !TL), "quantised nodes: flat tree in global memory");
    constexpr bool NONOPAQUE = MODE == kShadowBuffered || MODE == kShadowResolve;
    constexpr bool SLIM = MODE == kShadowSlim;
    constexpr int kLdsMax = MODE == kShadowResolve ? kExtendLdsStack : kShadowLdsStack;
    extern __shared__ __attribute__((aligned(128))) char smem[];
    LdsStack<DEPTH, kLdsMax> stack; LdsBvh<W> lbvh;
    constexpr size_t candBytes = MODE == kShadowBuffered ? (size_t)kShadowCandidates * 2 * kBlock * 4 : 0;
    setup_lds<LDS_BVH, DEPTH, W>(smem, a.scene, stack, lbvh, candBytes);
    if (DEPTH > kLdsMax) { stack.spill = a.spill[1] + blockIdx.x * kBlock + threadIdx.x; stack.spillStride = gridDim.x * kBlock; }
    LdsCandidates cand; cand.base = reinterpret_cast<int32_t*>(smem + (size_t)LdsStack<DEPTH, kLdsMax>::kRows * kBlock * 4) + threadIdx.x;
    LdsCandidates3 cand3; cand3.base = cand.base;        // TL == 2: (t, mesh triangle, instance) columns in the same place (the launch adds their bytes)
    typename GlobalBvhOf<(TL ? kTwoLevelTree : W)>::type gbvh = GlobalBvhOf<(TL ? kTwoLevelTree : W)>::make(a.scene);
    const SceneView& s = a.scene;
    const f3 sunDir = mk3(cb.m_SunDirection[0], cb.m_SunDirection[1], cb.m_SunDirection[2]);
    const float sunIntensity = s.lights[0].m_Intensity;      // g_Lights[0], PathTracer.hlsl:137 (reference quirk kept)

    const uint32_t wavesPerBlock = kBlock / 64, lane = lane_id();
    const uint32_t gw = uniform(blockIdx.x * wavesPerBlock + (threadIdx.x >> 6)), totalWaves = gridDim.x * wavesPerBlock;
    unsigned int nRays = 0, nSamples = 0, nRadiance = 0, nSkipped16 = 0;
    // the query of kShadowOpaque / kShadowSlim (no ForceNonOpaque instance in a flat scene): the any-hit pass over the LDS or the global tree;
    // TL == 2: the buffered query over the two-level structure, whose instances may be non-opaque
    auto opaque_query = [&](f3 origin, f3 L, float maxDist) {
        if (LDS_BVH) return shadow_query<true>(s, lbvh, origin, L, maxDist, stack);
        else if constexpr (TL == 2) return shadow_query_two_level_buffered<kTwoLevelCandidates>(s, gbvh, shadow_ray(origin, L, maxDist), stack, cand3);
        else return shadow_query<true>(s, gbvh, origin, L, maxDist, stack);
    };
    // one shadow-queue entry: every light sample of one path vertex
    auto process = [&](uint32_t e) {
                HRT_PHASE(PH_SHADOW_ENTRY);
                if (SLIM) {
                    const float4 h0 = a.b.sh0[e], h1 = a.b.sh1[e];
                    const uint32_t slot = __float_as_uint(h0.w);
                    const float4 rd = a.b.rayD[a.shadowParity][slot];
                    const f3 origin = mk3(h0.x, h0.y, h0.z), N = mk3(h1.x, h1.y, h1.z);
                    uint32_t rng = __float_as_uint(rd.w);
                    const float ux = hrt_rng_next(&rng), uy = hrt_rng_next(&rng);      // the two draws of nee_draw (CommonLighting.hlsli:730)
                    ++nSamples;
                    HrptGPULight l = load_light(s, 0u);
                    f3 L; float maxDist;
                    if (!nee_direction<true>(l, N, origin, sunDir, cb.m_CosSunAngularRadius, ux, uy, L, maxDist)) return;
                    const float shadow = opaque_query(origin, L, maxDist);
                    ++nRays;
                    if (shadow != 0.0f) {
                        const float4 th = a.primary ? make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(slot)) : a.b.thr[a.shadowParity][slot];
                        if (a.primary) ++nSkipped16;
                        const HrptMaterialConstants& mat = s.materials[__float_as_uint(h1.w)];
                        // GetPBRAttributes without textures (RaytracingCommon.hlsli:252-296): constants, roughness clamped at 0.04
                        f3 dif, spec;
                        nee_contribution<true>(s, l, nee_lighting(N, mk3(-rd.x, -rd.y, -rd.z), mk3(mat.m_BaseColor), hrt_max(mat.m_RoughnessMetallic[0], 0.04f),
                                                                  mat.m_RoughnessMetallic[1], mat.m_IOR), origin, sunDir, sunIntensity, L, dif, spec);
                        f3 totalDiffuse = mk3(0.0f, 0.0f, 0.0f) + dif * shadow, totalSpecular = mk3(0.0f, 0.0f, 0.0f);
                        if (bounce == 0) totalSpecular = totalSpecular + spec * shadow;
                        const f3 dsum = totalDiffuse + (bounce == 0 ? totalSpecular : mk3(0.0f, 0.0f, 0.0f));
                        if (dsum.x != 0.0f || dsum.y != 0.0f || dsum.z != 0.0f) {
                            const f3 term = mk3(th.x, th.y, th.z) * dsum;
                            const uint32_t smp = __float_as_uint(th.w);
                            float4 r = a.b.radiance[smp];
                            r.x = r.x + term.x; r.y = r.y + term.y; r.z = r.z + term.z;
                            a.b.radiance[smp] = r;
                            ++nRadiance;
                        }
                    }
                    return;
                }
                float4 h0 = a.b.sh0[e], h1 = a.b.sh1[e], h4 = a.b.sh4[e];
                f3 origin = mk3(h0.x, h0.y, h0.z), N = mk3(h1.x, h1.y, h1.z), T = mk3(h4.x, h4.y, h4.z);
                uint32_t smp = __float_as_uint(h0.w), n = __float_as_uint(h4.w);
                nSamples += n;
                f3 totalDiffuse = mk3(0.0f, 0.0f, 0.0f), totalSpecular = mk3(0.0f, 0.0f, 0.0f);
                // Variants that traverse themselves request the first sample's record together with the entry (one dependent round trip less:
                // single-light scenes -2 % shadow time). Not the resolve variant: it is held at 128 VGPRs and loses 3 % to the extra live
                // registers; requesting sample j + 1 while j is worked on costs every variant more than it hides.
                float4 ls0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (MODE != kShadowResolve && n) ls0 = a.b.shL[(size_t)e * a.maxLights];
                for (uint32_t j = 0; j < n; ++j) {
                    HRT_PHASE(PH_SHADOW_SAMPLE);
                    uint32_t vis = kVisCandidates;
                    if (MODE == kShadowResolve) {
                        // outcome of the opaque any-hit pass (wf_shadow_rays + wf_extend<ANYHIT>): most rays are settled there
                        vis = a.b.shVis[e * a.maxLights + j];
                        if (vis == kVisNoRay) continue;                                  // nee_direction said no
                        if (vis == kVisBlocked) { ++nRays; continue; }                   // shadow factor 0: contributes +0
                    }
                    float4 ls = ls0;
                    if (MODE == kShadowResolve || j) ls = a.b.shL[(size_t)e * a.maxLights + j];
                    HrptGPULight l = load_light(s, __float_as_uint(ls.z));
                    f3 L; float maxDist;
                    if (!nee_direction<DIRONLY>(l, N, origin, sunDir, cb.m_CosSunAngularRadius, ls.x, ls.y, L, maxDist)) continue;
                    float shadow;
                    HRT_PHASE(PH_SHADOW_QUERY);
                    if (MODE == kShadowResolve) {
                        if (vis == kVisClear) shadow = 1.0f;                             // no triangle at all in (tmin, tmax)
                        else {                                                           // the non-opaque triangles it crossed, nearest first
                            Ray sr = shadow_ray(origin, L, maxDist);
                            GlobalCandidates gc; gc.base = a.b.sqCand + (size_t)(e * a.maxLights + j) * kShadowCandidates;
                            const int cnt = (int)((vis >> 8) & 0xFFu); const bool ovf = (vis >> 16) & 1u;
                            if (LDS_BVH) shadow = shadow_resolve_candidates(s, lbvh, sr, make_shear(sr.d), cnt, ovf, gc, stack);
                            else shadow = shadow_resolve_candidates(s, gbvh, sr, make_shear(sr.d), cnt, ovf, gc, stack);
                        }
                    } else if (MODE == kShadowBuffered) {
                        // (no descent threshold here: without lane refill it only costs: config 2 shadow +3 %, config 4 +2.5 %)
                        if (LDS_BVH) shadow = shadow_query_buffered<kShadowCandidates>(s, lbvh, origin, L, maxDist, stack, cand);
                        else shadow = shadow_query_buffered<kShadowCandidates>(s, gbvh, origin, L, maxDist, stack, cand);
                    } else shadow = opaque_query(origin, L, maxDist);
                    ++nRays;
                    if (shadow != 0.0f) {   // an occluded sample contributes +0: its BRDF x radiance evaluation is skipped
                        HRT_PHASE(PH_SHADOW_CONTRIB);
                        float4 h2 = a.b.sh2[e], h3 = a.b.sh3[e];
                        f3 dif, spec;
                        nee_contribution<DIRONLY>(s, l, nee_lighting(N, mk3(h2.x, h2.y, h2.z), mk3(h3.x, h3.y, h3.z), h1.w, h2.w, h3.w), origin, sunDir,
                                                  sunIntensity, L, dif, spec);
                        totalDiffuse = totalDiffuse + dif * shadow;
                        if (bounce == 0) totalSpecular = totalSpecular + spec * shadow;
                    }
                }
                f3 dsum = totalDiffuse + (bounce == 0 ? totalSpecular : mk3(0.0f, 0.0f, 0.0f));
                if (dsum.x != 0.0f || dsum.y != 0.0f || dsum.z != 0.0f) {
                    f3 term = T * dsum;                                         // PathTracer.hlsl:261
                    float4 r = a.b.radiance[smp];
                    r.x = r.x + term.x; r.y = r.y + term.y; r.z = r.z + term.z;
                    a.b.radiance[smp] = r;
                    ++nRadiance;
                }
    };
    if (NONOPAQUE) {
        // Buffered variant (long, uneven entries): the wave hands out the entries of its segments (gw, gw + totalWaves, ...) as one
        // stream, an iteration whose segment runs out continues with the next one, so only the wave's last iteration is partly filled
        // (-4 % on configs 4 / 5). The short opaque any-hit variant below is faster with the plain per-segment loop (config 2).
        uint32_t seg = gw, cnt = 0, segBase = 0, next = 0; bool haveSeg = false;
        auto open_segment = [&]() {
            haveSeg = false; cnt = 0; next = 0;
            for (; seg < a.numSegments; seg += totalWaves) {
                cnt = uniform(a.b.shadowCnt[seg]);
                if (cnt) { segBase = seg * a.segSize; haveSeg = true; break; }
            }
        };
        open_segment();
        while (haveSeg) {
            uint32_t e = 0xFFFFFFFFu, filled = 0;
            while (filled < 64u && haveSeg) {
                uint32_t take = cnt - next < 64u - filled ? cnt - next : 64u - filled;
                if (lane >= filled && lane < filled + take) e = segBase + next + (lane - filled);
                next += take; filled += take;
                if (next >= cnt) { seg += totalWaves; open_segment(); }
            }
            if (e != 0xFFFFFFFFu) process(e);
        }
    } else {
        for (uint32_t seg = gw; seg < a.numSegments; seg += totalWaves) {
            const uint32_t cnt = uniform(a.b.shadowCnt[seg]), segBase = seg * a.segSize;
            for (uint32_t base = 0; base < cnt; base += 64) {
                uint32_t i = base + lane;
                if (i < cnt) process(segBase + i);
            }
        }
    }
    block_count_add(&a.counters->closestRays, 1, nRays);
    __syncthreads();
    block_count_add(&a.counters->closestRays, 4, nSamples);
    __syncthreads();
    block_count_add(&a.counters->closestRays, 6, nRadiance);
    if (SLIM && a.primary) { __syncthreads(); block_count_add(&a.counters->closestRays, 7, nSkipped16); }
}
