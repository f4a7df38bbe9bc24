// pt_wavefront_plan.h -- launch policy of the wavefront pipeline (pt_wavefront.hip): which kernel variant every stage runs, with how much LDS,
// on which grid, in which segment size. Values in, values out: no HIP call and no HIP header, so a plain C++17 compiler builds it
// (tests/test_wavefront_plan.py asserts the documented defaults that way, without a GPU).
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace hrt {

// Facts about the uploaded scene that select kernel variants / optional state streams.
struct SceneTraits {
    bool hasMedium = false;            // a thick (non-thin) transmissive material exists: interior IOR/sigma travel with the path
    bool hasStochasticAlpha = false;   // a non-transmissive BLEND material exists: TraceRayStandard draws RNG (RaytracingCommon.hlsli:181)
    bool hasTextures = false;          // some instanced material has m_TextureFlags != 0
    bool hasTransmissiveOrBlend = false;   // some instanced material takes the transmission branch (PathTracer.hlsl:149)
    bool directionalLightsOnly = true; // every GPULight is type 0
    bool hasNonOpaque = false;         // some instance is ForceNonOpaque (material alpha mode MASK or BLEND)
    uint32_t bvhMaxDepth = 0;
    uint32_t bvh4MaxDepth = 0;
    bool quantisedNodes = false;       // trees in global memory are walked through SceneView::nodesQ (64-byte nodes): chosen per scene at build time (pt_capi.cpp)
    uint32_t twoLevelStackNeed = 0;    // != 0: the scene holds the two-level structure (SceneView::instances); worst-case traversal stack entries
};

// What the plan reads of a SceneView.
struct TreeCounts {
    uint32_t nodeCount = 0, node4Count = 0, triCount = 0;
    bool hasNodesQ = false, hasInstances = false;      // SceneView::nodesQ / instances != nullptr
    uint32_t instanceCount = 0, materialCount = 0;     // records of SceneView::instShade / materials (0 = unknown: wf_shade reads its tables from global memory)
};

// Tuning knobs (0 = default): hrpt_create reads them from the environment, two have setters in the ABI.
struct WavefrontKnobs {
    uint32_t blocksPerCu = 0;
    uint32_t extendBlocksPerCu = 0;    // HRPT_WF_EXTEND_BLOCKS_PER_CU: grid of wf_extend alone (0 = automatic: 12 / 6 per CU for a tree in LDS / global memory)
    uint32_t refillMin = 0;            // wf_extend lane-refill threshold (1..64); 0 = default
    uint32_t segmentShift = 0;         // log2 of the segment size (6..10); 0 = automatic
    uint32_t segmentSize = 0;          // a segment size that is not a power of two (64..1024); 0 = from segmentShift
    bool drainSegments = false;        // wf_extend finishes every ray of a segment before it opens the next one (A/B knob)
    bool serialShadow = false;         // true: wf_shadow runs in stream order instead of concurrently with the next wf_extend
    uint32_t padLdsBytes = 0;          // experiment: extra dynamic LDS per trace block (lowers occupancy)
    uint32_t bvhWidth = 0;             // 2 or 4: node width the trace kernels traverse; 0 = default
    uint32_t nodeLoopMin = ~0u;        // HRPT_WF_NODE_LOOP_MIN: the descent loops end when fewer lanes than this are at inner nodes (~0 = automatic, 0 = never)
    bool noFusedPrimary = false;       // HRPT_WF_FUSED_PRIMARY=0: SIMPLE scenes keep the wf_raygen pass (A/B knob)
    bool noSlimShadow = false;         // HRPT_WF_SLIM_SHADOW=0: the SIMPLE shade variant writes full 96-byte shadow-queue entries (A/B knob)
    int shadeSort = -1;                // HRPT_WF_SHADE_SORT = 0 / 1: general wf_shade variants shade in queue order / grouped by shading class (-1: automatic)
    bool noFusedBounce0 = false;       // HRPT_WF_FUSED_BOUNCE0=0: bounce 0 keeps the wf_extend<PRIMARY> + wf_shade<PRIMARY> pair where wf_bounce0 would run (A/B knob)
    bool noShadeLdsTables = false;     // HRPT_WF_SHADE_LDS_TABLES=0: wf_shade gathers triangle / instance / material records from global memory even when they fit LDS (A/B knob)
    int shadowPath = 0;                // scenes with non-opaque geometry: 0 = automatic, 1 = wf_shadow traverses itself (buffered query), 2 = any-hit pass + resolve
    uint32_t radianceBatch = 0;        // HRPT_RADIANCE_BATCH: most rays hrpt_trace_radiance runs through the pipeline at once (0 = no cap of its own)
};

constexpr uint32_t kMaxSegment = 1024;       // largest wave-owned segment (samples); the size is chosen per batch, 64..1024
constexpr uint32_t kBlock = 256;             // 4 waves
constexpr uint32_t kMaxLights = 8;
constexpr size_t kLdsBudget = 64 * 1024;     // dynamic LDS per block: traversal stacks + BVH copy
// A 64-entry LDS stack is 64 KB per block, i.e. two blocks per CU: it cost 40 % on the scenes that needed it, although the worst case
// 3 * (depth4 + 1) that forces the size is never approached by real rays.
// Measured (MI355X): a 64-entry LDS stack -> 32 + spill: -33 % frame time on the 1.17 M-triangle scene; closest-hit kernel 32 -> 16 LDS
// entries + spill: another -3 % there and on config 4 (occupancy); the shadow kernel is faster with 32 (+4 % with 16 on configs 4, 5).
constexpr int kExtendLdsStack = 16, kShadowLdsStack = 32;
constexpr uint32_t kMaxStackNeed = 128;        // deepest supported 4-wide stack need (stack_entries4)
constexpr int kShadowCandidates = 8;           // non-opaque candidates a shadow ray buffers (LdsCandidates: two LDS columns each)
constexpr int kTwoLevelCandidates = 4;         // the same over the two-level structure (LdsCandidates3: three columns each)
constexpr size_t kCandidateLdsBytes = (size_t)kShadowCandidates * 2 * kBlock * 4;     // LdsCandidates of one block
// Stride of a 4-wide node in the LDS copy. At 128 bytes the rows of all even nodes start in the same four banks (and those of the odd nodes in four
// others): lanes at different nodes conflict 8-fold at worst. A multiple of 32 keeps the near ^ 16 = far addressing of inner_step.
#ifndef HRPT_LDS_NODE4_STRIDE
#define HRPT_LDS_NODE4_STRIDE 128
#endif
constexpr uint32_t kLdsNode4Stride = HRPT_LDS_NODE4_STRIDE;
static_assert(kLdsNode4Stride >= 128 && kLdsNode4Stride % 32 == 0, "LDS node stride: 128 bytes of node, near / far rows 32-byte aligned");
constexpr uint32_t kRefillMinDefault = 12;
// wf_shade
// The SIMPLE variant parks specular-lobe paths in a per-wave LDS ring of kShadeRing entries x kShadeRingFields floats.
constexpr uint32_t kShadeRing = 64, kShadeRingFields = 23;
constexpr size_t kShadeRingBytes = (size_t)(kBlock / 64) * kShadeRing * kShadeRingFields * 4;
// Every variant is compiled for kWavesShade = 4 waves per SIMD, i.e. four blocks per CU: of the CU's 160 KiB of LDS a block may take 40 KiB,
// static LDS (the statistics partials, 32 B) and the allocation granularity included -- 1 KiB is kept back for both.
constexpr uint32_t kShadeBlocksPerCu = 4;
constexpr size_t kCuLdsBytes = 160 * 1024, kShadeLdsMargin = 1024;
constexpr size_t kShadeLdsPerBlock = kCuLdsBytes / kShadeBlocksPerCu - kShadeLdsMargin;     // dynamic LDS a wf_shade block may ask for
// Records of the three tables the shading path gathers from (pt_scene_records.h GpuTriAttr, GpuInstShade; hobbyrt_pt.h HrptMaterialConstants;
// pt_wavefront.hip asserts the sizes). wf_shade_lt copies them whole, in their global layout, behind the ring.
constexpr size_t kTriAttrBytes = 80, kInstShadeBytes = 48, kMaterialBytes = 180;
constexpr size_t shade_table_bytes(uint32_t triCount, uint32_t instanceCount, uint32_t materialCount)
{
    const size_t b = (size_t)triCount * kTriAttrBytes + (size_t)instanceCount * kInstShadeBytes + (size_t)materialCount * kMaterialBytes;
    return (b + 15) & ~(size_t)15;
}
// wf_bounce0: trace and shade of bounce 0 in one kernel, at wf_shade's four blocks per CU. Its block holds what both halves hold -- traversal
// stack, specular ring, shading tables, tree copy, in this order -- so the ring is halved to 32 entries per wave (with 64 the Cornell-class block
// is 23.5 + 5.3 + 16 + 3.5 KB: too much). The tables are padded to 128 bytes: the tree copy behind them must start 128-byte aligned (setup_lds).
constexpr uint32_t kBounce0Ring = 32;
constexpr size_t kBounce0RingBytes = (size_t)(kBlock / 64) * kBounce0Ring * kShadeRingFields * 4;
static_assert(kBounce0RingBytes % 128 == 0, "the tree copy behind ring and tables starts 128-byte aligned");
constexpr size_t bounce0_shade_bytes(size_t tableBytes) { return kBounce0RingBytes + ((tableBytes + 127) & ~(size_t)127); }     // between stack and tree
// wf_shadow
// MODE kShadowOpaque: no ForceNonOpaque instance in the scene: plain any-hit query per light sample.
// MODE kShadowBuffered: non-opaque geometry, the kernel traverses itself: per-lane candidate buffer in LDS (after the stack) and the buffered query.
// MODE kShadowResolve: non-opaque geometry, visibility traversal already done by wf_shadow_rays + wf_extend<ANYHIT>: this kernel only walks
//   the recorded candidate lists (its stack serves the rare re-trace behind an overflowing list) and evaluates the contributions.
// MODE kShadowSlim: kShadowOpaque with directional lights only and the 32-byte entries of wf_shade<1, SIMPLE> (see there).
enum : int { kShadowOpaque = 0, kShadowBuffered = 1, kShadowResolve = 2, kShadowSlim = 3 };

// One instantiation of a traversal kernel family and the dynamic LDS it is launched with (without the candidate columns some modes add: see the
// launch_* functions of pt_wavefront.hip).
// stack need classes: BVH2 8/16/32/64 (maxDepth + 2), BVH4 16/32/64 (stack_entries4); class 64 = "deeper than the LDS part": the kernel keeps
// kExtendLdsStack / kShadowLdsStack entries in LDS and the rest in the overflow columns (LdsStack)
struct Variant { bool lds = false; int depth = 0, width = 0; size_t ldsBytes = 0; bool twoLevel = false; bool twoLevelCandidates = false; bool quantised = false; };

// Entries the 4-wide traversal can hold at once: inner_step (pt_traverse.h) pushes up to three siblings at every inner node it visits, and the path to
// the deepest inner node (depth4, the root being 0) visits depth4 + 1 of them. (3 * depth4 + 2 stood here before: one entry short on a ray that
// finds all four children of every node on the deepest path, where the LDS stack wraps and the overflow column is written one row past its end.)
inline uint32_t stack_entries4(uint32_t depth4) { return 3 * depth4 + 3; }
inline uint32_t stack_need4(const SceneTraits& traits) { return traits.twoLevelStackNeed ? traits.twoLevelStackNeed : stack_entries4(traits.bvh4MaxDepth); }

// The variant of one kernel class: `width` asked for, `extraBytes` of LDS the kernel takes besides stack and tree (they count against the
// budget, the launch adds them), `ldsStackMax` stack entries that kernel class keeps in LDS, `padBytes` added to the launch only.
inline Variant pick_variant(const SceneTraits& traits, const TreeCounts& tree, int width, size_t extraBytes, int ldsStackMax, size_t padBytes)
{
    Variant v; v.width = width;
    uint32_t need = traits.twoLevelStackNeed;
    if (need) { v.width = 4; v.twoLevel = true; v.twoLevelCandidates = traits.hasNonOpaque; }     // two-level structure: 4-wide trees in global memory, its own kernels
    else {
        if (v.width == 4 && stack_entries4(traits.bvh4MaxDepth) > kMaxStackNeed) v.width = 2;
        need = v.width == 2 ? traits.bvhMaxDepth + 2 : stack_entries4(traits.bvh4MaxDepth);
    }
    v.depth = (v.width == 2 && need <= 8) ? 8 : (need <= 16 ? 16 : (need <= 32 ? 32 : 64));
    const size_t bvhBytes = v.twoLevel ? 0 : (v.width == 2 ? (size_t)tree.nodeCount * 64 : (size_t)tree.node4Count * kLdsNode4Stride) + (size_t)tree.triCount * 48;
    const size_t stackBytes = (size_t)(v.depth > ldsStackMax ? ldsStackMax : v.depth) * kBlock * 4;
    v.lds = bvhBytes > 0 && stackBytes + extraBytes + bvhBytes <= kLdsBudget;
    v.ldsBytes = stackBytes + (v.lds ? bvhBytes : 0) + padBytes;
    v.quantised = v.width == 4 && !v.lds && !v.twoLevel && traits.quantisedNodes && tree.hasNodesQ;
    return v;
}

// What one wavefront_render decides before it allocates or launches anything.
struct RenderPlan {
    Variant vE, vS, vA;                // closest hits (wf_extend), wf_shadow, the any-hit pass of the resolve schedule (wf_extend<ANYHIT>)
    int shadowMode = kShadowOpaque;
    bool slim = false;                 // slim shadow-queue entries (shadowMode == kShadowSlim)
    bool simpleScene = false;          // wf_shade<1, SIMPLE>
    bool fusedPrimary = false;         // no wf_raygen pass: bounce 0 runs wf_extend<PRIMARY> / wf_shade<PRIMARY> (every batch of the render alike)
    uint32_t sortShade = 0, nodeLoopMin = 0;
    uint32_t maxLights = 1, cus = 0, blocksPerCu = 0, extendBlocksPerCu = 0;
    uint32_t spillEntries = 0; size_t spillThreads = 0;    // stack-overflow entries per thread (0 = none) in two columns (wf_extend, wf_shadow) of so many threads each
    uint32_t pathRecordBytes = 48; uint64_t bytesPerSample = 0;    // of the queue pool
    bool shadeLdsTables = false;       // wf_shade_lt: triangle, instance and material records are served from a per-block LDS copy
    size_t shadeTableBytes = 0;        // ... which takes so many bytes (0 when the tables stay in global memory)
    size_t shadeLdsBytes = 0;          // dynamic LDS of the SIMPLE shade launches: the ring + shadeTableBytes (the general variants size their sort tables per batch)
    bool fusedBounce0 = false;         // bounce 0 runs wf_bounce0 instead of wf_extend<PRIMARY> + wf_shade_lt<PRIMARY>
    size_t bounce0LdsBytes = 0;        // ... launched with so much dynamic LDS: vE's stack and tree + the 32-entry ring + the padded tables (0 when off)
};
struct BatchPlan { uint32_t segSize, numSegments, grid, gridExtend; };

inline RenderPlan plan_render(const SceneTraits& traits, const TreeCounts& tree, uint32_t lightCount, uint32_t cus, const WavefrontKnobs& k)
{
    RenderPlan p;
    const uint32_t maxLights = lightCount ? lightCount : 1;
    p.maxLights = maxLights; p.cus = cus;
    // the pool takes 240 B per sample with one light and no medium, but ~1.2 KB with 8 lights and non-opaque geometry (shadow-ray queue + candidate lists)
    p.bytesPerSample = 16ull * (2 * (3 + (traits.hasMedium ? 2 : 0)) + 1 + 5 + maxLights + 1) + (tree.hasInstances ? 4 : 0) +
                       ((traits.hasNonOpaque || maxLights > 1) ? (16ull + 16 + 4 + 4 + 8 * kShadowCandidates) * maxLights : 0);
    p.pathRecordBytes = traits.hasMedium ? 80u : 48u;
    // default: on for scenes that sample textures (the longest branch of shade_surface_a; Sponza-class config: same shade time, -15 % VALU
    // instructions), off otherwise (glass config: the sort costs 3.5 % of wf_shade, its classes are too few per segment to fill iterations)
    p.sortShade = k.shadeSort < 0 ? (traits.hasTextures ? 1u : 0u) : (uint32_t)k.shadeSort;
    // Node width per kernel class (measured, scripts/gpu_bvh4_ab.sh): the 4-wide tree wins for closest-hit queries everywhere
    // (fewer, fuller steps: -9..-11% extend time on configs 2/4/5) and for shadow queries that buffer non-opaque candidates or
    // read the BVH from global memory (-9..-14%); the small opaque any-hit kernel over an LDS-resident BVH is faster 2-wide
    // (the 4-wide step costs it 12 VGPRs = one wave of occupancy).
    const size_t candBytes = traits.hasNonOpaque ? kCandidateLdsBytes : 0;
    auto pick = [&](int width, size_t extraBytes, int ldsStackMax) { return pick_variant(traits, tree, width, extraBytes, ldsStackMax, k.padLdsBytes); };
    const int forced = k.bvhWidth == 2 ? 2 : (k.bvhWidth == 4 ? 4 : 0);
    p.vE = pick(forced ? forced : 4, 0, kExtendLdsStack);
    p.vS = pick(forced ? forced : 4, candBytes, kShadowLdsStack);
    if (!forced && p.vS.lds && !traits.hasNonOpaque) p.vS = pick(2, candBytes, kShadowLdsStack);
    // Shadow-ray schedule. Several lights per vertex, or glass (rays that cross many non-opaque triangles), make the per-ray cost very
    // uneven; when the tree is in global memory their visibility traversal runs in the refilling traversal kernel (wf_shadow_rays +
    // wf_extend<ANYHIT>, which also records the crossed non-opaque triangles) and wf_shadow only resolves: glass config 4.7 -> 4.2 ms per
    // bounce, an opaque 101 k-triangle scene with three lights 20.3 -> 18.4 ms per frame. With an LDS-resident tree the traversal is too
    // cheap to pay for the extra passes (Cornell box with three lights 11.3 vs 13.1 ms), and a single sun over alpha-tested foliage
    // (config 4) is faster with wf_shadow's own buffered query (0.96 vs 1.07 ms per bounce). HRPT_WF_SHADOW_PATH = 1 / 2 forces either.
    const bool manyLights = maxLights > 1;
    const bool unevenRays = manyLights || (traits.hasNonOpaque && traits.hasTransmissiveOrBlend);
    const int selfMode = traits.hasNonOpaque ? kShadowBuffered : kShadowOpaque;
    p.shadowMode = (!p.vS.lds && unevenRays) ? kShadowResolve : selfMode;
    if (k.shadowPath == 1) p.shadowMode = selfMode;
    if (k.shadowPath == 2 && (traits.hasNonOpaque || manyLights)) p.shadowMode = kShadowResolve;
    // two-level scenes: wf_shadow traverses itself (no any-hit pass over that structure); TL = 1 instantiations when every instance is opaque, TL = 2
    // (buffered candidates of non-opaque instances, shadow_query_two_level_buffered) otherwise -- launch_shadow picks by Variant::twoLevelCandidates
    if (traits.twoLevelStackNeed) p.shadowMode = kShadowOpaque;
    // any-hit pass over the shadow rays (same kernel family as vE). wf_extend<ANYHIT> always carves its candidate columns out of LDS
    // (launch_extend adds them to the launch), opaque scene or not, so the budget check must count them too.
    p.vA = pick(forced ? forced : 4, kCandidateLdsBytes, kExtendLdsStack);
    if (p.shadowMode == kShadowResolve) p.vS = pick(forced ? forced : 4, 0, kExtendLdsStack);
    p.simpleScene = !traits.hasTextures && !traits.hasTransmissiveOrBlend && traits.directionalLightsOnly;
    // slim shadow-queue entries: the SIMPLE single-light shade variant feeding the plain opaque any-hit query (HRPT_WF_SLIM_SHADOW=0 keeps the 96-byte entries)
    p.slim = p.simpleScene && !manyLights && p.shadowMode == kShadowOpaque && !k.noSlimShadow;
    if (p.slim) p.shadowMode = kShadowSlim;
    // Thresholded while-while (measured, scripts/env_sweep.sh HRPT_WF_NODE_LOOP_MIN): 16 lanes for an LDS-resident tree (config 2 extend -3 %),
    // 24 for a tree in global memory (config 4 extend -11 %, glass config extend -24 % and its any-hit pass -14 %)
    p.nodeLoopMin = k.nodeLoopMin != ~0u ? k.nodeLoopMin : (p.vE.lds ? 16u : 24u);
    // more blocks than fit: the dispatcher back-fills CUs as blocks retire (scripts/knob_sweep.py). A context that is one lane of a
    // two-frames-in-flight loop (hrpt_set_shadow_overlap(ctx, 0)) and traverses a tree in global memory does better with half the grid:
    // its latency-bound kernels leave room for the other lane's (config 4 14.4 -> 14.0 ms, config 5 22.6 -> 21.9 ms per frame).
    p.blocksPerCu = k.blocksPerCu ? k.blocksPerCu : ((k.serialShadow && !p.vE.lds) ? 8 : 16);
    // wf_extend gets a grid of its own: a whole number of rounds of the six blocks a CU holds of it. Measured (scripts/env_sweep.sh
    // HRPT_WF_EXTEND_BLOCKS_PER_CU): tree in LDS 12 per CU (two rounds; 16 = 2.67 rounds: +8 % on config 2, the last round runs with four of six
    // slots filled), tree in global memory 6 (one persistent round: its waves are latency-bound and every further round re-pays the ramp:
    // config 4 extend -6 %, glass config -20 %; the two-level kernels hold five blocks per CU and launch_rounds trims the six to that: -6 / -10 %
    // on instanced scenes of opaque / non-opaque materials).
    p.extendBlocksPerCu = k.extendBlocksPerCu ? k.extendBlocksPerCu : (k.blocksPerCu ? k.blocksPerCu : (p.vE.lds ? 12u : 6u));
    if (p.vE.depth > kExtendLdsStack || p.vS.depth > kShadowLdsStack) {
        // stack overflow columns for trees whose worst-case stack need exceeds the LDS entries (see LdsStack); sized for the smaller LDS part
        const uint32_t worst = traits.twoLevelStackNeed ? traits.twoLevelStackNeed : (p.vE.width == 4 || p.vS.width == 4 ? stack_entries4(traits.bvh4MaxDepth) : traits.bvhMaxDepth + 2);
        p.spillEntries = worst > (uint32_t)kExtendLdsStack ? worst - kExtendLdsStack : 1u;
        p.spillThreads = (size_t)cus * (p.blocksPerCu > p.extendBlocksPerCu ? p.blocksPerCu : p.extendBlocksPerCu) * kBlock;
    }
    // SIMPLE scenes: no raygen pass. wf_extend<PRIMARY> (the bounce-0 launch) derives the primary ray and the RNG seed of a slot (= sample index) from
    // PrimaryArgs in its refill and leaves {direction, seed} in rayD for wf_shade<PRIMARY> / wf_shadow, which take the camera position as origin and
    // (1, 1, 1) as throughput; wf_shade(0) stores the first radiance term instead of adding to a zeroed array; padding pixels of the 8 x 8 tiles get
    // a kNoPathRecord hit record. 96 B per sample less queue traffic and one launch less: config 2 -3 % one frame at a time, -4 % two in flight
    // (HRPT_WF_FUSED_PRIMARY=0 keeps wf_raygen). As run-time branches inside the ordinary kernels the same code cost every bounce 6 % (extend) and
    // 16 % (shade): the extra live values; and regenerating the ray in wf_shade instead of reading 16 bytes gave the saving back in instructions.
    // wf_shade's table gathers. Per 64-lane iteration the kernel issues 13 per-lane reads into three read-only tables of a few KB, and a CU's
    // L1 serves about one lane-request per cycle whatever the width (profiles/r03_gather_nodes_microbench.txt): copied to LDS at block start (every
    // launch, so hrpt_update_materials / hrpt_update_instances need no bookkeeping) they are ds_reads. Only where the copy still lets a CU hold its
    // four blocks; only the SIMPLE single-light variants have the LDS instantiation; two-level scenes (per-mesh records, instance from the hit)
    // and scenes whose counts are unknown keep the global tables. HRPT_WF_SHADE_LDS_TABLES=0 forces the global tables.
    p.shadeLdsBytes = kShadeRingBytes;
    if (p.simpleScene && !manyLights && !k.noShadeLdsTables && !tree.hasInstances && !traits.twoLevelStackNeed &&
        tree.triCount && tree.instanceCount && tree.materialCount) {
        const size_t tables = shade_table_bytes(tree.triCount, tree.instanceCount, tree.materialCount);
        if (kShadeRingBytes + tables <= kShadeLdsPerBlock) { p.shadeLdsTables = true; p.shadeTableBytes = tables; p.shadeLdsBytes = kShadeRingBytes + tables; }
    }
    p.fusedPrimary = p.simpleScene && !manyLights && maxLights <= kMaxLights && p.vE.width == 4 && !traits.hasMedium && !traits.hasStochasticAlpha && !k.noFusedPrimary;
    // Bounce 0 in one kernel (wf_bounce0). Primary rays are coherent (lane utilisation 0.91 / 0.92 in the two kernels against 0.60 / 0.74 at the
    // other bounces), yet the pair hands every sample's hit and {direction, seed} record through HBM. Where the bounce-0 pair is
    // wf_extend<LDS, OPQ, PRIMARY> + wf_shade_lt<1, SIMPLE, PRIMARY> -- tree and tables in LDS, every instance opaque, one light -- and one block
    // can hold the LDS of both, a wave traces 64 primary rays to completion and shades them from registers. HRPT_WF_FUSED_BOUNCE0=0 keeps the pair.
    if (p.fusedPrimary && p.shadeLdsTables && p.vE.lds && p.vE.width == 4 && !traits.hasNonOpaque && !manyLights && !k.noFusedBounce0) {
        const size_t bytes = p.vE.ldsBytes + bounce0_shade_bytes(p.shadeTableBytes);
        if (bytes <= kShadeLdsPerBlock) { p.fusedBounce0 = true; p.bounce0LdsBytes = bytes; }
    }
    return p;
}

// Segments and grids of one batch of `numSamples` samples (padded pixels x accumulation indices).
inline BatchPlan plan_batch(const RenderPlan& p, const WavefrontKnobs& k, uint32_t numSamples)
{
    BatchPlan b;
    // segment size: large segments amortise the partially filled last 64-lane iteration of every segment (after compaction a
    // segment holds ~80 % / 65 % / 53 % of its slots at bounces 1 / 2 / 3), small ones give every SIMD several waves when the batch is
    // small (tile-sharded multi-GPU runs) and balance uneven per-entry work (several lights per shadow entry). Measured on MI355X
    // (scripts/sweep_env.sh, scripts/seg_sweep.py): 512 wins for full-frame single-light batches (-3 % config 2, -4 % config 4),
    // 256 for a 135-row band (0.76 vs 0.89 ms) and for the three-light glass scene.
    // (512 only with an LDS-resident tree: rays through a big tree in global memory differ too much in length -- 256 is 2..4 % faster
    // there: config 4 14.4 -> 14.2 ms, 1.17 M triangles 20.1 -> 19.4 ms)
    const bool largeBatch = numSamples >= (8u << 20) && p.maxLights == 1 && p.vE.lds;
    uint32_t shift = k.segmentShift ? k.segmentShift : (largeBatch ? 9u : 8u);
    if (shift < 6) shift = 6;
    if (shift > 10) shift = 10;
    b.segSize = 1u << shift;
    if (k.segmentSize >= 64u && k.segmentSize <= kMaxSegment) b.segSize = k.segmentSize;       // HRPT_WF_SEGMENT_SIZE: any size (experiments)
    b.numSegments = (numSamples + b.segSize - 1) / b.segSize;
    const uint32_t wavesNeeded = b.numSegments, blocksNeeded = (wavesNeeded + 3) / 4;
    b.grid = p.cus * p.blocksPerCu; if (b.grid > blocksNeeded) b.grid = blocksNeeded; if (b.grid == 0) b.grid = 1;
    b.gridExtend = p.cus * p.extendBlocksPerCu; if (b.gridExtend > blocksNeeded) b.gridExtend = blocksNeeded; if (b.gridExtend == 0) b.gridExtend = 1;
    return b;
}

// hrpt_render_gbuffer (wavefront path): bounce 0 of a one-sample-per-pixel batch through the render's own front end -- wf_raygen and the
// closest-hit kernel plan_render / plan_batch pick for this scene (a single light slot: the lights are not read) -- followed by wf_gbuffer on
// the shade grid. Nothing is chosen here that a render does not choose: same variant, same LDS bytes, same segments, same grids.
struct GBufferPlan {
    Variant vE; BatchPlan batch;
    uint32_t nodeLoopMin = 0, pathRecordBytes = 48;
    uint32_t spillEntries = 0; size_t spillThreads = 0;
    uint64_t bytesPerSample = 0;       // of the queue pool: path record + hit record (+ instance) + the radiance slot wf_raygen zeroes
};
inline GBufferPlan plan_gbuffer(const SceneTraits& traits, const TreeCounts& tree, uint32_t cus, const WavefrontKnobs& k, uint32_t numSamples)
{
    const RenderPlan p = plan_render(traits, tree, 1, cus, k);
    GBufferPlan g;
    g.vE = p.vE; g.batch = plan_batch(p, k, numSamples);
    g.nodeLoopMin = p.nodeLoopMin; g.pathRecordBytes = p.pathRecordBytes;
    g.spillEntries = p.spillEntries; g.spillThreads = p.spillThreads;
    g.bytesPerSample = p.pathRecordBytes + 16u + (tree.hasInstances ? 4u : 0u) + 16u;
    return g;
}

// hrpt_trace_radiance (wavefront path): the render's pipeline between wf_raygen_rays and wf_store_radiance over a caller's rays. The plan is the
// render's for these traits and lights -- kernel variants, shadow mode, slim queue, LDS shade tables, class sort, grids -- with the two bounce-0
// forms off that derive their rays from the sample index (fusedPrimary, and fusedBounce0 which needs it): the rays are in the path queue.
inline RenderPlan plan_radiance(const SceneTraits& traits, const TreeCounts& tree, uint32_t lightCount, uint32_t cus, WavefrontKnobs k)
{
    k.noFusedPrimary = true;
    return plan_render(traits, tree, lightCount, cus, k);
}
// Rays per batch: at most 64 Mi, what `budgetBytes` of queue pool hold (0 = no such limit), what keeps the 32-bit (entry, light) slot ids in
// range and HRPT_RADIANCE_BATCH; never below one ray. The batch's pool is laid out for radiance_capacity samples: whole kMaxSegment segments.
constexpr uint64_t kMaxRadianceBatch = 64ull << 20;
inline uint64_t radiance_batch_rays(uint64_t count, const RenderPlan& p, uint64_t budgetBytes, const WavefrontKnobs& k)
{
    uint64_t n = kMaxRadianceBatch;
    if (budgetBytes && budgetBytes / p.bytesPerSample < n) n = budgetBytes / p.bytesPerSample;
    if (n * p.maxLights > 0xFFFFFFFFull) n = 0xFFFFFFFFull / p.maxLights;
    if (k.radianceBatch && k.radianceBatch < n) n = k.radianceBatch;
    if (count < n) n = count;
    return n ? n : 1;
}
inline uint64_t radiance_capacity(uint64_t batchRays) { return (batchRays + kMaxSegment - 1) / kMaxSegment * kMaxSegment; }

// hrpt_trace_rays over device arrays through the persistent refilling traversal kernel (wf_trace_rays): the closest-hit kernel class of the
// render path (4-wide, kExtendLdsStack), with these differences: HRPT_WF_BVH_WIDTH and HRPT_WF_PAD_LDS do not apply, and there is no 2-wide
// kernel to fall back to: wavefront_trace_rays_supported is false when the tree is too deep for it, and the caller asks before it plans.
struct TraceRaysPlan {
    Variant v;
    uint32_t grid = 0, refillMin = 0, nodeLoopMin = 0;
    uint32_t spillEntries = 0; size_t spillThreads = 0;    // stack-overflow entries per thread (0 = none), threads
};
inline bool wavefront_trace_rays_supported(const SceneTraits& traits) { return stack_need4(traits) <= kMaxStackNeed; }
inline TraceRaysPlan plan_trace_rays(const SceneTraits& traits, const TreeCounts& tree, uint64_t count, bool shadow, uint32_t cus, const WavefrontKnobs& k)
{
    TraceRaysPlan p;
    p.v = pick_variant(traits, tree, 4, shadow ? kCandidateLdsBytes : 0, kExtendLdsStack, 0);
    const uint32_t blocksPerCu = k.blocksPerCu ? k.blocksPerCu : 16;
    const uint64_t chunks = (count + 255) / 256, blocksNeeded = (chunks + 3) / 4;
    p.grid = cus * blocksPerCu; if (p.grid > blocksNeeded) p.grid = (uint32_t)blocksNeeded;
    p.refillMin = k.refillMin ? k.refillMin : kRefillMinDefault;
    p.nodeLoopMin = k.nodeLoopMin != ~0u ? k.nodeLoopMin : (p.v.lds ? 16u : 24u);
    if (p.v.depth > kExtendLdsStack) {
        const uint32_t need = stack_need4(traits);
        p.spillEntries = need > (uint32_t)kExtendLdsStack ? need - kExtendLdsStack : 1u;
        p.spillThreads = (size_t)cus * blocksPerCu * kBlock;
    }
    return p;
}

} // namespace hrt
