// pt_wf_common.h -- what every wavefront kernel shares: the queue pool's streams (WfBuffers) and the per-launch arguments (WfArgs, PrimaryArgs,
// JitterTable), the sample -> tile -> pixel enumeration and the primary ray, the per-lane LDS traversal stack and candidate columns, the tree
// view in LDS (LdsBvh) with the block-start LDS copy (setup_lds), the wave helpers (lane_id, uniform, prefix_rank) and the
// per-block statistics adds. A piece of pt_wavefront.hip, which includes it inside hrt's anonymous namespace after pt_path.h: no stand-alone header.

constexpr uint32_t kMaxSppPerBatch = 64;

struct WfBuffers {
    float4 *rayO[2], *rayD[2], *thr[2], *med0[2], *med1[2];
    uint32_t* pathCnt[2];
    float4* hit;
    uint32_t* hitInst;         // two-level structure only: CommittedInstanceIndex of the hit in `hit` (the record's triangle index is per mesh)
    float4 *sh0, *sh1, *sh2, *sh3, *sh4, *shL;
    uint32_t* shadowCnt;
    // shadow-ray stage of scenes with non-opaque geometry: one compacted ray per valid light sample {o, tmin} {d, tmax}, the (entry, light)
    // slot it belongs to, rays per segment, and the outcome of the opaque any-hit pass per (entry, light) slot (kVis*)
    float4 *sqO, *sqD; uint32_t* sqId; uint32_t* sqCnt; uint32_t* shVis;
    uint2* sqCand;             // kShadowCandidates (t, triangle) keys per (entry, light) slot: the non-opaque triangles a ray crossed, nearest first
    float4* radiance;
};

struct WfArgs {
    SceneView scene;
    WfBuffers b;
    uint32_t segSize;          // samples per segment (any size from 64 to kMaxSegment: chosen per batch so that the segments divide evenly among the waves of the grids)
    uint32_t numSegments;      // segments in this batch
    uint32_t numSamples;       // tilesX*tilesY*64*spp (padded to 8x8 pixel tiles)
    uint32_t pixelsPadded;     // tilesX*tilesY*64
    uint32_t tilesX, tilesY;
    TileRect rect;
    uint32_t imageWidth;
    uint32_t spp;              // accumulation indices in this batch
    uint32_t maxLights;        // per-path light-sample slots in the shadow queue
    uint32_t hasMedium;        // scene has thick transmissive materials (medium state travels with the path)
    uint32_t hasStochasticAlpha;
    uint32_t allOpaque;        // no ForceNonOpaque instance in the scene: closest-hit launches take the OPQ instantiations of wf_extend
    uint32_t refillMin;        // wf_extend refills its idle lanes once at least this many have finished their ray
    uint32_t streamSegments;   // wf_extend moves on to its next segment while rays of the previous one are still in flight
    uint32_t slimShadow;       // slim shadow-queue entries (scenes of the SIMPLE shade variant with one light): sh0{origin, input slot} sh1{N, material}
    uint32_t shadowParity;     // ... and the path queue those slots index (the input queue of the bounce's wf_shade)
    uint32_t nodeLoopMin;      // wf_extend leaves its node-descent loop once fewer lanes than this are still at inner nodes (0: never)
    uint32_t sortShade;        // wf_shade (general variants) shades the entries of a segment grouped by shading class
    uint32_t shadeInstances, shadeMaterials;   // wf_shade_lt: records of scene.instShade / scene.materials it copies to LDS (with scene.triCount records of scene.attrs)
    const struct PrimaryArgs* primaryArgs;     // device copy (queue pool), valid when `primary`
    uint32_t primary;          // this launch works on bounce 0 of a batch whose primary rays are NOT in the path queue: slot == sample index, every
                               // wf_extend<PRIMARY> derives the ray of a slot from PrimaryArgs and leaves {direction, RNG seed} in rayD; origin = camera, throughput (1,1,1)
                               // (no wf_raygen launch; SIMPLE scenes)
    int32_t* spill[2];         // per-lane stack overflow columns of wf_extend / wf_shadow (they run concurrently), element k of thread g at [k * threads + g]
    DeviceCounters* counters;
};

enum : uint32_t { kVisNoRay = 0, kVisBlocked = 1, kVisClear = 2, kVisCandidates = 3 };   // shVis codes

struct JitterTable { float2 j[kMaxSppPerBatch]; };
// what the primary ray of a sample is computed from (PathTracer.hlsl:61-72, PathTracerRenderer.cpp:62-65); by value to the bounce-0 launches
struct PrimaryArgs { float clipToWorld[16]; float cam[3]; float invW, invH; uint32_t accumIndex; float2 j[kMaxSppPerBatch]; };

// Tile enumeration: row-major over the rectangle; with interleaved columns (stripeCount > 1) column-major, so that the consecutive tiles
// of a segment stay neighbours in the image (8 pixels apart vertically instead of 8 * stripeCount horizontally: -3 % per rank at 8 ranks).
HRT_DEV void tile_position(const WfArgs& a, uint32_t tile, uint32_t& tcol, uint32_t& trow)
{
    if (a.rect.stripeCount > 1u) { tcol = tile / a.tilesY; trow = tile - tcol * a.tilesY; }
    else { trow = tile / a.tilesX; tcol = tile - trow * a.tilesX; }
}

// Pixel and primary ray of sample `smp` of the batch (the body of wf_raygen; with a.primary the bounce-0 kernels call it instead of reading the
// path queue). false: the sample's pixel lies outside the rectangle (tiles are padded to 8 x 8).
HRT_DEV bool primary_ray(const WfArgs& a, const PrimaryArgs& pr, uint32_t smp, f3& o, f3& d, uint32_t& rng)
{
    const uint32_t k = smp / a.pixelsPadded, p = smp - k * a.pixelsPadded;
    const uint32_t tile = p >> 6, within = p & 63u;
    uint32_t tcol, trow; tile_position(a, tile, tcol, trow);
    const uint32_t px = a.rect.column_x(tcol) + (within & 7u), py = a.rect.y0 + trow * 8u + (within >> 3);
    if (!(px < a.rect.x1 && py < a.rect.y1)) return false;
    // a deliberate copy of camera_ray's body (pt_direct.h) with the jitter / RNG stream of accumulation index
    // first + k (PathTracerRenderer.cpp:62,:65)
    const float u = (((float)px + 0.5f) + pr.j[k].x) * pr.invW;
    const float v = (((float)py + 0.5f) + pr.j[k].y) * pr.invH;
    const float cx = u * 2.0f + -1.0f, cy = v * -2.0f + 1.0f;
    const float* M = pr.clipToWorld;
    const float ex = ((cx * M[0] + cy * M[4]) + 0.9f * M[8]) + 1.0f * M[12];
    const float ey = ((cx * M[1] + cy * M[5]) + 0.9f * M[9]) + 1.0f * M[13];
    const float ez = ((cx * M[2] + cy * M[6]) + 0.9f * M[10]) + 1.0f * M[14];
    const float ew = ((cx * M[3] + cy * M[7]) + 0.9f * M[11]) + 1.0f * M[15];
    const f3 end = mk3(ex / ew, ey / ew, ez / ew);
    o = mk3(pr.cam[0], pr.cam[1], pr.cam[2]);
    d = normalize(end - o);
    rng = hrt_rng_seed(px, py, pr.accumIndex + k);
    return true;
}
// entries of segment `seg` of the input path queue: counted by the producing kernel, or -- bounce 0 without a raygen pass -- every slot of the batch
HRT_DEV uint32_t path_count(const WfArgs& a, uint32_t in, uint32_t seg)
{
    (void)in;
    const uint32_t base = seg * a.segSize, left = a.numSamples - base, size = a.segSize; return left < size ? left : size;
}

// per-lane traversal stack in LDS: element (sp, lane-in-block) at base[sp * kBlock]
// DEPTH 64 = "deeper than 32": the first 32 entries stay in LDS, the (rarely reached) rest lives in a per-lane column of global memory.
template <int DEPTH, int LDSMAX>
struct LdsStack {
    static constexpr int kLdsStackMax = LDSMAX;
    static constexpr int kLds = DEPTH > kLdsStackMax ? kLdsStackMax : DEPTH;
    static constexpr int kRows = kLds;
    int32_t* base; int32_t* spill; uint32_t spillStride;
    HRT_DEV void push(int sp, int32_t v)
    {
        if (DEPTH <= kLdsStackMax || sp < kLds) base[(sp & (kLds - 1)) * kBlock] = v;
        else spill[(size_t)(sp - kLds) * spillStride] = v;
    }
    HRT_DEV int32_t pop(int sp)
    {
        if (DEPTH <= kLdsStackMax || sp < kLds) return base[(sp & (kLds - 1)) * kBlock];
        return spill[(size_t)(sp - kLds) * spillStride];
    }
};
// per-lane buffer of the K closest non-opaque shadow candidates: (t, triangle) of entry k at base[(k*2 + {0,1}) * kBlock];
// the barycentrics are recomputed from the triangle when the candidate is processed (same test => same bits).
// One interface for the three buffers (pt_shadow.h candidate_insert / shadow_resolve_candidates): key and set carry an instance, which the
// two-column buffers neither store nor yield -- the triangle record of a flat tree names it.
struct LdsCandidates {
    int32_t* base;
    HRT_DEV void key(int k, float& t, uint32_t& tri) const { t = __int_as_float(base[(k * 2 + 0) * kBlock]); tri = (uint32_t)base[(k * 2 + 1) * kBlock]; }
    HRT_DEV void key(int k, float& t, uint32_t& tri, uint32_t&) const { key(k, t, tri); }
    HRT_DEV void set(int k, float t, uint32_t tri, uint32_t) { base[(k * 2 + 0) * kBlock] = __float_as_int(t); base[(k * 2 + 1) * kBlock] = (int32_t)tri; }
    HRT_DEV void move(int dst, int src) { base[(dst * 2 + 0) * kBlock] = base[(src * 2 + 0) * kBlock]; base[(dst * 2 + 1) * kBlock] = base[(src * 2 + 1) * kBlock]; }
};
// ... with the instance next to the triangle (two-level structure: the triangle index is per mesh): entry k at base[(k*3 + {0,1,2}) * kBlock]
struct LdsCandidates3 {
    int32_t* base;
    HRT_DEV void key(int k, float& t, uint32_t& tri, uint32_t& inst) const { t = __int_as_float(base[(k * 3 + 0) * kBlock]); tri = (uint32_t)base[(k * 3 + 1) * kBlock]; inst = (uint32_t)base[(k * 3 + 2) * kBlock]; }
    HRT_DEV void set(int k, float t, uint32_t tri, uint32_t inst) { base[(k * 3 + 0) * kBlock] = __float_as_int(t); base[(k * 3 + 1) * kBlock] = (int32_t)tri; base[(k * 3 + 2) * kBlock] = (int32_t)inst; }
    HRT_DEV void move(int dst, int src) { for (int w = 0; w < 3; ++w) base[(dst * 3 + w) * kBlock] = base[(src * 3 + w) * kBlock]; }
};
// candidate list of one shadow ray in global memory (written by wf_extend<ANYHIT> when the ray finishes, read by wf_shadow)
struct GlobalCandidates {
    const uint2* base;
    HRT_DEV void key(int k, float& t, uint32_t& tri, uint32_t&) const { uint2 v = base[k]; t = __uint_as_float(v.x); tri = v.y; }
};
// BVH copy in LDS; W = node width (2: GpuNode, 4: GpuNode4)
template <int W>
struct LdsBvh {
    static constexpr int kWidth = W == 5 ? 4 : W; static constexpr bool kTwoLevel = false; static constexpr bool kLds = true;
    const float4* nodes; const float4* tris;
    HRT_DEV void node(int i, float4& a, float4& b, float4& c, float4& d) const { const float4* p = nodes + 4 * i; a = p[0]; b = p[1]; c = p[2]; d = p[3]; }
    HRT_DEV void tri(uint32_t i, float4& a, float4& b, float4& c) const { const float4* p = tris + 3 * i; a = p[0]; b = p[1]; c = p[2]; }
    // rows by 32-bit LDS address (the copy starts 128-byte aligned: setup_lds, so near ^ 16 is the far row of the same axis)
    typedef __attribute__((address_space(3))) const char* LdsPtr;
    HRT_DEV uint32_t rowoff(int i, uint32_t byteOffset) const { return (uint32_t)(uintptr_t)(LdsPtr) reinterpret_cast<const char*>(nodes) + (uint32_t)i * kLdsNode4Stride + byteOffset; }
    HRT_DEV float4 load(uint32_t off) const { return *reinterpret_cast<const float4*>((const char*)(LdsPtr)(uintptr_t)off); }
};
// (the trees in global memory: GlobalBvhOf, pt_traverse.h)

// Carves dynamic LDS: [stack: min(DEPTH, 32)*kBlock ints][bvh copy]; copies the BVH when LDS_BVH.
template <bool LDS_BVH, int DEPTH, int W, int LDSMAX>
HRT_DEV void setup_lds(char* smem, const SceneView& s, LdsStack<DEPTH, LDSMAX>& stack, LdsBvh<W>& lbvh, size_t extraBytes = 0)
{
    stack.base = reinterpret_cast<int32_t*>(smem) + threadIdx.x;
    stack.spill = nullptr; stack.spillStride = 0;
    if (LDS_BVH) {
        float4* dst = reinterpret_cast<float4*>(smem + (size_t)LdsStack<DEPTH, LDSMAX>::kRows * kBlock * 4 + extraBytes);
        const float4* srcN = W == 2 ? reinterpret_cast<const float4*>(s.nodes) : reinterpret_cast<const float4*>(s.nodes4);
        const float4* srcT = reinterpret_cast<const float4*>(s.tris);
        uint32_t nN = W == 2 ? s.nodeCount * 4 : s.node4Count * 8, nT = s.triCount * 3;
        uint32_t nNdst = nN;                                   // float4s the node copy occupies
        if (W == 2 || kLdsNode4Stride == 128u) { for (uint32_t i = threadIdx.x; i < nN; i += kBlock) dst[i] = srcN[i]; }
        else { nNdst = s.node4Count * (kLdsNode4Stride / 16u); for (uint32_t i = threadIdx.x; i < nN; i += kBlock) dst[(i >> 3) * (kLdsNode4Stride / 16u) + (i & 7u)] = srcN[i]; }
        for (uint32_t i = threadIdx.x; i < nT; i += kBlock) dst[nNdst + i] = srcT[i];
        lbvh.nodes = dst; lbvh.tris = dst + nNdst;
        __syncthreads();
    }
}

HRT_DEV uint32_t lane_id() { return threadIdx.x & 63u; }
// A value every lane of the wave holds identically (segment cursors, counts read from memory, the wave's index), moved to a scalar
// register: the compiler cannot prove uniformity of anything derived from threadIdx or from a load, and would otherwise keep such cursors
// in VGPRs and turn every test on them into an exec-mask branch.
HRT_DEV uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
HRT_DEV uint32_t prefix_rank(unsigned long long mask) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u)); }

// Statistics (wave_sum_u32: pt_path.h): one atomic per BLOCK on a counter shard (a returning-free add per wave on one word costs ~11 ns each and
// serialises at the kernel tail: 8192 waves = ~0.1 ms per launch).
HRT_DEV void block_count_add(unsigned long long* counterField0, size_t fieldOffsetWords, unsigned int perLane)
{
    __shared__ unsigned long long partial[kBlock / 64];
    unsigned long long w = wave_sum_u32(perLane);
    if (lane_id() == 0) partial[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (uint32_t i = 0; i < kBlock / 64; ++i) t += partial[i];
        if (t) atomicAdd(counterField0 + (size_t)(blockIdx.x % kCounterShards) * (sizeof(DeviceCounters) / 8) + fieldOffsetWords, t);
    }
}
// The same for N wave-uniform counts (each wave passes its own totals; fields = word indices into DeviceCounters).
template <int N>
HRT_DEV void block_count_add_uniform(DeviceCounters* counters, const int (&fields)[N], const unsigned int (&perWave)[N])
{
    __shared__ unsigned int partialU[N][kBlock / 64];
    if (lane_id() == 0)
        for (int k = 0; k < N; ++k) partialU[k][threadIdx.x >> 6] = perWave[k];
    __syncthreads();
    if (threadIdx.x < (uint32_t)N) {
        unsigned long long t = 0;
        for (uint32_t i = 0; i < kBlock / 64; ++i) t += partialU[threadIdx.x][i];
        if (t) atomicAdd(reinterpret_cast<unsigned long long*>(counters + blockIdx.x % kCounterShards) + fields[threadIdx.x], t);
    }
}
