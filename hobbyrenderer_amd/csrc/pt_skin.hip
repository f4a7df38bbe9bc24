// pt_skin.hip -- the gfx950 kernel of the vertex producer (hrpt_skin_vertices_device, hrpt_update_vertices_skinned): morph targets and
// four-joint linear-blend skinning of a bind pose in device memory into HrptVertexFloat records, what the quantiser (pt_deform.hip)
// reads. The arithmetic is pt_skin.h (shared with the host executor); this file holds skin_vertices<LDS> and its launcher.
// One vertex per lane, 256 lanes per block, bounds-checked; a block walks the 256-vertex chunks blockIdx.x, blockIdx.x + gridDim.x, ...
// (at most kMaxBlocks blocks: beyond about a quarter of a million vertices a block takes several chunks and stages its palette once for
// all of them). Per lane: the bind pose as three 16-byte loads, the four joint indices as one 8-byte load, the four weights as one
// 16-byte load, a morph delta as the nine dwords of its 36-byte record (4-byte aligned: a wave's records are 2 304 contiguous bytes),
// the result as three 16-byte stores.
// The joint palette is 48 bytes per joint, 16-byte aligned. LDS = true (jointCount <= HRPT_SKIN_LDS_MAX_JOINTS): the block stages
// jointCount x 48 bytes with 16-byte loads behind one barrier, and a lane's gather of 4 x 48 bytes is twelve ds_read_b128; the LDS is
// the palette stage (48 x HRPT_SKIN_LDS_MAX_JOINTS bytes) and nothing more. LDS = false: the same twelve 16-byte reads go to global
// memory (read-only, L2-resident). Status: word 0 "output position not finite", word 1 "joint index out of range", each raised by a
// plain vector store of 1 (every writer stores the same value); may be null. DESIGN.md section 22 has the register count, the ISA of
// the loads, the measurements, and the variant that quantised in the same kernel (measured no faster, so not kept).
#include "pt_skin.h"
#include "pt_kernels.h"

namespace hrt {

namespace {
constexpr uint32_t kBlock = 256;
constexpr uint32_t kMaxBlocks = 1024;           // four blocks for each of the 256 compute units

// Stages the palette (LDS = true; every lane of the block must arrive) and returns the 16-byte rows the lanes gather from.
template <bool LDS> __device__ __forceinline__ const float4* stage_palette(const HrptSkinArgs& a)
{
    const float4* rows = reinterpret_cast<const float4*>(a.jointMatrices);
    if constexpr (LDS) {
        __shared__ float4 palette[3 * HRPT_SKIN_LDS_MAX_JOINTS];
        if (a.joints) {
            for (uint32_t k = threadIdx.x; k < 3u * a.jointCount; k += kBlock) palette[k] = rows[k];
            __syncthreads();
        }
        return palette;
    } else {
        return rows;
    }
}

// Vertex i < a.count through pt_skin.h's skin_vertex; returns its status bits.
__device__ __forceinline__ uint32_t skin_lane(const HrptSkinArgs& a, const float4* __restrict__ palette, uint32_t i, HrptVertexFloat& v)
{
    const float4* in = reinterpret_cast<const float4*>(a.base);
    const float4 x = in[3ull * i], y = in[3ull * i + 1u], z = in[3ull * i + 2u];
    HrptVertexFloat b;
    b.pos[0] = x.x; b.pos[1] = x.y; b.pos[2] = x.z;
    b.normal[0] = x.w; b.normal[1] = y.x; b.normal[2] = y.y;
    b.uv[0] = y.z; b.uv[1] = y.w;
    b.tangent[0] = z.x; b.tangent[1] = z.y; b.tangent[2] = z.z; b.tangent[3] = z.w;
    uint16_t joints[4] = { 0, 0, 0, 0 };
    float weights[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (a.joints) {
        const uint2 j = reinterpret_cast<const uint2*>(a.joints)[i];
        const float4 w = reinterpret_cast<const float4*>(a.weights)[i];
        joints[0] = (uint16_t)(j.x & 0xffffu); joints[1] = (uint16_t)(j.x >> 16); joints[2] = (uint16_t)(j.y & 0xffffu); joints[3] = (uint16_t)(j.y >> 16);
        weights[0] = w.x; weights[1] = w.y; weights[2] = w.z; weights[3] = w.w;
    }
    const HrptSkinMorphDelta* deltas = a.deltas;
    const uint32_t count = a.count;
    return skin::skin_vertex(
        b, a.morphWeights, a.targetCount,
        [=](uint32_t k, float* d) {
            const float* r = reinterpret_cast<const float*>(deltas + ((size_t)k * count + i));
            for (int c = 0; c < 9; ++c) d[c] = r[c];
        },
        a.joints != nullptr, joints, weights, a.jointCount,
        [=](uint32_t j, float* m) {
            const float4 r0 = palette[3u * j], r1 = palette[3u * j + 1u], r2 = palette[3u * j + 2u];
            m[0] = r0.x; m[1] = r0.y; m[2] = r0.z; m[3] = r0.w; m[4] = r1.x; m[5] = r1.y; m[6] = r1.z; m[7] = r1.w;
            m[8] = r2.x; m[9] = r2.y; m[10] = r2.z; m[11] = r2.w;
        },
        v);
}

__device__ __forceinline__ void raise_status(uint32_t* __restrict__ status, uint32_t bits)
{
    if (!status) return;
    if (bits & skin::kPositionNotFinite) status[0] = 1u;
    if (bits & skin::kJointOutOfRange) status[1] = 1u;
}

template <bool LDS> __global__ __launch_bounds__(kBlock) void skin_vertices(HrptSkinArgs a, float4* __restrict__ out, uint32_t* __restrict__ status)
{
    const float4* palette = stage_palette<LDS>(a);
    const uint32_t chunks = a.count / kBlock + (a.count % kBlock != 0u);
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const uint32_t i = chunk * kBlock + threadIdx.x;
        if (i >= a.count) break;
        HrptVertexFloat v;
        raise_status(status, skin_lane(a, palette, i, v));
        out[3ull * i] = make_float4(v.pos[0], v.pos[1], v.pos[2], v.normal[0]);
        out[3ull * i + 1u] = make_float4(v.normal[1], v.normal[2], v.uv[0], v.uv[1]);
        out[3ull * i + 2u] = make_float4(v.tangent[0], v.tangent[1], v.tangent[2], v.tangent[3]);
    }
}

// palette: 0 = by joint count, 1 = always the global gather (pt_kernels.h)
bool palette_in_lds(const HrptSkinArgs& a, int palette)
{
    return a.joints && a.jointCount <= HRPT_SKIN_LDS_MAX_JOINTS && palette != 1;
}

uint32_t grid_of(uint32_t count)
{
    const uint32_t chunks = count / kBlock + (count % kBlock != 0u);
    return chunks < kMaxBlocks ? chunks : kMaxBlocks;
}
} // namespace

hipError_t launch_skin_vertices(const HrptSkinArgs& a, HrptVertexFloat* out, uint32_t* status2, int palette, hipStream_t stream)
{
    if (a.count == 0) return hipSuccess;
    if (palette_in_lds(a, palette)) hipLaunchKernelGGL(skin_vertices<true>, dim3(grid_of(a.count)), dim3(kBlock), 0, stream, a, reinterpret_cast<float4*>(out), status2);
    else hipLaunchKernelGGL(skin_vertices<false>, dim3(grid_of(a.count)), dim3(kBlock), 0, stream, a, reinterpret_cast<float4*>(out), status2);
    return hipGetLastError();
}

} // namespace hrt
