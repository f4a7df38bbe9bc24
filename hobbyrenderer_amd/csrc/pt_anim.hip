// pt_anim.hip -- the gfx950 kernels of the animation stage (hrpt_animate): times -> node poses -> instance records + joint palette + morph
// weights, all in device memory, so that a moving frame needs no host arithmetic and no palette upload. The arithmetic is pt_anim.h (shared
// with the host executor); this file holds three small kernels and their launcher. 256 lanes per block, every lane bounds-checked.
//   anim_sample          one lane per live channel: the animation's time (staged in LDS up to HRPT_ANIM_LDS_MAX_ANIMATIONS animations, read
//                        from global memory beyond), one sampler evaluation, a scatter to the channel's live targets in the per-node TRS array
//                        (48 bytes per node, seeded with the base pose at upload) or the weight array. A (node, path) or slot has one live
//                        writer (resolved at creation): no races, no order.
//   anim_compose         one lane per composed node of ONE depth group: local from TRS, world = local . world(parent); the parent was written
//                        by an earlier launch, or is a static node whose baseWorld seeded the array. One launch per group.
//   anim_compose_groups  the same for an animation whose composed nodes all fit one workgroup: one launch that walks the groups with a
//                        barrier between them (the worlds go through global memory; __syncthreads orders them within the workgroup).
//   anim_emit            lanes [0, instanceRange): one 160-byte instance record each, read and written as ten 16-byte vectors: m_PrevWorld =
//                        m_World, then m_World = world(node) where the record hangs under a composed node. Lanes after those: one joint each,
//                        three 16-byte stores of the palette row-major 3 x 4.
// No scratch, no dynamic allocation, no communication between workgroups. LDS: anim_sample's staged times and nothing else.
#include "pt_anim.h"
#include "pt_kernels.h"

namespace hrt {

namespace {
constexpr uint32_t kBlock = 256;

__global__ __launch_bounds__(kBlock) void anim_sample(anim::Tables tb, const float* __restrict__ times, float* __restrict__ trs, float* __restrict__ weights)
{
    __shared__ float staged[HRPT_ANIM_LDS_MAX_ANIMATIONS];
    const bool inLds = tb.animationCount <= HRPT_ANIM_LDS_MAX_ANIMATIONS;
    if (inLds) {
        for (uint32_t k = threadIdx.x; k < tb.animationCount; k += kBlock) staged[k] = times[k];
        __syncthreads();
    }
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= tb.channelCount) return;
    const uint32_t animation = tb.samplers[tb.channels[k].sampler].animation;
    anim::apply_channel(tb, k, inLds ? staged[animation] : times[animation], trs, weights);
}

__global__ __launch_bounds__(kBlock) void anim_compose(anim::Tables tb, const float* __restrict__ trs, float* worlds, uint32_t first, uint32_t count)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k < count) anim::compose_node(tb, first + k, trs, worlds);
}

// One workgroup; tb.composedCount <= kBlock.
__global__ __launch_bounds__(kBlock) void anim_compose_groups(anim::Tables tb, const float* __restrict__ trs, float* worlds, const uint32_t* __restrict__ groupFirst, uint32_t groups)
{
    for (uint32_t g = 0; g < groups; ++g) {
        const uint32_t k = groupFirst[g] + threadIdx.x;
        if (k < groupFirst[g + 1]) anim::compose_node(tb, k, trs, worlds);
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void anim_emit(anim::Tables tb, const float* __restrict__ worlds, float4* __restrict__ records, uint32_t recordCount, float4* __restrict__ palette)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k < recordCount) {
        float4* r = records + 10ull * k;
        float4 v[10];
        for (int e = 0; e < 10; ++e) v[e] = r[e];
        for (int e = 0; e < 4; ++e) v[4 + e] = v[e];
        const uint32_t node = tb.rangeNode[k];
        if (node != anim::kNoNode) {
            const float4* w = reinterpret_cast<const float4*>(worlds) + 4ull * node;
            for (int e = 0; e < 4; ++e) v[e] = w[e];
        }
        for (int e = 0; e < 10; ++e) r[e] = v[e];
    } else if (k - recordCount < tb.jointCount) {
        const uint32_t j = k - recordCount;
        float m[12];
        anim::joint_matrix(tb.inverseBind + 16ull * j, worlds + 16ull * tb.jointNode[j], m);
        float4* out = palette + 3ull * j;
        out[0] = make_float4(m[0], m[1], m[2], m[3]);
        out[1] = make_float4(m[4], m[5], m[6], m[7]);
        out[2] = make_float4(m[8], m[9], m[10], m[11]);
    }
}

uint32_t blocks_for(uint32_t n) { return n / kBlock + (n % kBlock != 0u); }
} // namespace

hipError_t launch_animate(const anim::Tables& tb, const float* times, const uint32_t* groupFirst, const uint32_t* groupFirstHost, uint32_t groups,
                          float* trs, float* worlds, float* weights, float* palette, void* records, hipStream_t stream)
{
    if (tb.channelCount) hipLaunchKernelGGL(anim_sample, dim3(blocks_for(tb.channelCount)), dim3(kBlock), 0, stream, tb, times, trs, weights);
    if (tb.composedCount && tb.composedCount <= kBlock) {
        hipLaunchKernelGGL(anim_compose_groups, dim3(1), dim3(kBlock), 0, stream, tb, trs, worlds, groupFirst, groups);
    } else {
        for (uint32_t g = 0; g < groups; ++g) {
            const uint32_t first = groupFirstHost[g], count = groupFirstHost[g + 1] - first;
            if (count) hipLaunchKernelGGL(anim_compose, dim3(blocks_for(count)), dim3(kBlock), 0, stream, tb, trs, worlds, first, count);
        }
    }
    const uint32_t recordCount = records ? tb.instanceRange : 0u;
    if (recordCount + tb.jointCount)
        hipLaunchKernelGGL(anim_emit, dim3(blocks_for(recordCount + tb.jointCount)), dim3(kBlock), 0, stream, tb, worlds, static_cast<float4*>(records), recordCount,
                           reinterpret_cast<float4*>(palette));
    return hipGetLastError();
}

} // namespace hrt
