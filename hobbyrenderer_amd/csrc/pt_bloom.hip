// pt_bloom.hip -- bloom, the first stage of the HDR post chain: /root/reference/src/shaders/Bloom.hlsl as driven by
// BloomRenderer::Render (src/BloomRenderer.cpp:48-175). A six-level image pyramid in R11G11B10_FLOAT: prefilter, five Jimenez
// downsamples, five tent upsamples, additive composite into the HDR colour image. The arithmetic is pt_bloom.h (shared with
// hrpt_bloom_host); this file holds the gfx950 kernels, the launch schedule and the host-thread executor.
//
// Schedule. One kernel per pass over 32 x 8 tiles (a wave = 32 x 2 texels, packed uint32 loads / stores; float4 for the HDR image). The
// seed copy Up[L - 1] = Down[L - 1] is not made: the first upsample reads Down[L - 1] directly (same values).
// Behind HRPT_BLOOM_FUSED_TAIL (off by default) ONE workgroup runs the downsamples that produce levels T..L-1 and the upsamples that
// produce levels L-2..T entirely in LDS, levels separated by __syncthreads(), and writes Up[T] -- the only thing a later pass reads -- to
// global memory; T is the first level with at most `tailTexels` texels whose tail fits in LDS. Both schedules run the same per-texel
// functions in the same order: identical bits. Measured at 1920 x 1080 (profiles/bloom_bench.txt) the tail LOSES: with the filter, the
// format decode and the correctly rounded divisions in software a downsampled texel is ~2000 dependent instructions, so the small levels
// are bound by that instruction stream (5 us per pass however small), not by launches or bytes, and one workgroup that walks several
// texels per lane serialises exactly that: 49 us for levels 4..5 against 15 us for the three launches it replaces.
#include <cmath>
#include <vector>

#include "pt_bloom.h"
#include "pt_host_rows.h"
#include "pt_image_kernel.h"
#include "pt_kernels.h"

namespace hrt {

namespace {
using namespace bloom;
using img::kTileX;
using img::kTileY;
using img::stage_grid;
using img::stage_index;
using img::stage_pixel;

constexpr int kTailThreads = 512;         // 256 VGPRs per lane: the 13-tap downsample keeps its 52 loads in flight without spilling (1024 threads spilled 320 B per lane)
constexpr size_t kTailLdsLimit = 160u * 1024u;      // LDS of one gfx950 CU
constexpr size_t kLdsNoOptIn = 64u * 1024u;         // dynamic LDS a launch may ask for without raising the kernel's limit

__global__ __launch_bounds__(kTileX * kTileY) void bloom_prefilter(const float* __restrict__ hdr, int W, int H, uint32_t* __restrict__ down0,
                                                                   int w, int h, float knee)
{
    int px, py;
    if (stage_pixel(w, h, &px, &py)) down0[stage_index(w, px, py)] = prefilter_texel(hdr, W, H, w, h, px, py, knee);
}

__global__ __launch_bounds__(kTileX * kTileY) void bloom_downsample(const uint32_t* __restrict__ src, int sw, int sh, uint32_t* __restrict__ dst,
                                                                    int w, int h)
{
    int px, py;
    if (stage_pixel(w, h, &px, &py)) dst[stage_index(w, px, py)] = down_texel(src, sw, sh, w, h, px, py);
}

__global__ __launch_bounds__(kTileX * kTileY) void bloom_upsample(const uint32_t* __restrict__ upper, int uw, int uh, const uint32_t* __restrict__ down,
                                                                  uint32_t* __restrict__ dst, int w, int h, float radius)
{
    int px, py;
    if (stage_pixel(w, h, &px, &py)) dst[stage_index(w, px, py)] = up_texel(upper, uw, uh, down, w, h, px, py, radius);
}

__global__ __launch_bounds__(kTileX * kTileY) void bloom_composite(float4* __restrict__ hdr, int W, int H, const uint32_t* __restrict__ up0, int w, int h,
                                                                   float intensity)
{
    int px, py;
    if (!stage_pixel(W, H, &px, &py)) return;
    const B3 b = composite_texel(up0, w, h, W, H, px, py, intensity);
    const size_t idx = stage_index(W, px, py);
    float4 c = hdr[idx];
    c.x = c.x + b.x; c.y = c.y + b.y; c.z = c.z + b.z;                              // BlendTargetAdditive; alpha stays
    hdr[idx] = c;
}

// Levels T..L-1 of the down pyramid and L-2..T of the up pyramid in one workgroup. LDS: Down[T], ..., Down[L-1], then Up[T+1], ..., Up[L-2]
// (Up[L-1] is Down[L-1]; Up[T] goes to global memory). Level i is (w0 >> i) x (h0 >> i). Requires T >= 1 and T <= L - 2.
__global__ __launch_bounds__(kTailThreads) void bloom_tail(const uint32_t* __restrict__ downPrev, uint32_t* __restrict__ upOut, int w0, int h0,
                                                           int T, int L, float radius)
{
    extern __shared__ uint32_t bloomLds[];
    const int tid = threadIdx.x;
    {   // Down[T] from Down[T - 1] in global memory
        const int sw = w0 >> (T - 1), sh = h0 >> (T - 1), w = w0 >> T, h = h0 >> T, n = w * h;
        for (int idx = tid; idx < n; idx += kTailThreads) bloomLds[idx] = down_texel(downPrev, sw, sh, w, h, idx % w, idx / w);
    }
    __syncthreads();
    int srcOff = 0;                                   // word offset of Down[i - 1] in LDS
    for (int i = T + 1; i < L; ++i) {
        const int sw = w0 >> (i - 1), sh = h0 >> (i - 1), w = w0 >> i, h = h0 >> i, n = w * h;
        const uint32_t* src = bloomLds + srcOff;
        uint32_t* dst = bloomLds + srcOff + sw * sh;
        for (int idx = tid; idx < n; idx += kTailThreads) dst[idx] = down_texel(src, sw, sh, w, h, idx % w, idx / w);
        srcOff += sw * sh;
        __syncthreads();
    }
    // srcOff = offset of Down[L - 1]; the up levels follow it
    const int upBase = srcOff + (w0 >> (L - 1)) * (h0 >> (L - 1));
    int downOff = srcOff;                             // offset of Down[i], walking back from L - 1
    int upperOff = srcOff;                            // offset of Up[i + 1]: Down[L - 1] first
    int nextUpOff = upBase;                           // where Up[i] goes while i > T: Up[L-2] first, then Up[L-3], ...
    for (int i = L - 2; i >= T; --i) {
        const int uw = w0 >> (i + 1), uh = h0 >> (i + 1), w = w0 >> i, h = h0 >> i, n = w * h;
        downOff -= n;
        const uint32_t* upper = bloomLds + upperOff;
        const uint32_t* down = bloomLds + downOff;
        if (i == T) {
            for (int idx = tid; idx < n; idx += kTailThreads) upOut[idx] = up_texel(upper, uw, uh, down, w, h, idx % w, idx / w, radius);
        } else {
            uint32_t* dst = bloomLds + nextUpOff;
            for (int idx = tid; idx < n; idx += kTailThreads) dst[idx] = up_texel(upper, uw, uh, down, w, h, idx % w, idx / w, radius);
            upperOff = nextUpOff;
            nextUpOff += n;
            __syncthreads();
        }
    }
}

struct Schedule {
    int L = 0;
    int w[kMipCount] = {}, h[kMipCount] = {};
    size_t off[kMipCount + 1] = {};                  // word offset of level i in a pyramid buffer
    Schedule(uint32_t W, uint32_t H)
    {
        L = level_count(W, H);
        for (int i = 0; i < L; ++i) { w[i] = (int)((W / 2u) >> i); h[i] = (int)((H / 2u) >> i); off[i + 1] = off[i] + (size_t)w[i] * (size_t)h[i]; }
    }
    // first level of the fused tail, or L when there is none
    int tail_start(uint32_t tailTexels, size_t* ldsBytes) const
    {
        if (tailTexels == 0) return L;
        for (int T = 1; T + 2 <= L; ++T) {
            size_t words = off[L] - off[T];                                          // Down[T..L-1]
            if (L - 2 >= T + 1) words += off[L - 1] - off[T + 1];                    // Up[T+1..L-2]
            if ((size_t)w[T] * (size_t)h[T] <= tailTexels && words * 4u <= kTailLdsLimit) { *ldsBytes = words * 4u; return T; }
        }
        return L;
    }
};

} // namespace

size_t bloom_pyramid_words(uint32_t width, uint32_t height) { Schedule s(width, height); return s.off[s.L]; }

void bloom_pack_probe(const float* rgb, uint32_t count, uint32_t* packed, float* unpacked)
{
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t p = pack(b3(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]));
        if (packed) packed[i] = p;
        if (unpacked) { const B3 c = unpack(p); unpacked[3 * i] = c.x; unpacked[3 * i + 1] = c.y; unpacked[3 * i + 2] = c.z; }
    }
}

bool bloom_params_valid(const HrptBloomParams& p)
{
    return std::isfinite(p.knee) && std::isfinite(p.intensity) && std::isfinite(p.upsampleRadius) && p.knee >= 0.0f && p.intensity >= 0.0f &&
           p.upsampleRadius >= 0.0f;
}

hipError_t launch_bloom(float4* hdr, uint32_t width, uint32_t height, const HrptBloomParams& p, uint32_t* downPyramid, uint32_t* upPyramid,
                        uint32_t tailTexels, hipStream_t stream)
{
    const Schedule s(width, height);
    if (s.L == 0) return hipSuccess;
    const int W = (int)width, H = (int)height;
    const dim3 block = img::stage_block();
    size_t ldsBytes = 0;
    const int T = s.tail_start(tailTexels, &ldsBytes);
    hipLaunchKernelGGL(bloom_prefilter, stage_grid(s.w[0], s.h[0]), block, 0, stream, reinterpret_cast<const float*>(hdr), W, H, downPyramid, s.w[0], s.h[0], p.knee);
    for (int i = 1; i < s.L && i < T; ++i)
        hipLaunchKernelGGL(bloom_downsample, stage_grid(s.w[i], s.h[i]), block, 0, stream, downPyramid + s.off[i - 1], s.w[i - 1], s.h[i - 1],
                           downPyramid + s.off[i], s.w[i], s.h[i]);
    int top = s.L - 1;                                         // the level the remaining upsamples start from
    const uint32_t* upper = downPyramid + s.off[top];          // Up[L - 1] = Down[L - 1] (the seed copy, not made)
    if (T < s.L) {
        if (ldsBytes > kLdsNoOptIn) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(bloom_tail), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTailLdsLimit);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(bloom_tail, dim3(1), dim3(kTailThreads), ldsBytes, stream, downPyramid + s.off[T - 1], upPyramid + s.off[T], s.w[0], s.h[0],
                           T, s.L, p.upsampleRadius);
        top = T; upper = upPyramid + s.off[T];
    }
    for (int i = top - 1; i >= 0; --i) {
        hipLaunchKernelGGL(bloom_upsample, stage_grid(s.w[i], s.h[i]), block, 0, stream, upper, s.w[i + 1], s.h[i + 1], downPyramid + s.off[i],
                           upPyramid + s.off[i], s.w[i], s.h[i], p.upsampleRadius);
        upper = upPyramid + s.off[i];
    }
    hipLaunchKernelGGL(bloom_composite, stage_grid(width, height), block, 0, stream, hdr, W, H, upper, s.w[0], s.h[0], p.intensity);
    return hipGetLastError();
}

void bloom_host(const float* hdrIn, float* hdrOut, uint32_t width, uint32_t height, const HrptBloomParams& p, int nthreads)
{
    const Schedule s(width, height);
    const int W = (int)width, H = (int)height;
    if (s.L > 0) {
        std::vector<uint32_t> down(s.off[s.L]), up(s.off[s.L]);
        uint32_t* d = down.data(); uint32_t* u = up.data();
        over_rows(s.h[0], nthreads, [&](int y) { for (int x = 0; x < s.w[0]; ++x) d[(size_t)y * s.w[0] + x] = prefilter_texel(hdrIn, W, H, s.w[0], s.h[0], x, y, p.knee); });
        for (int i = 1; i < s.L; ++i)
            over_rows(s.h[i], nthreads, [&](int y) {
                for (int x = 0; x < s.w[i]; ++x) d[s.off[i] + (size_t)y * s.w[i] + x] = down_texel(d + s.off[i - 1], s.w[i - 1], s.h[i - 1], s.w[i], s.h[i], x, y);
            });
        const uint32_t* upper = d + s.off[s.L - 1];
        for (int i = s.L - 2; i >= 0; --i) {
            over_rows(s.h[i], nthreads, [&](int y) {
                for (int x = 0; x < s.w[i]; ++x)
                    u[s.off[i] + (size_t)y * s.w[i] + x] = up_texel(upper, s.w[i + 1], s.h[i + 1], d + s.off[i], s.w[i], s.h[i], x, y, p.upsampleRadius);
            });
            upper = u + s.off[i];
        }
        // hdrOut may be hdrIn: the composite reads and writes one pixel, the prefilter has finished with the image
        over_rows(H, nthreads, [&](int y) {
            for (int x = 0; x < W; ++x) {
                const B3 b = composite_texel(upper, s.w[0], s.h[0], W, H, x, y, p.intensity);
                const img::T4 in = img::load4(hdrIn, W, x, y);
                store4(hdrOut + ((size_t)y * W + x) * 4, img::t4(in.x + b.x, in.y + b.y, in.z + b.z, in.w));
            }
        });
    } else if (hdrOut != hdrIn) {
        for (size_t i = 0, n = (size_t)W * H * 4; i < n; ++i) hdrOut[i] = hdrIn[i];
    }
}

} // namespace hrt
