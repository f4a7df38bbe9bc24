// pt_deform.hip -- the gfx950 kernel of the vertex quantiser (hrpt_quantize_vertices_device, hrpt_update_vertices_device): float vertices
// a skinning or simulation kernel left in device memory become the scene format's 24-byte records without crossing PCIe. The
// arithmetic is pt_deform.h (shared with the host executor); this file holds the kernel and its launcher.
//
// One thread per vertex, 256 threads per block, bounds-checked. A lane reads its 48 bytes as three 16-byte loads (a wave reads 3 072
// contiguous bytes) and writes its 24-byte record; a wave's records are 1 536 contiguous bytes, so every cache line the wave touches is
// written whole between its stores. No LDS, no scratch, 72 bytes of traffic per vertex. A position that is not finite raises *flag (a plain
// store of 1 by every lane that sees one: all writers write the same value); flag may be null. DESIGN.md section 21 has the register
// count and the store shape the compiler chose.
#include "pt_deform.h"
#include "pt_kernels.h"

namespace hrt {

namespace {
constexpr uint32_t kBlock = 256;

// `out` need only be 4-byte aligned (a range of the vertex buffer starts at any record): the record goes out as six dwords the compiler may group
struct Words6 { uint32_t w[6]; };

__global__ __launch_bounds__(kBlock) void quantise_vertices(const float4* __restrict__ in, uint32_t count, Words6* __restrict__ out, uint32_t* __restrict__ flag)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const float4 a = in[3ull * i], b = in[3ull * i + 1u], c = in[3ull * i + 2u];
    HrptVertexFloat v;
    v.pos[0] = a.x; v.pos[1] = a.y; v.pos[2] = a.z;
    v.normal[0] = a.w; v.normal[1] = b.x; v.normal[2] = b.y;
    v.uv[0] = b.z; v.uv[1] = b.w;
    v.tangent[0] = c.x; v.tangent[1] = c.y; v.tangent[2] = c.z; v.tangent[3] = c.w;
    if (flag && !deform::position_finite(v.pos)) *flag = 1u;
    const HrptVertexQuantized q = deform::quantize_vertex(v);
    Words6 r;
    r.w[0] = deform::float_bits(q.m_Pos[0]); r.w[1] = deform::float_bits(q.m_Pos[1]); r.w[2] = deform::float_bits(q.m_Pos[2]);
    r.w[3] = q.m_Normal; r.w[4] = q.m_Uv; r.w[5] = q.m_Tangent;
    out[i] = r;
}
} // namespace

hipError_t launch_quantise_vertices(const HrptVertexFloat* in, uint32_t count, HrptVertexQuantized* out, uint32_t* flag, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(quantise_vertices, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, reinterpret_cast<const float4*>(in), count,
                       reinterpret_cast<Words6*>(out), flag);
    return hipGetLastError();
}

} // namespace hrt
