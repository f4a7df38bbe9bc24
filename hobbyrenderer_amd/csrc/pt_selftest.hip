// pt_selftest.hip -- the device side of pt_capi_selftest.cpp's decode and lookup self-tests: the binary16 and unorm8 decode tables, and the
// probes that call the texture sampling and atmosphere lookups of the shading code off the render path. (The acceleration structure's
// self-test is pt_bvh_nodes.hip.)
#include "pt_kernels.h"
#include "pt_surface.h"
#include "pt_atmosphere.h"

namespace hrt {

__global__ void pt_f16_table_kernel(float* __restrict__ out)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 65536u) out[i] = half_bits_to_float(i);
}
__global__ void pt_unorm8_table_kernel(float* __restrict__ out)
{
    uint32_t i = threadIdx.x;
    if (i < 256u) { out[i] = unorm8_to_float(i); out[256u + i] = (float)i / 255.0f; }      // fast path, and the division it replaces
}
hipError_t launch_unorm8_table(float* out512, hipStream_t stream)
{
    hipLaunchKernelGGL(pt_unorm8_table_kernel, dim3(1), dim3(256), 0, stream, out512);
    return hipGetLastError();
}
hipError_t launch_f16_table(float* out, hipStream_t stream)
{
    hipLaunchKernelGGL(pt_f16_table_kernel, dim3(256), dim3(256), 0, stream, out);
    return hipGetLastError();
}

// Self-test of texture sampling (hrpt_selftest_sample_textures): one thread per probe calls sample_texture, pbr_textures_batched and
// sample_texture_grad of pt_surface.h / pt_texture.h as the shade and any-hit code does, over the scene's own texture and material tables.
__device__ __forceinline__ void store4(float* dst, const f4& v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w; }
__global__ void pt_sample_textures_kernel(SceneView s, uint32_t materialCount, const HrptTextureProbe* __restrict__ probes,
                                          HrptTextureProbeResult* __restrict__ results, uint32_t count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const HrptTextureProbe p = probes[i];
    HrptTextureProbeResult& r = results[i];
    f4 zero; zero.x = zero.y = zero.z = zero.w = 0.0f;
    f4 single[4] = { zero, zero, zero, zero }, batched[4] = { zero, zero, zero, zero }, grad = zero;
    uint32_t accepted = 0u;
    if (p.material < materialCount) {
        const HrptMaterialConstants& m = s.materials[p.material];
        f2 uv, ddx, ddy; uv.x = p.uv[0]; uv.y = p.uv[1]; ddx.x = p.ddx[0]; ddx.y = p.ddx[1]; ddy.x = p.ddy[0]; ddy.y = p.ddy[1];
        if (p.texFlags & HRPT_TEXFLAG_ALBEDO) single[0] = sample_texture(s, m.m_AlbedoTextureIndex, m.m_AlbedoSamplerIndex, uv);
        if (p.texFlags & HRPT_TEXFLAG_ROUGHNESS_METALLIC) single[1] = sample_texture(s, m.m_RoughnessMetallicTextureIndex, m.m_RoughnessSamplerIndex, uv);
        if (p.texFlags & HRPT_TEXFLAG_EMISSIVE) single[2] = sample_texture(s, m.m_EmissiveTextureIndex, m.m_EmissiveSamplerIndex, uv);
        if (p.texFlags & HRPT_TEXFLAG_NORMAL) single[3] = sample_texture(s, m.m_NormalTextureIndex, m.m_NormalSamplerIndex, uv);
#ifndef HRPT_NO_BATCHED_TEXTURES
        f4 tex[4];
        if (pbr_textures_batched(s, uv, m, p.texFlags, tex)) {
            accepted = 1u;
            for (int k = 0; k < 4; ++k) batched[k] = tex[k];
        }
#endif
        if (m.m_AlbedoTextureIndex < s.textureCount && s.textures[m.m_AlbedoTextureIndex].texels)      // candidate_alpha_grad's guards
            grad = sample_texture_grad(s.textures[m.m_AlbedoTextureIndex], m.m_AlbedoSamplerIndex, uv, ddx, ddy);
    }
    for (int k = 0; k < 4; ++k) { store4(r.single[k], single[k]); store4(r.batched[k], batched[k]); }
    r.batchedAccepted = accepted; r.pad[0] = r.pad[1] = r.pad[2] = 0u;
    store4(r.grad, grad);
}
hipError_t launch_sample_textures(const SceneView& scene, uint32_t materialCount, const HrptTextureProbe* probes, HrptTextureProbeResult* results,
                                  uint32_t count, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(pt_sample_textures_kernel, dim3((count + 63u) / 64u), dim3(64), 0, stream, scene, materialCount, probes, results, count);
    return hipGetLastError();
}

// Self-test of the run-time atmosphere lookups (hrpt_selftest_atmosphere): one thread per probe calls atm::sky_radiance, atm::sun_radiance
// and atm::transmittance_to_top of pt_atmosphere.h as the miss and sun-light code of pt_path.h does, over the scene's own RGBA16F tables.
__global__ void pt_atmosphere_probe_kernel(SceneView s, const HrptAtmosphereProbe* __restrict__ probes, HrptAtmosphereProbeResult* __restrict__ results,
                                           uint32_t count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const HrptAtmosphereProbe p = probes[i];
    HrptAtmosphereProbeResult& r = results[i];
    const f3 cam = mk3(p.cameraPos[0], p.cameraPos[1], p.cameraPos[2]), view = mk3(p.viewRay[0], p.viewRay[1], p.viewRay[2]);
    const f3 sunDir = mk3(p.sunDir[0], p.sunDir[1], p.sunDir[2]);
    const f3 pa = atm::atmosphere_pos(cam);
    const f3 sky = atm::sky_radiance(s, cam, view, sunDir, p.sunIntensity, p.addSunDisk != 0u);
    const f3 sun = atm::sun_radiance(s, pa, sunDir, p.sunIntensity);
    const float rr = length(pa), mu = dot(pa, view) / rr;
    const f3 tr = atm::transmittance_to_top(s, rr, mu);
    r.sky[0] = sky.x; r.sky[1] = sky.y; r.sky[2] = sky.z;
    r.sun[0] = sun.x; r.sun[1] = sun.y; r.sun[2] = sun.z;
    r.transmittance[0] = tr.x; r.transmittance[1] = tr.y; r.transmittance[2] = tr.z;
    r.r = rr; r.mu = mu; r.pad = 0.0f;
}
hipError_t launch_atmosphere_probes(const SceneView& scene, const HrptAtmosphereProbe* probes, HrptAtmosphereProbeResult* results, uint32_t count, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(pt_atmosphere_probe_kernel, dim3((count + 63u) / 64u), dim3(64), 0, stream, scene, probes, results, count);
    return hipGetLastError();
}

} // namespace hrt
