// pt_atmosphere.h -- the Bruneton atmosphere lookups (namespace atm).
#pragma once

#include "pt_texture.h"

namespace hrt {

// ------------------------------------------------------------------ atmosphere (Atmosphere.hlsli)
namespace atm {
constexpr float kBottom = 6360.0f, kTop = 6420.0f;
constexpr float kSunAngularRadius = 0.004675f;      // 0.00935 / 2.0, Atmosphere.hlsli:42
constexpr float kMuSMin = -0.207912f, kMieG = 0.8f;

HRT_DEV f3 solar_irradiance() { return mk3(1.474000f, 1.850400f, 1.911980f); }
HRT_DEV float safe_sqrt(float a) { return hrt_sqrt(hrt_max(a, 0.0f)); }
HRT_DEV float dist_top(float r, float mu)                                   // :130-134
{
    float disc = r * r * (mu * mu - 1.0f) + kTop * kTop;
    return hrt_max(-r * mu + safe_sqrt(disc), 0.0f);
}
HRT_DEV bool ray_hits_ground(float r, float mu)                              // :157-160
{
    return mu < 0.0f && r * r * (mu * mu - 1.0f) + kBottom * kBottom >= 0.0f;
}
HRT_DEV float texcoord(float x, int size) { return 0.5f / (float)size + x * (1.0f - 1.0f / (float)size); }   // :176-179
HRT_DEV f3 transmittance_to_top(const SceneView& s, float r, float mu)      // :190-198, :207-211
{
    float rho = safe_sqrt(r * r - kBottom * kBottom);
    float d = dist_top(r, mu);
    float H = safe_sqrt(kTop * kTop - kBottom * kBottom);
    float x_mu = texcoord(d / (rho + H), 256);
    float x_r = texcoord(rho / H, 64);
    f4 t = sample_lut2d(s.lutTransmittance, 256, 64, x_mu, x_r);
    return mk3(t.x, t.y, t.z);
}
HRT_DEV f4 scattering_uvwz(float r, float mu, float mu_s, float nu, bool hitsGround)   // :263-297
{
    float H = hrt_sqrt(kTop * kTop - kBottom * kBottom);
    float rho = safe_sqrt(r * r - kBottom * kBottom);
    float u_r = texcoord(rho / H, 32);
    float r_mu = r * mu;
    float disc = r_mu * r_mu - r * r + kBottom * kBottom;
    float u_mu;
    if (hitsGround) {
        float d = -r_mu - safe_sqrt(disc);
        float d_min = r - kBottom, d_max = rho;
        u_mu = 0.5f - 0.5f * texcoord(d_max == d_min ? 0.0f : (d - d_min) / (d_max - d_min), 64);
    } else {
        float d = -r_mu + safe_sqrt(disc + H * H);
        float d_min = kTop - r, d_max = rho + H;
        u_mu = 0.5f + 0.5f * texcoord((d - d_min) / (d_max - d_min), 64);
    }
    float d = dist_top(kBottom, mu_s);
    float d_min = kTop - kBottom, d_max = H;
    float a = (d - d_min) / (d_max - d_min);
    float D = dist_top(kBottom, kMuSMin);
    float A = (D - d_min) / (d_max - d_min);
    float u_mu_s = texcoord(hrt_max(1.0f - a / A, 0.0f) / (1.0f + a), 32);
    f4 o; o.x = (nu + 1.0f) / 2.0f; o.y = u_mu_s; o.z = u_mu; o.w = u_r;
    return o;
}
HRT_DEV f3 combined_scattering(const SceneView& s, float r, float mu, float mu_s, float nu, bool hitsGround, f3& singleMie)  // :305-341
{
    f4 uvwz = scattering_uvwz(r, mu, mu_s, nu, hitsGround);
    float tex_coord_x = uvwz.x * 7.0f;
    float tex_x = hrt_floor(tex_coord_x);
    float lerp_val = tex_coord_x - tex_x;
    float u0 = (tex_x + uvwz.y) / 8.0f, u1 = (tex_x + 1.0f + uvwz.y) / 8.0f;
    f4 s0 = sample_lut3d(s.lutScattering, 256, 128, 32, u0, uvwz.z, uvwz.w);
    f4 s1 = sample_lut3d(s.lutScattering, 256, 128, 32, u1, uvwz.z, uvwz.w);
    f4 cs = lerp4(s0, s1, lerp_val);
    if (cs.x <= 0.0f) singleMie = mk3(0.0f, 0.0f, 0.0f);
    else {
        const f3 ray = mk3(0.005802f, 0.013558f, 0.033100f), mie = mk3(0.003996f, 0.003996f, 0.003996f);
        float k = ray.x / mie.x;
        f3 ratio = mk3(mie.x / ray.x, mie.y / ray.y, mie.z / ray.z);
        f3 t = mk3(cs.x * cs.w / cs.x * k, cs.y * cs.w / cs.x * k, cs.z * cs.w / cs.x * k);
        singleMie = t * ratio;
    }
    return mk3(cs.x, cs.y, cs.z);
}
HRT_DEV float rayleigh_phase(float nu) { float k = 3.0f / (16.0f * HRT_PI); return k * (1.0f + nu * nu); }   // :349-353
HRT_DEV float mie_phase(float g, float nu)                                                                   // :355-359
{
    float k = 3.0f / (8.0f * HRT_PI) * (1.0f - g * g) / (2.0f + g * g);
    float b = hrt_max(1.0f + g * g - 2.0f * g * nu, 0.0001f);
    return k * (1.0f + nu * nu) / (b * hrt_sqrt(b));
}
HRT_DEV float smoothstep(float a, float b, float x) { float t = hrt_saturate((x - a) / (b - a)); return (t * t) * (3.0f - 2.0f * t); }
HRT_DEV f3 transmittance_to_sun(const SceneView& s, float r, float mu_s)    // :414-420
{
    float sin_theta_h = kBottom / r;
    float cos_theta_h = -hrt_sqrt(hrt_max(1.0f - sin_theta_h * sin_theta_h, 0.0f));
    float e = sin_theta_h * kSunAngularRadius;
    float f = smoothstep(-e, e, mu_s - cos_theta_h);
    return transmittance_to_top(s, r, mu_s) * f;
}
HRT_DEV f3 atmosphere_pos(f3 worldPos) { return (worldPos - mk3(0.0f, -6360000.0f, 0.0f)) / 1000.0f; }   // :564-567
HRT_DEV f3 sun_radiance(const SceneView& s, f3 p_atmo, f3 sunDir, float sunIntensity)   // :569-574
{
    float r = length(p_atmo);
    float mu_s = dot(p_atmo, sunDir) / r;
    return (solar_irradiance() * transmittance_to_sun(s, r, mu_s)) * sunIntensity;
}
// GetAtmosphereSkyRadiance :583-601 (GetSkyRadiance :458-500 with shadow_length 0)
HRT_DEV f3 sky_radiance(const SceneView& s, f3 cameraPos, f3 viewRay, f3 sunDir, float sunIntensity, bool addSunDisk)
{
    f3 camera = atmosphere_pos(cameraPos);
    float r = length(camera);
    float rmu = dot(camera, viewRay);
    float dtop = -rmu - safe_sqrt(rmu * rmu - r * r + kTop * kTop);
    f3 transmittance, sky;
    bool outside = false;
    if (dtop > 0.0f) { camera = camera + viewRay * dtop; r = kTop; rmu += dtop; }
    else if (r > kTop) outside = true;
    if (outside) { transmittance = mk3(1.0f, 1.0f, 1.0f); sky = mk3(0.0f, 0.0f, 0.0f); }
    else {
        float mu = rmu / r;
        float mu_s = dot(camera, sunDir) / r;
        float nu = dot(viewRay, sunDir);
        bool hitsGround = ray_hits_ground(r, mu);
        transmittance = hitsGround ? mk3(0.0f, 0.0f, 0.0f) : transmittance_to_top(s, r, mu);
        f3 mie;
        f3 scat = combined_scattering(s, r, mu, mu_s, nu, hitsGround, mie);
        sky = scat * rayleigh_phase(nu) + mie * mie_phase(kMieG, nu);
    }
    if (addSunDisk) {
        float nu = dot(viewRay, sunDir);
        if (nu > hrt_cos(kSunAngularRadius)) {
            float den = HRT_PI * kSunAngularRadius * kSunAngularRadius;
            f3 si = solar_irradiance();
            sky = sky + mk3(si.x / den, si.y / den, si.z / den) * transmittance;
        }
    }
    return sky * sunIntensity;
}
} // namespace atm

} // namespace hrt
