// pt_denoise_host.cpp -- the host-thread executor of the denoise stage (hrpt_denoise_host): pt_denoise.h's per-pixel function over rows, the
// default noise tile and the parameter rules. Plain C++ with no HIP call, so that the sanitizer program (denoise_asan.cpp,
// `make denoise_asan`) builds it with g++ as it is.
#include <cmath>

#include "pt_denoise.h"
#include "pt_host_rows.h"

namespace hrt {

size_t denoise_noise_floats() { return denoise::kNoiseFloats; }

void denoise_default_tile(float* tile)
{
    for (int y = 0; y < denoise::kNoiseSize; ++y)
        for (int x = 0; x < denoise::kNoiseSize; ++x)
            denoise::default_tile_texel(x, y, tile + ((size_t)y * denoise::kNoiseSize + x) * 2);
}

bool denoise_params_valid(const HrptDenoiseParams& p)
{
    const float f[6] = { p.radius, p.phi, p.lumaPhi, p.depthPhi, p.normalPhi, p.roughnessPhi };
    for (float x : f) if (!std::isfinite(x)) return false;
    if (!(p.radius > 0.0f && p.phi > 0.0f && p.lumaPhi >= 0.0f && p.depthPhi >= 0.0f && p.normalPhi >= 0.0f && p.roughnessPhi >= 0.0f)) return false;
    if (p.iterations < 1u || p.iterations > 5u) return false;
    if (!std::isfinite(p.radius * (float)(1u << (p.iterations - 1u)))) return false;
    return (p.flags & ~HRPT_DENOISE_OUTPUT_ONLY) == 0u && p.reserved == 0u;
}

// One pass with params.radius and params.frame. colorOut may be color (a pixel reads only its own colour texel and reads it before
// writing); output must not be input (the taps read input texels other rows write).
void denoise_host(const HrptDenoiseImages& images, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                  const HrptDenoiseParams& params, int nthreads)
{
    const denoise::Args a = denoise::make_args(view, params, params.radius, params.frame, (int)width, (int)height);
    std::vector<float> tile;
    const float* noise = images.noise;
    if (!noise) { tile.resize(denoise::kNoiseFloats); denoise_default_tile(tile.data()); noise = tile.data(); }
    const int W = (int)width, H = (int)height;
    over_rows(H, nthreads, [&, noise](int y) {
        for (int x = 0; x < W; ++x) {
            const img::T4 out = denoise::pixel(a, images.input, images.depth, images.normal, images.geoNormal, noise, x, y);
            const size_t i = ((size_t)y * W + x) * 4;
            store4(images.output + i, out);
            if (images.colorOut) store4(images.colorOut + i, img::t4(out.x, out.y, out.z, images.color[i + 3]));     // alpha read before the write
        }
    });
}

} // namespace hrt
