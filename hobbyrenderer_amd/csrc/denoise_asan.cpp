// denoise_asan.cpp -- driver of the sanitizer build of the denoise stage's host side (`make denoise_asan`: AddressSanitizer + UBSan, CPU only).
// Runs pt_denoise.h through denoise_host over exactly sized heap images (the noise tile included) with random radii up to the largest the
// context call can reach and random frames, so that taps cross every image edge; hostile values (NaN, inf, huge, zero and negative depth,
// negative radiance and age) sprinkled in; with the default and a caller tile, with and without the colour pair, in place, three chained
// passes with a doubling radius, nthreads 1-3. Any out-of-bounds read, undefined float -> int conversion or other report ends the program
// with a non-zero status.   usage: denoise_asan [seed]
#include "asan_common.h"
#include "pt_denoise.h"

namespace hrt {
void denoise_host(const HrptDenoiseImages& images, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                  const HrptDenoiseParams& params, int nthreads);
}

static int run(int w, int h, bool hostile)
{
    const size_t n = (size_t)w * h * 4;
    std::vector<float> input(n), depth(n), normal(n), geo(n), color(n), outA(n), outB(n), colorOut(n), tile(hrt::denoise::kNoiseFloats);
    for (float& t : tile) t = rnd();
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t i = ((size_t)y * w + x) * 4;
            const bool miss = (w > 2 && x == 0) || (h > 3 && y == h - 1) || rnd() < 0.05f;
            const float vd = 0.3f + 0.05f * (float)x + ((x > w / 3 && x < 2 * w / 3 && y > h / 3) ? 4.0f : 0.0f);   // near geometry: the disk reaches radius * 4
            input[i] = 4.0f * rnd(); input[i + 1] = rnd(); input[i + 2] = 0.25f * rnd(); input[i + 3] = 300.0f * rnd() * rnd();
            depth[i] = miss ? 1e10f : vd; depth[i + 1] = miss ? 1e10f : vd; depth[i + 2] = rnd(); depth[i + 3] = rnd();
            normal[i] = 0.0f; normal[i + 1] = 0.6f; normal[i + 2] = -0.8f; normal[i + 3] = rnd();
            geo[i] = 0.0f; geo[i + 1] = 0.6f; geo[i + 2] = -0.8f; geo[i + 3] = rnd() < 0.5f ? 0.0f : 1.0f;
            color[i] = rnd(); color[i + 1] = rnd(); color[i + 2] = rnd(); color[i + 3] = rnd();
            if (hostile && rnd() < 0.1f) {
                float* planes[] = { input.data(), depth.data(), normal.data(), geo.data() };
                planes[(int)(rnd() * 3.999f)][i + (int)(rnd() * 3.999f)] = kBad[(int)(rnd() * 7.999f)];
            }
        }
    if (hostile) for (size_t i = 0; i < tile.size(); i += 5) if (rnd() < 0.05f) tile[i] = rnd() < 0.5f ? kNan : -3e38f;
    const HrptPlanarViewConstants view = make_view(w, h);
    int calls = 0;
    for (int variant = 0; variant < 4; ++variant) {
        HrptDenoiseParams p;
        std::memset(&p, 0, sizeof p);
        p.radius = 0.25f + 12.0f * rnd(); p.phi = 0.5f; p.lumaPhi = 5.0f; p.depthPhi = 2.0f; p.normalPhi = 50.0f; p.roughnessPhi = 50.0f; p.iterations = 1;
        const uint32_t frame = variant == 3 ? 0xFFFFFFFFu : (uint32_t)(rnd() * 100000.0f);
        const float* src = input.data();
        for (int pass = 0; pass < 3; ++pass) {
            HrptDenoiseImages img;
            std::memset(&img, 0, sizeof img);
            float* dst = (pass & 1) ? outB.data() : outA.data();
            img.input = src; img.depth = depth.data(); img.normal = normal.data(); img.geoNormal = geo.data();
            img.noise = (variant & 1) ? tile.data() : nullptr;
            img.output = dst;
            if (variant >= 1) { img.color = color.data(); img.colorOut = variant == 2 ? color.data() : colorOut.data(); }
            HrptDenoiseParams q = p;
            q.radius = p.radius * (float)(1u << pass); q.frame = frame * 3u + (uint32_t)pass;
            hrt::denoise_host(img, (uint32_t)w, (uint32_t)h, view, q, 1 + (calls % 3));
            ++calls;
            src = dst;
        }
    }
    return calls;
}

int main(int argc, char** argv)
{
    seed_from(argc, argv);
    int calls = 0;
    for (const auto& s : kSizes)
        for (int hostile = 0; hostile < 2; ++hostile)
            calls += run(s[0], s[1], hostile != 0);
    std::printf("denoise_asan: %d calls, no report\n", calls);
    return 0;
}
