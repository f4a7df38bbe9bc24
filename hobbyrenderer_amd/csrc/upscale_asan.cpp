// upscale_asan.cpp -- driver of the sanitizer build of the upscale stage's host side (`make upscale_asan`: AddressSanitizer + UBSan, CPU only).
// Runs pt_upscale.h through upscale_host over exactly sized heap images at scale ratios from 1 to 4 (integer and not, per axis), with a
// per-texel random motion field of +-`reach` render pixels (history taps over every image edge, reprojection outside [0, 1]), jitter at and
// inside its limits, hostile values (NaN, inf, huge motion, zero and negative depth) sprinkled in, with and without history and clamp, three
// chained frames. Any out-of-bounds read, undefined float -> int conversion or other report ends the program with a non-zero status.
// usage: upscale_asan [seed]
#include "asan_common.h"
#include "pt_upscale.h"

namespace hrt {
void upscale_host(const HrptUpscaleImages& images, uint32_t width, uint32_t height, uint32_t displayWidth, uint32_t displayHeight,
                  const HrptPlanarViewConstants& view, const HrptPlanarViewConstants& prevView, const HrptUpscaleParams& params, int nthreads);
}

static int run(int w, int h, int W, int H, float reach, bool hostile)
{
    const size_t n = (size_t)w * h * 4, N = (size_t)W * H * 4;
    std::vector<float> color(n), depth(n), motion(n), histA(N), histB(N), out(N);
    static const float kJitter[4][2] = { { 0.0f, 0.0f }, { 0.5f, -0.5f }, { -0.5f, 0.5f }, { 0.3125f, -0.4375f } };
    int calls = 0;
    for (int frame = 0; frame < 3; ++frame) {
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t i = ((size_t)y * w + x) * 4;
                const bool miss = (w > 2 && x < 2) || y == h - 1 || rnd() < 0.05f;
                const float vd = 2.0f + 0.05f * (float)x + ((x > w / 3 && x < 2 * w / 3 && y > h / 3) ? -1.0f : 0.0f);
                color[i] = 4.0f * rnd(); color[i + 1] = rnd(); color[i + 2] = 0.25f * rnd(); color[i + 3] = rnd();
                motion[i] = (2.0f * rnd() - 1.0f) * reach; motion[i + 1] = (2.0f * rnd() - 1.0f) * reach; motion[i + 2] = 0.0f; motion[i + 3] = miss ? 0.0f : 1.0f;
                depth[i] = miss ? 1e10f : vd; depth[i + 1] = miss ? 1e10f : vd; depth[i + 2] = rnd(); depth[i + 3] = rnd();
                if (hostile && rnd() < 0.1f) {
                    float* planes[] = { color.data(), depth.data(), motion.data() };
                    planes[(int)(rnd() * 2.999f)][i + (int)(rnd() * 3.999f)] = kBad[(int)(rnd() * 7.999f)];
                }
            }
        for (uint32_t flags = 0; flags < 2; ++flags)
            for (int jitter = 0; jitter < 4; ++jitter)
                for (int history = 0; history < 2; ++history) {
                    const HrptPlanarViewConstants view = make_view(w, h, 0.25f, -0.125f), prev = make_view(w, h, jitter ? -0.3f : 0.25f, jitter ? 0.4f : -0.125f);
                    HrptUpscaleParams p;
                    p.jitter[0] = kJitter[jitter][0]; p.jitter[1] = kJitter[jitter][1];
                    p.kernel = jitter == 3 ? 16.0f : 2.29f; p.maxHistory = jitter == 2 ? 0.0f : 8.0f; p.flags = flags;
                    p.reserved[0] = p.reserved[1] = p.reserved[2] = 0;
                    HrptUpscaleImages img;
                    img.color = color.data(); img.depth = depth.data(); img.motion = motion.data();
                    img.historyIn = (history && frame > 0) ? histA.data() : nullptr; img.historyOut = histB.data(); img.colorOut = out.data();
                    hrt::upscale_host(img, (uint32_t)w, (uint32_t)h, (uint32_t)W, (uint32_t)H, view, prev, p, 1 + (calls % 3));
                    ++calls;
                }
        histA.swap(histB);
        if (hostile) for (size_t i = 0; i < N; i += 7) if (rnd() < 0.02f) histA[i] = (rnd() < 0.5f) ? kNan : kInf;
    }
    return calls;
}

int main(int argc, char** argv)
{
    seed_from(argc, argv);
    // display size per render size: 1x, 2x, 4x, non-integer, and a different ratio per axis
    static const float kScale[5][2] = { { 1.0f, 1.0f }, { 2.0f, 2.0f }, { 4.0f, 4.0f }, { 1.5f, 1.5f }, { 3.0f, 1.0f } };
    int calls = 0;
    for (const auto& s : kSizes)
        for (const auto& k : kScale) {
            const int W = (int)((float)s[0] * k[0]), H = (int)((float)s[1] * k[1]);
            for (int hostile = 0; hostile < 2; ++hostile) {
                calls += run(s[0], s[1], W, H, 4.0f, hostile != 0);
                calls += run(s[0], s[1], W, H, 0.9f, hostile != 0);
            }
        }
    std::printf("upscale_asan: %d calls, no report\n", calls);
    return 0;
}
