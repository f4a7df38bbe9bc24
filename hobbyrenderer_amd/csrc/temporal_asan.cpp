// temporal_asan.cpp -- driver of the sanitizer build of the temporal stage's host side (`make temporal_asan`: AddressSanitizer + UBSan, CPU only).
// Runs pt_temporal.h through temporal_host over exactly sized heap images with a per-pixel random motion field of +-`reach` pixels (taps over
// every image edge, reprojection outside [0, 1]), hostile values (NaN, inf, huge motion, zero and negative depth) sprinkled in, in both
// colour spaces, with and without history, three chained frames. Any out-of-bounds read, undefined float -> int conversion or other report
// ends the program with a non-zero status.   usage: temporal_asan [seed]
#include "asan_common.h"
#include "pt_temporal.h"

namespace hrt {
void temporal_host(const HrptTemporalImages& images, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                   const HrptPlanarViewConstants& prevView, const HrptTemporalParams& params, int nthreads);
}

static int run(int w, int h, float reach, bool hostile)
{
    const size_t n = (size_t)w * h * 4;
    std::vector<float> color(n), motion(n), depth(n), normal(n), histA(n), histB(n), out(n);
    int calls = 0;
    for (int frame = 0; frame < 3; ++frame) {
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t i = ((size_t)y * w + x) * 4;
                const bool miss = x == 0 || y == h - 1 || rnd() < 0.05f;
                const float vd = 2.0f + 0.05f * (float)x + ((x > w / 3 && x < 2 * w / 3 && y > h / 3) ? -1.0f : 0.0f);
                color[i] = 4.0f * rnd(); color[i + 1] = rnd(); color[i + 2] = 0.25f * rnd(); color[i + 3] = 1.0f;
                motion[i] = (2.0f * rnd() - 1.0f) * reach; motion[i + 1] = (2.0f * rnd() - 1.0f) * reach; motion[i + 2] = 0.0f; motion[i + 3] = miss ? 0.0f : 1.0f;
                depth[i] = miss ? 1e10f : vd; depth[i + 1] = miss ? 1e10f : vd; depth[i + 2] = rnd(); depth[i + 3] = rnd();
                normal[i] = 0.0f; normal[i + 1] = 0.6f; normal[i + 2] = -0.8f; normal[i + 3] = 0.5f;
                if (hostile && rnd() < 0.1f) {
                    float* planes[] = { color.data(), motion.data(), depth.data(), normal.data() };
                    planes[(int)(rnd() * 3.999f)][i + (int)(rnd() * 3.999f)] = kBad[(int)(rnd() * 7.999f)];
                }
            }
        for (uint32_t flags = 0; flags < 2; ++flags)
            for (int jitter = 0; jitter < 2; ++jitter)
                for (int history = 0; history < 2; ++history) {
                    const HrptPlanarViewConstants view = make_view(w, h, 0.25f, -0.125f), prev = make_view(w, h, jitter ? -0.3f : 0.25f, jitter ? 0.4f : -0.125f);
                    HrptTemporalParams p; p.blend = 0.9f; p.flags = flags; p.reserved[0] = p.reserved[1] = 0;
                    HrptTemporalImages img;
                    img.color = color.data(); img.motion = motion.data(); img.depth = depth.data(); img.normal = normal.data();
                    img.historyIn = (history && frame > 0) ? histA.data() : nullptr; img.historyOut = histB.data(); img.colorOut = out.data();
                    hrt::temporal_host(img, (uint32_t)w, (uint32_t)h, view, prev, p, 1 + (calls % 3));
                    ++calls;
                }
        histA.swap(histB);
        if (hostile) for (size_t i = 0; i < n; i += 7) if (rnd() < 0.02f) histA[i] = (rnd() < 0.5f) ? kNan : kInf;
    }
    return calls;
}

int main(int argc, char** argv)
{
    seed_from(argc, argv);
    int calls = 0;
    for (const auto& s : kSizes)
        for (int hostile = 0; hostile < 2; ++hostile) {
            calls += run(s[0], s[1], 4.0f, hostile != 0);
            calls += run(s[0], s[1], 0.9f, hostile != 0);
        }
    std::printf("temporal_asan: %d calls, no report\n", calls);
    return 0;
}
