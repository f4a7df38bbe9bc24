// modulation_asan.cpp -- driver of the sanitizer build of the demodulate / compose stages' host side (`make modulation_asan`:
// AddressSanitizer + UBSan, CPU only). Runs pt_modulation.h through demodulate_host, compose_host and modulation_probe over exactly sized heap
// images with random planes and hostile values sprinkled in (NaN, inf, huge, negative albedo, zero normals, view depth 0, negative
// radiance), with and without the emissive image, in place and not, with three floors, nthreads 1-3. Any out-of-bounds access or other
// report ends the program with a non-zero status.   usage: modulation_asan [seed]
#include "asan_common.h"
#include "pt_modulation.h"

namespace hrt {
void demodulate_host(const HrptDemodulateImages& images, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                     const HrptModulationParams& params, int nthreads);
void compose_host(const HrptComposeImages& images, uint32_t width, uint32_t height, int nthreads);
void modulation_probe(const float* albedo3, const float* N3, const float* V3, float rough, float metal, float floor, float* outM3);
}

static int run(int w, int h, bool hostile)
{
    const size_t n = (size_t)w * h * 4;
    std::vector<float> color(n), albedo(n), normal(n), geo(n), depth(n), emissive(n), colorOut(n), modulation(n), composed(n);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t i = ((size_t)y * w + x) * 4;
            const bool miss = (w > 2 && x == 0) || (h > 3 && y == h - 1) || rnd() < 0.05f;
            const float vd = 0.3f + 0.05f * (float)x;
            color[i] = 4.0f * rnd(); color[i + 1] = rnd(); color[i + 2] = 0.25f * rnd(); color[i + 3] = rnd();
            albedo[i] = rnd(); albedo[i + 1] = rnd() < 0.3f ? 0.0f : rnd(); albedo[i + 2] = rnd() < 0.3f ? 1.0f : rnd(); albedo[i + 3] = 1.0f;
            const float nz = rnd() < 0.2f ? (rnd() < 0.5f ? 1.0f : -1.0f) : -0.8f;
            normal[i] = 0.0f; normal[i + 1] = nz == -0.8f ? 0.6f : 0.0f; normal[i + 2] = nz; normal[i + 3] = rnd();
            geo[i] = normal[i]; geo[i + 1] = normal[i + 1]; geo[i + 2] = normal[i + 2]; geo[i + 3] = rnd() < 0.5f ? 0.0f : (rnd() < 0.5f ? 1.0f : rnd());
            depth[i] = miss ? 1e10f : vd; depth[i + 1] = miss ? 1e10f : vd; depth[i + 2] = rnd(); depth[i + 3] = rnd();
            const bool lit = rnd() < 0.05f;
            for (int k = 0; k < 3; ++k) emissive[i + k] = lit ? 2.0f * rnd() * color[i + k] : 0.0f;
            emissive[i + 3] = 1.0f;
            if (hostile && rnd() < 0.15f) {
                float* planes[] = { color.data(), albedo.data(), normal.data(), geo.data(), depth.data(), emissive.data() };
                planes[(int)(rnd() * 5.999f)][i + (int)(rnd() * 3.999f)] = kBad[(int)(rnd() * 7.999f)];
            }
            if (hostile && rnd() < 0.03f) { normal[i] = normal[i + 1] = normal[i + 2] = 0.0f; }      // zero normal
            if (hostile && rnd() < 0.03f) depth[i + 1] = 0.0f;                                        // view depth 0
        }
    const HrptPlanarViewConstants view = make_view(w, h);
    const float floors[3] = { 0.04f, 0.5f, 1e-6f };
    int calls = 0;
    for (int variant = 0; variant < 6; ++variant) {
        HrptModulationParams p;
        std::memset(&p, 0, sizeof p);
        p.floor = floors[variant % 3];
        std::vector<float> work = color;
        const bool inPlace = variant >= 3;
        HrptDemodulateImages img;
        std::memset(&img, 0, sizeof img);
        img.color = inPlace ? work.data() : color.data(); img.albedo = albedo.data(); img.normal = normal.data(); img.geoNormal = geo.data();
        img.depth = depth.data(); img.emissive = (variant & 1) ? emissive.data() : nullptr;
        img.colorOut = inPlace ? work.data() : colorOut.data(); img.modulationOut = modulation.data();
        hrt::demodulate_host(img, (uint32_t)w, (uint32_t)h, view, p, 1 + (calls % 3));
        ++calls;
        HrptComposeImages cimg;
        std::memset(&cimg, 0, sizeof cimg);
        cimg.color = img.colorOut; cimg.modulation = modulation.data(); cimg.emissive = img.emissive;
        cimg.colorOut = inPlace ? work.data() : composed.data();
        hrt::compose_host(cimg, (uint32_t)w, (uint32_t)h, 1 + (calls % 3));
        ++calls;
        if (!hostile)                                  // the floor holds, and a miss has the marker
            for (size_t i = 0; i < n; i += 4) {
                const bool miss = depth[i] == 1e10f;
                for (int k = 0; k < 3; ++k)
                    if (!(modulation[i + k] >= p.floor) || (miss && modulation[i + k] != 1.0f)) { std::fprintf(stderr, "modulation_asan: factor %g below the floor\n", modulation[i + k]); return -1000000; }
                if (modulation[i + 3] != (miss ? 0.0f : 1.0f)) { std::fprintf(stderr, "modulation_asan: wrong marker\n"); return -1000000; }
            }
    }
    for (int k = 0; k < 64; ++k) {                     // the probe, vectors of any kind
        float a[3], N[3], V[3], out[3];
        for (int j = 0; j < 3; ++j) { a[j] = rnd(); N[j] = 2.0f * rnd() - 1.0f; V[j] = 2.0f * rnd() - 1.0f; }
        if (hostile && (k & 3) == 0) N[k % 3] = kBad[k % 8];
        if (hostile && (k & 3) == 1) V[k % 3] = kBad[k % 8];
        if (hostile && (k & 7) == 2) N[0] = N[1] = N[2] = 0.0f;
        hrt::modulation_probe(a, N, V, rnd(), rnd(), floors[k % 3], out);
        ++calls;
    }
    return calls;
}

int main(int argc, char** argv)
{
    seed_from(argc, argv);
    int calls = 0;
    for (const auto& s : kSizes)
        for (int hostile = 0; hostile < 2; ++hostile) {
            const int r = run(s[0], s[1], hostile != 0);
            if (r < 0) return 1;
            calls += r;
        }
    std::printf("modulation_asan: %d calls, no report\n", calls);
    return 0;
}
