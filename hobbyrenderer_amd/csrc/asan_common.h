// asan_common.h -- what the drivers of the stages' sanitizer builds share (temporal_asan.cpp, denoise_asan.cpp, modulation_asan.cpp): the
// random stream, a plausible view, the table of hostile values and the image sizes. Each driver stays a program of its own and decides what
// it feeds its stage; the same seed gives the same draws as before the table and the stream were shared.
#pragma once

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/hobbyrt_pt.h"
#include "../../include/hobbyrt/detmath.h"

static uint32_t g_state = 1;
static float rnd() { g_state = hrt_pcg_hash(g_state); return (float)(g_state >> 8) * (1.0f / 16777216.0f); }
static void seed_from(int argc, char** argv) { g_state = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 1u; }     // usage: NAME [seed]

static const float kNan = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();
static const float kBad[8] = { kNan, kInf, -kInf, 3e38f, -3e38f, 0.0f, -1.0f, 1e-42f };
// 1 x 1, smaller than a tap footprint, odd, and a multiple of nothing in particular
static const int kSizes[4][2] = { { 1, 1 }, { 2, 3 }, { 37, 23 }, { 64, 36 } };

// A w x h view from the origin of the world with the pixel offset (ox, oy)
static HrptPlanarViewConstants make_view(int w, int h, float ox = 0.0f, float oy = 0.0f)
{
    HrptPlanarViewConstants v;
    std::memset(&v, 0, sizeof v);
    const float n = 0.1f, sx = 1.2f, sy = 1.2f * (float)w / (float)h;
    float* P = v.m_MatViewToClip;                   // reversed-Z, infinite far plane
    P[0] = sx; P[5] = sy; P[11] = 1.0f; P[14] = n;
    float* M = v.m_MatClipToWorld;                  // its inverse (camera at the origin of the world)
    M[0] = 1.0f / sx; M[5] = 1.0f / sy; M[11] = 1.0f / n; M[14] = 1.0f;
    v.m_ViewportSize[0] = (float)w; v.m_ViewportSize[1] = (float)h;
    v.m_ViewportSizeInv[0] = 1.0f / (float)w; v.m_ViewportSizeInv[1] = 1.0f / (float)h;
    v.m_PixelOffset[0] = ox; v.m_PixelOffset[1] = oy;
    v.m_CameraDirectionOrPosition[3] = 1.0f;
    return v;
}
