// pt_vec.h -- vector algebra of the device code: f2 / f3 / f4 and their operators, in the fixed expression order of pt_device.h. One
// __host__ __device__ source (HRT_FN of hobbyrt/detmath.h): a plain C++ compiler builds it too, for the host executors and sanitizer
// programs of the stages that share device arithmetic (pt_direct.h, pt_deferred.h).
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

#include "../../include/hobbyrt/detmath.h"

namespace hrt {

// ------------------------------------------------------------------ vectors
struct f2 { float x, y; };
struct f3 { float x, y, z; };
struct f4 { float x, y, z, w; };

HRT_FN f3 mk3(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
HRT_FN f3 mk3(const float* p) { return mk3(p[0], p[1], p[2]); }
HRT_FN f3 operator+(f3 a, f3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
HRT_FN f3 operator-(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
HRT_FN f3 operator*(f3 a, f3 b) { return mk3(a.x * b.x, a.y * b.y, a.z * b.z); }
HRT_FN f3 operator*(f3 a, float s) { return mk3(a.x * s, a.y * s, a.z * s); }
HRT_FN f3 operator/(f3 a, float s) { return mk3(a.x / s, a.y / s, a.z / s); }
HRT_FN f3 operator-(f3 a) { return mk3(-a.x, -a.y, -a.z); }
HRT_FN float dot(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
HRT_FN f3 cross(f3 a, f3 b) { return mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
HRT_FN float length(f3 a) { return hrt_sqrt(dot(a, a)); }
HRT_FN f3 normalize(f3 a) { float inv = 1.0f / hrt_sqrt(dot(a, a)); return a * inv; }
HRT_FN float lerp(float a, float b, float t) { return a + t * (b - a); }
HRT_FN float comp(f3 a, int k) { return k == 0 ? a.x : (k == 1 ? a.y : a.z); }
HRT_FN float maxcomp(f3 a) { return hrt_max(a.x, hrt_max(a.y, a.z)); }
HRT_FN f3 reflect(f3 i, f3 n) { float s = 2.0f * dot(i, n); return i - n * s; }
HRT_FN f3 refract(f3 i, f3 n, float eta)
{
    float d = dot(n, i);
    float k = 1.0f - (eta * eta) * (1.0f - d * d);
    if (k < 0.0f) return mk3(0.0f, 0.0f, 0.0f);
    float s = eta * d + hrt_sqrt(k);
    return i * eta - n * s;
}
HRT_FN f4 lerp4(f4 a, f4 b, float t)
{
    f4 r; float w = 1.0f - t;
    r.x = a.x * w + b.x * t; r.y = a.y * w + b.y * t; r.z = a.z * w + b.z * t; r.w = a.w * w + b.w * t;
    return r;
}

} // namespace hrt
