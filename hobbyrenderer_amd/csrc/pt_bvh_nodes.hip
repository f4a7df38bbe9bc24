// pt_bvh_nodes.hip -- the two kernels that, besides the traversal (pt_traverse.h inner_step), know the GpuNodeQ encoding
// (pt_scene_records.h): pt_quantise_nodes_kernel, which makes the quantised nodes after every build or refit of the flat tree (production
// code), and pt_bvh_check_kernel, the containment check of hrpt_selftest_bvh over the 2-wide, the 4-wide and the quantised tree. Both decode
// a plane through node_q_decode / node_q_plane.
#include "pt_kernels.h"
#include "pt_scene_records.h"

namespace hrt {

// Self-test of the acceleration structure (hrpt_selftest_bvh): every child box stored in a node must contain what hangs below it -- the
// child's own child boxes when it is an inner node, the vertices of its triangles when it is a leaf. The GPU builder fits boxes bottom-up
// with relaxed agent-scope atomics and write-through stores (bvh_build_gpu.hip k_fit); a stale read there would give a parent box that is
// too small, i.e. silently missed hits, which image parity on a few scenes cannot rule out. One thread per node; violations are counted.
__device__ __forceinline__ bool box_in(const float* mn, const float* mx, const float* cmn, const float* cmx)
{
    return cmn[0] >= mn[0] && cmn[1] >= mn[1] && cmn[2] >= mn[2] && cmx[0] <= mx[0] && cmx[1] <= mx[1] && cmx[2] <= mx[2];
}
__device__ __forceinline__ bool leaf_in(const SceneView& s, int32_t ref, const float* mn, const float* mx)
{
    const uint32_t enc = (uint32_t)(~ref), first = enc >> 2, count = (enc & 3u) + 1u;
    bool ok = first + count <= s.triCount;
    for (uint32_t i = 0; ok && i < count; ++i) {
        const GpuTri& t = s.tris[first + i];
        for (int k = 0; k < 3; ++k)
            ok = ok && t.p0[k] >= mn[k] && t.p0[k] <= mx[k] && t.p1[k] >= mn[k] && t.p1[k] <= mx[k] && t.p2[k] >= mn[k] && t.p2[k] <= mx[k];
    }
    return ok;
}
__global__ void pt_bvh_check_kernel(SceneView s, unsigned long long* violations)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned int bad = 0;
    if (i < s.nodeCount) {                              // 2-wide tree
        const GpuNode& n = s.nodes[i];
        const float* mn[2] = { n.lmin, n.rmin }; const float* mx[2] = { n.lmax, n.rmax }; const int32_t ref[2] = { n.left, n.right };
        for (int c = 0; c < 2; ++c) {
            if (ref[c] >= 0) {
                if ((uint32_t)ref[c] >= s.nodeCount) { ++bad; continue; }
                const GpuNode& m = s.nodes[ref[c]];
                if (!box_in(mn[c], mx[c], m.lmin, m.lmax) || !box_in(mn[c], mx[c], m.rmin, m.rmax)) ++bad;
            } else if (!leaf_in(s, ref[c], mn[c], mx[c])) ++bad;
        }
    }
    if (i < s.node4Count) {                             // its 4-wide collapse
        const GpuNode4& n = s.nodes4[i];
        const float* r[6] = { &n.minx.x, &n.miny.x, &n.minz.x, &n.maxx.x, &n.maxy.x, &n.maxz.x };
        const int32_t* ch = &n.child.x;
        for (int c = 0; c < 4; ++c) {
            if (ch[c] == 0x7fffffff) continue;          // unused slot
            const float mn[3] = { r[0][c], r[1][c], r[2][c] }, mx[3] = { r[3][c], r[4][c], r[5][c] };
            if (ch[c] >= 0) {
                if ((uint32_t)ch[c] >= s.node4Count) { ++bad; continue; }
                const GpuNode4& m = s.nodes4[ch[c]];
                const float* q[6] = { &m.minx.x, &m.miny.x, &m.minz.x, &m.maxx.x, &m.maxy.x, &m.maxz.x };
                const int32_t* mch = &m.child.x;
                for (int k = 0; k < 4; ++k) {
                    if (mch[k] == 0x7fffffff) continue;
                    const float cmn[3] = { q[0][k], q[1][k], q[2][k] }, cmx[3] = { q[3][k], q[4][k], q[5][k] };
                    if (!box_in(mn, mx, cmn, cmx)) ++bad;
                }
            } else if (!leaf_in(s, ch[c], mn, mx)) ++bad;
        }
    }
    if (s.nodesQ && i < s.node4Count) {                 // ... and its quantised form: every decoded box contains the fp32 box it was made from
        const GpuNode4& n = s.nodes4[i]; const GpuNodeQ& q = s.nodesQ[i];
        const float* r[6] = { &n.minx.x, &n.miny.x, &n.minz.x, &n.maxx.x, &n.maxy.x, &n.maxz.x };
        const float o[3] = { q.ox, q.oy, q.oz }, st[3] = { q.sx, q.sy, q.sz };
        const uint32_t lo[3] = { q.lox, q.loy, q.loz }, hi[3] = { q.hix, q.hiy, q.hiz };
        const int32_t* ch = &n.child.x;
        for (int c = 0; c < 4; ++c) {
            if (q.child[c] != ch[c]) ++bad;
            for (int a = 0; a < 3; ++a) {
                const float dlo = node_q_plane(o[a], st[a], lo[a], c), dhi = node_q_plane(o[a], st[a], hi[a], c);
                if (ch[c] == 0x7fffffff) { if (!(dlo > dhi)) ++bad; }                 // unused slot: an empty interval on every axis
                else if (!(dlo <= r[a][c] && dhi >= r[3 + a][c]) || !(st[a] > 0.0f)) ++bad;
            }
        }
    }
    if (bad) atomicAdd(violations, (unsigned long long)bad);
}
hipError_t launch_bvh_check(const SceneView& scene, unsigned long long* violations, hipStream_t stream)
{
    const uint32_t n = scene.nodeCount > scene.node4Count ? scene.nodeCount : scene.node4Count;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(pt_bvh_check_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, scene, violations);
    return hipGetLastError();
}

// GpuNode4 -> GpuNodeQ (see pt_scene_records.h), one thread per node; run after every build / rebuild of the flat structure, whichever builder made it.
__global__ void pt_quantise_nodes_kernel(const GpuNode4* __restrict__ in, uint32_t count, GpuNodeQ* __restrict__ out, double* __restrict__ leafArea)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const GpuNode4 n = in[i];
    const float* r[6] = { &n.minx.x, &n.miny.x, &n.minz.x, &n.maxx.x, &n.maxy.x, &n.maxz.x };
    const int32_t* ch = &n.child.x;
    float o[3], st[3]; uint32_t lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        float mn = 3.0e38f, mx = -3.0e38f;
        for (int c = 0; c < 4; ++c) if (ch[c] != 0x7fffffff) { mn = fminf(mn, r[a][c]); mx = fmaxf(mx, r[3 + a][c]); }
        // 254 steps span the extent (the top plane may still need one step outward after rounding)
        float step = (mx - mn) * (1.0f / 254.0f) * 1.000001f;
        step = fmaxf(step, fmaxf(fabsf(mn), fabsf(mx)) * 2.4e-7f);       // never below two ulps of the coordinates: the slack must outweigh the rounding of o + q * s
        step = fmaxf(step, 1.0e-30f);
        o[a] = mn; st[a] = step; lo[a] = 0u; hi[a] = 0u;
        for (int c = 0; c < 4; ++c) {
            uint32_t ql = 255u, qh = 0u;
            if (ch[c] != 0x7fffffff) {
                float fl = floorf((r[a][c] - mn) / step), fh = ceilf((r[3 + a][c] - mn) / step);
                fl = fminf(fmaxf(fl, 0.0f), 255.0f); fh = fminf(fmaxf(fh, 0.0f), 255.0f);
                ql = (uint32_t)fl; qh = (uint32_t)fh;
                // the decode itself (the one the self-test uses): step outward until the decoded plane is on the right side (at most a step or two)
                while (ql > 0u && !(node_q_decode(mn, step, ql) <= r[a][c])) --ql;
                while (qh < 255u && !(node_q_decode(mn, step, qh) >= r[3 + a][c])) ++qh;
            }
            lo[a] |= ql << (8 * c); hi[a] |= qh << (8 * c);
        }
    }
    // what the rounding costs: surface area of the LEAF boxes before and after (the chance that a ray enters a box grows with its area, and
    // every entered leaf is three requests and a watertight test per triangle): leafArea[0] += fp32 area, leafArea[1] += decoded area
    if (leafArea) {
        double a0 = 0.0, a1 = 0.0, r0 = 0.0, r1 = 0.0;
        for (int c = 0; c < 4; ++c) {
            if (ch[c] == 0x7fffffff || ch[c] >= 0) continue;
            float e0[3], e1[3];
            for (int a = 0; a < 3; ++a) {
                e0[a] = r[3 + a][c] - r[a][c];
                e1[a] = node_q_plane(o[a], st[a], hi[a], c) - node_q_plane(o[a], st[a], lo[a], c);
            }
            const double s0 = (double)e0[0] * e0[1] + (double)e0[1] * e0[2] + (double)e0[2] * e0[0], s1 = (double)e1[0] * e1[1] + (double)e1[1] * e1[2] + (double)e1[2] * e1[0];
            a0 += s0; a1 += s1;
            if (s0 > 0.0) { r0 += s1 / s0; r1 += 1.0; }
        }
        if (a0 > 0.0 || a1 > 0.0) { atomicAdd(&leafArea[0], a0); atomicAdd(&leafArea[1], a1); atomicAdd(&leafArea[2], r0); atomicAdd(&leafArea[3], r1); }
    }
    GpuNodeQ q;
    q.ox = o[0]; q.oy = o[1]; q.oz = o[2]; q.sx = st[0]; q.sy = st[1]; q.sz = st[2];
    q.lox = lo[0]; q.hix = hi[0]; q.loy = lo[1]; q.hiy = hi[1]; q.loz = lo[2]; q.hiz = hi[2];
    for (int c = 0; c < 4; ++c) q.child[c] = ch[c];
    out[i] = q;
}
hipError_t launch_quantise_nodes(const GpuNode4* nodes4, uint32_t count, GpuNodeQ* out, double* leafArea, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(pt_quantise_nodes_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, nodes4, count, out, leafArea);
    return hipGetLastError();
}

} // namespace hrt
