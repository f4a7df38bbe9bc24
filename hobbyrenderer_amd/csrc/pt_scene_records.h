// pt_scene_records.h -- the records of an uploaded scene as the kernels read them, and SceneView; plain structs and, next to GpuNodeQ, the
// decode of its planes (host units include this header alone; pt_record_layout.h ties the records to the Host* ones of bvh_build.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hobbyrt_pt.h"

namespace hrt {

// ------------------------------------------------------------------ device scene view
struct GpuNode {            // 64 B: both child boxes live in the parent -> one 64 B read per step
    float lmin[3]; int32_t left;    // child >= 0: inner node index; child < 0: leaf = ~((first << 2) | (count - 1))
    float lmax[3]; int32_t right;
    float rmin[3]; uint32_t pad0;
    float rmax[3]; uint32_t pad1;
};
struct GpuNode4 {           // 128 B: four child boxes in SoA + four child refs (bvh_build.h HostNode4); empty slot = far-away box
    float4 minx, maxx, miny, maxy, minz, maxz; int4 child; uint4 pad;     // rows at byte 0, 16, ..., 80; child refs at 96
};
// 64 B: the same four child boxes as a GpuNode4, quantised to 8 bits per plane relative to the node's own extent (origin = min corner of the
// union of the child boxes, one fp32 step per axis), rounded OUTWARD (and checked against the decode arithmetic), so a decoded box contains the fp32 box it came
// from (hrpt_selftest_bvh checks every node). What it buys: a lane's node fetch is 4 sixteen-byte requests instead of 7, and the L1 (TCP)
// of a CU looks up about ONE lane-request per cycle whatever the request's width -- the traversal kernels on trees in global memory are
// bound by exactly that rate (scripts/microbench/gather_nodes.hip; three more requests per step cost config 4's wf_extend +45 %).
// Culling only: the hit definition never depends on the boxes. Rows: {ox, oy, oz, sx} {lo_x, hi_x, lo_y, hi_y}
// {lo_z, hi_z, sy, sz} {child[4]}; byte c of a plane word belongs to child c; an unused slot has lo = 255 > hi = 0 on every axis.
struct GpuNodeQ {
    float ox, oy, oz, sx;
    uint32_t lox, hix, loy, hiy;
    uint32_t loz, hiz; float sy, sz;
    int32_t child[4];
};
static_assert(sizeof(GpuNodeQ) == 64, "four 16-byte rows");
// The decode of a plane: byte q of an axis with origin o and step s, and the byte of child c in a plane word (lo_* or hi_*) of that axis.
// The quantiser rounds against this arithmetic and hrpt_selftest_bvh checks it (pt_bvh_nodes.hip); inner_step (pt_traverse.h) folds the
// same o + q * s into the ray's plane distances.
__host__ __device__ inline float node_q_decode(float o, float s, uint32_t q) { return o + (float)q * s; }
__host__ __device__ inline float node_q_plane(float o, float s, uint32_t word, int c) { return node_q_decode(o, s, (word >> (8 * c)) & 255u); }
struct GpuTri {             // 48 B world-space triangle (instance transform applied at upload)
    float p0[3]; uint32_t inst;
    float p1[3]; uint32_t prim;
    float p2[3]; uint32_t flags;    // bit 0: instance is ForceOpaque (src/Scene.cpp:150-154)
};
// Per-triangle shading attributes, unpacked once at upload (bvh_build.h HostTriAttr), and per-instance adjugate rows.
struct GpuTriAttr { float4 a, b, c, d, e; };   // a{n0,n1.x} b{n1.yz,n2.xy} c{n2.z,uv0,uv1.x} d{uv1.y,uv2,material} e{inst,prim,-,-}
struct GpuTriTangent { float4 t0, t1, t2; };
struct GpuInstShade { float4 adj0, adj1, adj2; };
// Two-level structure (bvh_build.h HostInstance): one record per instance, 128 B
struct GpuInstance {
    float world[12];            // m_World rows 0..3, xyz each
    float inv[12];              // inverse map, same layout (only the 3x3 part is read on the device)
    int32_t blasRoot; uint32_t flags, material; float boxEps;
    uint32_t mesh; float objMaxAbs, invNorm; uint32_t pad;
};
struct GpuTexture {         // decoded texels of all levels (HrptTextureDesc); level l starts mipOffset[l] TEXELS after `texels`
    const uint8_t* texels; uint32_t w, h, format, mipCount;
    uint32_t mipOffset[HRPT_TEXTURE_MAX_MIPS];
};

struct SceneView {
    const GpuNode* nodes; uint32_t nodeCount;
    const GpuNode4* nodes4; uint32_t node4Count;   // the same tree collapsed to 4-wide nodes (wavefront kernels); root = 0
    const GpuNodeQ* nodesQ;                         // nodes4 in the 64-byte quantised form, same indices (flat structure only; null otherwise)
    const GpuTri* tris; uint32_t triCount;
    int32_t rootLeaf;       // when the whole scene fits one leaf: encoded leaf, else 0
    const GpuTriAttr* attrs;            // parallel to tris
    const GpuTriTangent* tangents;      // parallel to tris, or null when no material samples a normal map
    const GpuInstShade* instShade;      // per instance
    const HrptMaterialConstants* materials;
    const HrptGPULight* lights; uint32_t lightCount;
    const GpuTexture* textures; uint32_t textureCount;
    const uint16_t* lutTransmittance;   // 256 x 64 RGBA16F
    const uint16_t* lutScattering;      // 256 x 128 x 32 RGBA16F
    // two-level structure (instanced scenes; null = the flat world-space tree above): nodes4 then holds the tree over the instances
    // (root 0, leaves ~(instance << 2)) followed by the object-space trees of the distinct meshes, tris / attrs / tangents are per MESH
    // triangle (object space), and a hit carries its instance next to the triangle index.
    const GpuInstance* instances; uint32_t instanceCount;
};

} // namespace hrt
