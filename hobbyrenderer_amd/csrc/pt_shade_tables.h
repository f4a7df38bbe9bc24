// pt_shade_tables.h -- the attribute records of a hit triangle unpacked, and where the shading path reads its three small tables from.
#pragma once

#include "pt_traverse.h"

namespace hrt {

// ------------------------------------------------------------------ triangle attributes
// What GetTriangleVertices + UnpackVertex (RaytracingCommon.hlsli:33-50, MeshCommon.hlsli:9-22) yield for a hit,
// read from the per-triangle record built at upload (the quantised vertex / index buffers are consumed there).
struct TriVerts { f3 n0, n1, n2; f2 uv0, uv1, uv2; uint32_t material, inst; };
HRT_DEV TriVerts unpack_tri_attr(const float4* p)      // one GpuTriAttr record
{
    float4 a = p[0], b = p[1], c = p[2], d = p[3], e = p[4];
    TriVerts t;
    t.n0 = mk3(a.x, a.y, a.z); t.n1 = mk3(a.w, b.x, b.y); t.n2 = mk3(b.z, b.w, c.x);
    t.uv0.x = c.y; t.uv0.y = c.z; t.uv1.x = c.w; t.uv1.y = d.x; t.uv2.x = d.y; t.uv2.y = d.z;
    t.material = __float_as_uint(d.w); t.inst = __float_as_uint(e.x);
    return t;
}
HRT_DEV TriVerts load_tri_attr(const SceneView& s, uint32_t tri) { return unpack_tri_attr(reinterpret_cast<const float4*>(s.attrs + tri)); }
// ... for a committed hit: with the two-level structure the record is per MESH triangle and the instance (hence the material) comes
// from the hit
HRT_DEV TriVerts load_hit_attr(const SceneView& s, const Hit& hit)
{
    TriVerts tv = load_tri_attr(s, hit.tri);
    if (s.instances) { tv.inst = hit.inst; tv.material = s.instances[hit.inst].material; }
    return tv;
}
// GetInterpolatedUV, RaytracingCommon.hlsli:79-89
HRT_DEV f2 interpolated_uv(const TriVerts& tv, float bx, float by)
{
    float w0 = (1.0f - bx) - by; f2 r;
    r.x = (tv.uv0.x * w0 + tv.uv1.x * bx) + tv.uv2.x * by;
    r.y = (tv.uv0.y * w0 + tv.uv1.y * bx) + tv.uv2.y * by;
    return r;
}
// TransformNormal, Common.hlsli:33-47
HRT_DEV f3 transform_normal(f3 n, const GpuInstShade& is)
{
    // adjugate rows cross(r1,r2), cross(r2,r0), cross(r0,r1) are precomputed per instance with the same arithmetic
    f3 a0 = mk3(is.adj0.x, is.adj0.y, is.adj0.z), a1 = mk3(is.adj1.x, is.adj1.y, is.adj1.z), a2 = mk3(is.adj2.x, is.adj2.y, is.adj2.z);
    f3 o = mk3((n.x * a0.x + n.y * a1.x) + n.z * a2.x,
               (n.x * a0.y + n.y * a1.y) + n.z * a2.y,
               (n.x * a0.z + n.y * a1.z) + n.z * a2.z);
    return normalize(o);
}

// ------------------------------------------------------------------ where the shading path reads its three small tables
// shade_surface_a (pt_path.h) gathers, per lane, the hit triangle's GpuTriAttr, its instance's GpuInstShade and its material's
// HrptMaterialConstants. It takes one of these accessors, the way traversal takes LdsBvh / GlobalBvh4:
//   GlobalShadeTables  the arrays of the SceneView (every kernel but wf_shade_lt)
//   LdsShadeTables     a block's copy of the three arrays in LDS, whole records in their global layout (pt_wavefront.hip copy_shade_tables).
//                      Records are addressed by 32-bit LDS byte addresses through address_space(3) pointers so that the reads are ds_read_*:
//                      a generic pointer into LDS would become flat_load, which takes the vector-memory path the copy exists to avoid.
struct GlobalShadeTables {
    const SceneView& s;
    HRT_DEV TriVerts hit_attr(const Hit& hit) const { return load_hit_attr(s, hit); }
    HRT_DEV const GpuInstShade& inst_shade(uint32_t inst) const { return s.instShade[inst]; }
    HRT_DEV const HrptMaterialConstants& material(uint32_t material) const { return s.materials[material]; }
};
struct LdsShadeTables {
    typedef __attribute__((address_space(3))) const char* LdsPtr;
    uint32_t attrs, instShade, materials;      // LDS byte address of each table (16-byte aligned)
    template <class T> HRT_DEV const T& at(uint32_t address) const { return *reinterpret_cast<const T*>((const char*)(LdsPtr)(uintptr_t)address); }
    // (flat structure only: the record holds the instance and the material, load_hit_attr's two-level branch does not apply)
    HRT_DEV TriVerts hit_attr(const Hit& hit) const { return unpack_tri_attr(&at<float4>(attrs + hit.tri * (uint32_t)sizeof(GpuTriAttr))); }
    HRT_DEV const GpuInstShade& inst_shade(uint32_t inst) const { return at<GpuInstShade>(instShade + inst * (uint32_t)sizeof(GpuInstShade)); }
    HRT_DEV const HrptMaterialConstants& material(uint32_t material) const { return at<HrptMaterialConstants>(materials + material * (uint32_t)sizeof(HrptMaterialConstants)); }
};

} // namespace hrt
