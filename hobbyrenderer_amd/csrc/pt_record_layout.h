// pt_record_layout.h -- the one place that sees both sides of an upload: the Host* records the builders fill (bvh_build.h) and the Gpu*
// records the kernels read (pt_scene_records.h). A Host* array is copied to the device byte for byte and handed to the kernels as an array
// of its Gpu* partner (upload_records in pt_capi_scene.cpp, the only unit that includes this): the asserts below are what makes that cast sound.
#pragma once

#include <cstddef>
#include <type_traits>

#include "bvh_build.h"
#include "pt_scene_records.h"

namespace hrt {

// The Gpu* record a Host* record is read as.
template <class Host> struct GpuRecordOf;
template <> struct GpuRecordOf<HostNode> { using type = GpuNode; };
template <> struct GpuRecordOf<HostNode4> { using type = GpuNode4; };
template <> struct GpuRecordOf<HostTri> { using type = GpuTri; };
template <> struct GpuRecordOf<HostTriAttr> { using type = GpuTriAttr; };
template <> struct GpuRecordOf<HostTriTangent> { using type = GpuTriTangent; };
template <> struct GpuRecordOf<HostInstShade> { using type = GpuInstShade; };
template <> struct GpuRecordOf<HostInstance> { using type = GpuInstance; };

#define HRT_SAME_RECORD(H, G, bytes) \
    static_assert(std::is_same<GpuRecordOf<H>::type, G>::value && sizeof(H) == (bytes) && sizeof(G) == (bytes) && \
                  std::is_trivially_copyable<H>::value && std::is_trivially_copyable<G>::value, #H " / " #G ": size")
#define HRT_SAME_FIELD(H, G, field) static_assert(offsetof(H, field) == offsetof(G, field), #H " / " #G ": offset of " #field)
#define HRT_FIELD_AT(T, field, byte) static_assert(offsetof(T, field) == (byte), #T ": offset of " #field)

HRT_SAME_RECORD(HostNode, GpuNode, 64);
HRT_SAME_FIELD(HostNode, GpuNode, lmin); HRT_SAME_FIELD(HostNode, GpuNode, left);
HRT_SAME_FIELD(HostNode, GpuNode, lmax); HRT_SAME_FIELD(HostNode, GpuNode, right);
HRT_SAME_FIELD(HostNode, GpuNode, rmin); HRT_SAME_FIELD(HostNode, GpuNode, pad0);
HRT_SAME_FIELD(HostNode, GpuNode, rmax); HRT_SAME_FIELD(HostNode, GpuNode, pad1);

// float[4] rows on the host, float4 rows on the device: the row offsets the traversal adds to a node's byte address (GlobalBvh4::rowoff)
HRT_SAME_RECORD(HostNode4, GpuNode4, 128);
HRT_SAME_FIELD(HostNode4, GpuNode4, minx); HRT_SAME_FIELD(HostNode4, GpuNode4, maxx);
HRT_SAME_FIELD(HostNode4, GpuNode4, miny); HRT_SAME_FIELD(HostNode4, GpuNode4, maxy);
HRT_SAME_FIELD(HostNode4, GpuNode4, minz); HRT_SAME_FIELD(HostNode4, GpuNode4, maxz);
HRT_SAME_FIELD(HostNode4, GpuNode4, child); HRT_SAME_FIELD(HostNode4, GpuNode4, pad);
HRT_FIELD_AT(GpuNode4, minx, 0); HRT_FIELD_AT(GpuNode4, maxx, 16); HRT_FIELD_AT(GpuNode4, miny, 32); HRT_FIELD_AT(GpuNode4, maxy, 48);
HRT_FIELD_AT(GpuNode4, minz, 64); HRT_FIELD_AT(GpuNode4, maxz, 80); HRT_FIELD_AT(GpuNode4, child, 96);

HRT_SAME_RECORD(HostTri, GpuTri, 48);
HRT_SAME_FIELD(HostTri, GpuTri, p0); HRT_SAME_FIELD(HostTri, GpuTri, inst);
HRT_SAME_FIELD(HostTri, GpuTri, p1); HRT_SAME_FIELD(HostTri, GpuTri, prim);
HRT_SAME_FIELD(HostTri, GpuTri, p2); HRT_SAME_FIELD(HostTri, GpuTri, flags);
HRT_FIELD_AT(HostTri, prim, 7 * 4);         // pt_shadow.h candidate_insert and the leaf loops read the primitive as b.w of a triangle record

// No field has a name on both sides: the device reads five float4 rows (unpack_tri_attr states which word is what), the host names the words.
HRT_SAME_RECORD(HostTriAttr, GpuTriAttr, 80);
HRT_FIELD_AT(HostTriAttr, n0, 0); HRT_FIELD_AT(HostTriAttr, n1, 3 * 4); HRT_FIELD_AT(HostTriAttr, n2, 6 * 4);
HRT_FIELD_AT(HostTriAttr, uv0, 9 * 4); HRT_FIELD_AT(HostTriAttr, uv1, 11 * 4); HRT_FIELD_AT(HostTriAttr, uv2, 13 * 4);
HRT_FIELD_AT(HostTriAttr, material, 15 * 4);    // d.w
HRT_FIELD_AT(HostTriAttr, inst, 16 * 4);        // e.x: pt_motion.h reads word [16] of an attribute record
HRT_FIELD_AT(HostTriAttr, prim, 17 * 4);        // e.y: pt_gbuffer.h and pt_motion.h read word [17]
HRT_FIELD_AT(GpuTriAttr, d, 48); HRT_FIELD_AT(GpuTriAttr, e, 64);

HRT_SAME_RECORD(HostTriTangent, GpuTriTangent, 48);
HRT_SAME_FIELD(HostTriTangent, GpuTriTangent, t0); HRT_SAME_FIELD(HostTriTangent, GpuTriTangent, t1); HRT_SAME_FIELD(HostTriTangent, GpuTriTangent, t2);

HRT_SAME_RECORD(HostInstShade, GpuInstShade, 48);
HRT_SAME_FIELD(HostInstShade, GpuInstShade, adj0); HRT_SAME_FIELD(HostInstShade, GpuInstShade, adj1); HRT_SAME_FIELD(HostInstShade, GpuInstShade, adj2);

HRT_SAME_RECORD(HostInstance, GpuInstance, 128);
HRT_SAME_FIELD(HostInstance, GpuInstance, world); HRT_SAME_FIELD(HostInstance, GpuInstance, inv);
HRT_SAME_FIELD(HostInstance, GpuInstance, blasRoot); HRT_SAME_FIELD(HostInstance, GpuInstance, flags);
HRT_SAME_FIELD(HostInstance, GpuInstance, material); HRT_SAME_FIELD(HostInstance, GpuInstance, boxEps);
HRT_SAME_FIELD(HostInstance, GpuInstance, mesh); HRT_SAME_FIELD(HostInstance, GpuInstance, objMaxAbs);
HRT_SAME_FIELD(HostInstance, GpuInstance, invNorm); HRT_SAME_FIELD(HostInstance, GpuInstance, pad);

#undef HRT_SAME_RECORD
#undef HRT_SAME_FIELD
#undef HRT_FIELD_AT

} // namespace hrt
