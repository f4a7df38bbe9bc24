// pt_motion_records.h -- the records of the motion pass (pt_motion.h) that the host fills: plain structs, no device functions, so that the
// C-API units can include them without the device code.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hrt {

// Per-instance record of the motion tables (pt_capi.cpp builds them at the first motion call): m_PrevWorld rows 0..3, xyz each (the layout of
// GpuInstance::world), and where the mesh's LOD-0 indices start.
struct MotionInst { float prevWorld[12]; uint32_t firstIndex; uint32_t pad[3]; };
static_assert(sizeof(MotionInst) == 64, "four 16-byte rows");

// What a motion kernel gets next to the scene: the tables, last frame's view (the three members of HrptPlanarViewConstants that
// ComputeMotionVectors reads) and the plane.
struct MotionArgs {
    const MotionInst* inst;         // per instance
    const float* positions;         // object space, 3 floats per vertex (HrptVertexQuantized::m_Pos)
    const float* prevPositions;     // the same one frame ago (hrpt_update_vertices); == positions where nothing deformed
    const uint32_t* indices;        // the scene's index buffer
    float4* plane;                  // W x H
    float prevWorldToClip[16];      // prevView->m_MatWorldToClip
    float prevScale[2], prevBias[2];   // prevView->m_ClipToWindowScale / m_ClipToWindowBias
};

} // namespace hrt
