// pt_device.h -- gfx950 device code shared by the path-tracer kernels: vector algebra, BVH
// traversal with a watertight triangle test, bindless/LUT sampling, Bruneton atmosphere
// lookups, PBR BRDF evaluation and sampling.
//
// Follows /root/reference/src/shaders/{PathTracer.hlsl, RaytracingCommon.hlsli,
// CommonLighting.hlsli, Atmosphere.hlsli, MeshCommon.hlsli, Common.hlsli, RNG.hlsli}; each
// function names the lines it implements. Scalar HLSL intrinsics come from the numeric
// contract include/hobbyrt/detmath.h; expression order is fixed (left to right, no FMA
// contraction: build with -ffp-contract=off) so that radiance is a pure function of
// (Scene, constants, pixel, accumulation index).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hobbyrt_pt.h"
#include "../../include/hobbyrt/detmath.h"
#include "../../include/hobbyrt/srgb_table.h"

// The code, one subject per header. Every header includes what it needs; this order is the order of declaration the kernels were built with,
// and keeping it keeps their code objects as they are. pt_vec.h, pt_lighting.h and pt_direct.h are __host__ __device__ and need no HIP
// runtime: the deferred stage's host executors and its sanitizer program build them with a plain C++ compiler.
#include "pt_phase.h"
#include "pt_vec.h"
#include "pt_scene_records.h"
#include "pt_traverse.h"
#include "pt_shade_tables.h"
#include "pt_texture.h"
#include "pt_atmosphere.h"
#include "pt_lighting.h"
#include "pt_direct.h"
#include "pt_surface.h"
