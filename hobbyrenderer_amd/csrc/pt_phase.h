// pt_phase.h -- HRT_DEV and the phase profile of the diagnostic build: HRT_PHASE and its ids.
#pragma once

#include <hip/hip_runtime.h>

#define HRT_DEV __device__ __forceinline__

// Phase profile (make PHASES=1 builds libhobbyrt_pt_phases.so): HRT_PHASE(k) counts, per wave, how often a code region runs and with how
// many lanes -- the lane utilisation of every stage of a kernel, which the PMC counters only give per kernel. One aggregated atomic per
// wave and execution: slow, a diagnostic build only (scripts/phase_profile.py prints the table).
#if defined(HRPT_PHASE_PROFILE) && defined(HRPT_PHASE_TU)       // only the wavefront translation unit is instrumented (no RDC)
extern __device__ unsigned long long g_phaseCounters[128];
#define HRT_PHASE(k)                                                                                                      \
    do {                                                                                                                  \
        const unsigned long long m_ = __ballot(true);                                                                     \
        if ((threadIdx.x & 63u) == (unsigned)(__ffsll((long long)m_) - 1)) {                                              \
            atomicAdd(&g_phaseCounters[2 * (k)], 1ull); atomicAdd(&g_phaseCounters[2 * (k) + 1], (unsigned long long)__popcll(m_)); \
        }                                                                                                                 \
    } while (0)
#else
#define HRT_PHASE(k) do { } while (0)
#endif
// phase ids
enum {
    PH_EXT_ITER = 0, PH_EXT_REFILL, PH_EXT_NODE, PH_EXT_LEAF, PH_EXT_TRI, PH_EXT_FINISH, PH_EXT_CANDIDATE,
    PH_ANY_ITER = 8, PH_ANY_REFILL, PH_ANY_NODE, PH_ANY_LEAF, PH_ANY_TRI, PH_ANY_FINISH,
    PH_SHADE_ITER = 16, PH_SHADE_HIT, PH_SHADE_ATTR, PH_SHADE_TEX, PH_SHADE_TRANS, PH_SHADE_NEE, PH_SHADE_LOBE_BEGIN, PH_SHADE_DIFFUSE, PH_SHADE_SPEC,
    PH_SHADE_SKY, PH_SHADE_WRITE, PH_SHADE_SORT,
    PH_SHADOW_ENTRY = 32, PH_SHADOW_SAMPLE, PH_SHADOW_QUERY, PH_SHADOW_CONTRIB, PH_SHADOW_RAYS_ITEM,
    PH_COUNT = 40
};
