"""Register / scratch budget of the wavefront kernels, read from the code-object metadata of the built library (no GPU needed).

Why a test: several kernels are compiled for a FORCED number of waves per SIMD (amdgpu_waves_per_eu, pt_wf_extend.h), i.e. into fewer
registers than the compiler would take. While the library was still built with the SLP vectoriser, exactly that forcing gave a wf_shade
that spilled (68 B of scratch per lane) and rendered every sky pixel 5-10 % wrong (reproducible with
`make -C hobbyrenderer_amd/csrc variant NAME=slp EXTRA="-Xarch_device -fslp-vectorize"` + tests/test_parity_gpu.py seed 1). The parity
tests on the GPU are the real guard; this one fails earlier, on the CPU, when a compiler or flag change pushes one of these kernels into
spilling or over its occupancy budget again."""
import re

import pytest

import kernel_metadata


@pytest.fixture(scope="module")
def kernels():
    out = kernel_metadata.kernels("pt_wavefront.hip.o")
    assert len(out) > 100
    return out


def _waves(vgpr):
    alloc = (vgpr + 7) // 8 * 8
    return min(8, 512 // alloc)


def test_forced_budget_kernels_do_not_spill(kernels):
    """wf_shade at 4 waves per SIMD (128 VGPRs): the single-light variants and the streamed one fit without scratch; the 8-light variant keeps
    its light-sample buffer in scratch by design (NeeBuf, ~100 B), nothing more."""
    for name in ("wf_shade<1, true, true>", "wf_shade<1, true, false>", "wf_shade<1, false, false>", "wf_shade<0, false, false>"):
        k = kernels[name]
        assert k["vgpr"] <= 128 and k["scratch"] == 0, (name, k)
    k = kernels["wf_shade<8, false, false>"]
    assert k["vgpr"] <= 128 and k["scratch"] <= 128, k


def test_traversal_kernels_keep_their_occupancy(kernels):
    """Closest-hit traversal: six waves per SIMD (<= 80 VGPRs) over LDS trees and over global trees (fp32 and quantised nodes), five for the
    two-level variants; at most a few spilled registers (the bounce-0 instantiations give up some for the sixth wave)."""
    seen = 0
    for name, k in kernels.items():
        m = re.match(r"wf_extend<(true|false), (\d+), (\d), (true|false), (\d)(?:, (true|false))?(?:, (true|false))?>", name)
        if not m:
            continue
        seen += 1
        lds, anyhit, tl = m.group(1) == "true", m.group(4) == "true", int(m.group(5))
        want = 5 if tl else 6
        assert _waves(k["vgpr"]) >= want, (name, k)
        assert k["scratch"] <= 64, (name, k)
        if lds and not anyhit and m.group(7) == "true":        # all-opaque instantiation of an LDS tree: no candidate state
            assert k["vgpr"] <= 80
    assert seen >= 40
    # the slim / opaque shadow kernels of LDS trees: seven waves
    assert _waves(kernels["wf_shadow<true, 16, 2, true, 3, 0>"]["vgpr"]) >= 7


# scratch bytes of wf_shadow<LDS_BVH, DEPTH, W, false, kShadowResolve, 0> in the build before pt_shadow.h existed: (LDS_BVH, DEPTH, W) -> bytes
RESOLVE_SCRATCH = {
    (False, 8, 2): 20, (False, 16, 2): 20, (False, 16, 4): 44, (False, 16, 5): 16, (False, 32, 2): 28, (False, 32, 4): 44, (False, 32, 5): 28,
    (False, 64, 2): 28, (False, 64, 4): 44, (False, 64, 5): 28,
    (True, 8, 2): 28, (True, 16, 2): 28, (True, 16, 4): 52, (True, 32, 2): 28, (True, 32, 4): 60, (True, 64, 2): 28, (True, 64, 4): 60,
}


def test_shadow_resolve_variants_keep_their_spill_budget(kernels):
    """wf_shadow's resolve variants (MODE 2) are compiled into 128 VGPRs for the fourth wave and spill a few registers; how many depends on
    how shadow_resolve_candidates (pt_shadow.h) is spelled, and with other spellings the glass config lost 0.5 to 2 %. No variant may take
    more scratch than it did before that function moved to pt_shadow.h."""
    seen = set()
    for name, k in kernels.items():
        m = re.match(r"wf_shadow<(true|false), (\d+), (\d), false, 2, 0>", name)
        if m:
            key = (m.group(1) == "true", int(m.group(2)), int(m.group(3)))
            seen.add(key)
            assert k["vgpr"] <= 128 and k["scratch"] <= RESOLVE_SCRATCH[key], (name, k)
    assert seen == set(RESOLVE_SCRATCH)
