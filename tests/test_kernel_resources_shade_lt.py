"""wf_shade_lt (wf_shade over triangle / instance / material tables in LDS, pt_wf_shade.h): register, scratch and LDS budget of every
instantiation, read from the code-object metadata of the built library -- tests/kernel_metadata.py reads it, no GPU needed.

The kernel is compiled for a forced four waves per SIMD like wf_shade, whose history of miscompiles under register pressure is told in
tests/test_kernel_resources.py:
no scratch and at most 128 VGPRs. Four waves per SIMD are four 256-thread blocks per CU, so the static LDS plus the largest dynamic LDS the
launch plan ever asks for (pt_wavefront_plan.h kShadeLdsPerBlock) must fit a quarter of the CU's 160 KiB; and the table reads must be
ds_read, neither flat_load nor more global_load than the global-table kernel minus its gathers."""
import re
import subprocess

import pytest

import kernel_metadata
from kernel_metadata import CSRC

CU_LDS, BLOCKS_PER_CU = 160 * 1024, 4

LIMITS = r"""
#include <stdio.h>
#include "pt_wavefront_plan.h"
int main() { printf("%zu %zu %zu\n", hrt::kShadeLdsPerBlock, hrt::kShadeRingBytes, hrt::kShadeLdsMargin); return 0; }
"""


@pytest.fixture(scope="module")
def code_object():
    kernels = {n: k for n, k in kernel_metadata.kernels("pt_wavefront.hip.o").items() if "wf_shade" in n}
    bodies = {n: b for n, b in kernel_metadata.disassembly("pt_wavefront.hip.o").items() if "wf_shade" in n}
    return kernels, bodies


@pytest.fixture(scope="module")
def limits(tmp_path_factory):
    d = tmp_path_factory.mktemp("shade_lt_limits")
    (d / "limits.cpp").write_text(LIMITS)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(d / "limits"), str(d / "limits.cpp")])
    per_block, ring, margin = (int(x) for x in subprocess.check_output([str(d / "limits")]).split())
    return {"per_block": per_block, "ring": ring, "margin": margin}


def _lt(kernels):
    return {n: k for n, k in kernels.items() if n.startswith("wf_shade_lt<")}


def test_instantiations_exist(code_object):
    kernels, _ = code_object
    assert {"wf_shade_lt<1, true, true>", "wf_shade_lt<1, true, false>"} <= set(_lt(kernels))
    for n in _lt(kernels):          # every one has its global-table partner of the same template arguments
        assert n.replace("wf_shade_lt<", "wf_shade<") in kernels, n


def test_no_scratch_and_four_waves(code_object):
    kernels, _ = code_object
    for n, k in _lt(kernels).items():
        assert k["scratch"] == 0 and k["vgpr"] <= 128, (n, k)


def test_four_blocks_per_cu_fit_lds(code_object, limits):
    kernels, _ = code_object
    assert limits["per_block"] >= limits["ring"]
    for n, k in _lt(kernels).items():
        assert k["lds"] <= limits["margin"], (n, k)           # static LDS stays inside the margin the plan keeps back
        assert BLOCKS_PER_CU * (k["lds"] + limits["per_block"]) <= CU_LDS, (n, k)


def test_table_reads_are_ds_reads(code_object):
    """No flat_load (a generic pointer into LDS), the 13 per-lane table gathers of the global-table kernel (2 x dwordx4 + 3 x dword of GpuTriAttr,
    3 x dwordx3 of GpuInstShade, 5 loads of HrptMaterialConstants fields) gone from the shading loop, and ds_reads in their place."""
    _, bodies = code_object
    for n in ("wf_shade_lt<1, true, true>", "wf_shade_lt<1, true, false>"):
        lt, gl = bodies[n], bodies[n.replace("wf_shade_lt<", "wf_shade<")]
        assert "flat_load" not in lt and "flat_load" not in gl, n
        # after the block-start copy (it ends at the first s_barrier) the LDS kernel holds that many load instructions fewer than the global
        # one (12 or 13 with this compiler: it merges the field loads differently per instantiation; ten would still mean "the tables are in LDS")
        loop = lt[lt.index("s_barrier"):]
        assert len(re.findall(r"global_load", gl)) - len(re.findall(r"global_load", loop)) >= 10, n
        assert len(re.findall(r"ds_read", loop)) >= len(re.findall(r"ds_read", gl)) + 9, n
