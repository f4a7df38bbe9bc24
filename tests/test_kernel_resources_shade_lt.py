"""wf_shade_lt (wf_shade over triangle / instance / material tables in LDS, pt_wf_shade.h): register, scratch and LDS budget of every
instantiation, read from the code-object metadata of the built library -- the method of tests/test_kernel_resources.py, no GPU needed.

The kernel is compiled for a forced four waves per SIMD like wf_shade, whose history of miscompiles under register pressure is told there:
no scratch and at most 128 VGPRs. Four waves per SIMD are four 256-thread blocks per CU, so the static LDS plus the largest dynamic LDS the
launch plan ever asks for (pt_wavefront_plan.h kShadeLdsPerBlock) must fit a quarter of the CU's 160 KiB; and the table reads must be
ds_read, neither flat_load nor more global_load than the global-table kernel minus its gathers."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
CSRC = os.path.join(ROOT, "hobbyrenderer_amd", "csrc")
OBJ = os.path.join(CSRC, "build", "pt_wavefront.hip.o")
CU_LDS, BLOCKS_PER_CU = 160 * 1024, 4

LIMITS = r"""
#include <stdio.h>
#include "pt_wavefront_plan.h"
int main() { printf("%zu %zu %zu\n", hrt::kShadeLdsPerBlock, hrt::kShadeRingBytes, hrt::kShadeLdsMargin); return 0; }
"""


def _short(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    return name.replace("hrt::(anonymous namespace)::", "").replace("void ", "").split("(")[0]


@pytest.fixture(scope="module")
def code_object():
    if not os.path.exists(OBJ) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("pt_wavefront.hip.o or the LLVM tools are not here (the object is built by __graft_entry__.build())")
    with tempfile.TemporaryDirectory() as t:
        fb, co = os.path.join(t, "fb"), os.path.join(t, "co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fb}", OBJ])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}", f"--output={co}", "--unbundle"])
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
        asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
    kernels = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+).*?\.vgpr_count:\s+(\d+)", notes, re.S):
        if "wf_shade" in m.group(2):
            kernels[_short(m.group(2))] = {"lds": int(m.group(1)), "scratch": int(m.group(3)), "vgpr": int(m.group(5))}
    bodies = {}
    for m in re.finditer(r"\n[0-9a-f]+ <(\S*wf_shade\S*)>:\n(.*?)(?=\n[0-9a-f]+ <|\Z)", asm, re.S):
        bodies[_short(m.group(1))] = m.group(2)
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
