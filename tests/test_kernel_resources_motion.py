"""The kernels of hrpt_render_motion_vectors: register and scratch budget, read from the code-object metadata of the
built objects -- the method of tests/test_kernel_resources_shade_lt.py, no GPU needed.

wf_gbuffer_motion is held to what the shade kernels are held to: no scratch and at most 128 VGPRs (four waves per SIMD). pt_motion_kernel,
the validation path, may use no scratch beyond the private traversal stack pt_gbuffer_kernel has."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
BUILD = os.path.join(ROOT, "hobbyrenderer_amd", "csrc", "build")


def _short(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    return name.replace("hrt::(anonymous namespace)::", "").replace("hrt::", "").replace("void ", "").split("(")[0]


def _kernels(obj):
    path = os.path.join(BUILD, obj)
    if not os.path.exists(path) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip(f"{obj} or the LLVM tools are not here (the object is built by __graft_entry__.build())")
    with tempfile.TemporaryDirectory() as t:
        fb, co = os.path.join(t, "fb"), os.path.join(t, "co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fb}", path])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}", f"--output={co}", "--unbundle"])
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    out = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+).*?\.vgpr_count:\s+(\d+)", notes, re.S):
        out[_short(m.group(2))] = {"lds": int(m.group(1)), "scratch": int(m.group(3)), "vgpr": int(m.group(5))}
    return out


@pytest.fixture(scope="module")
def wavefront():
    return _kernels("pt_wavefront.hip.o")


@pytest.fixture(scope="module")
def megakernel():
    return _kernels("pt_megakernel.hip.o")


def test_wf_gbuffer_motion_exists_without_scratch_at_four_waves(wavefront):
    motion = {n: k for n, k in wavefront.items() if n.startswith("wf_gbuffer_motion")}
    assert {"wf_gbuffer_motion<true>", "wf_gbuffer_motion<false>"} <= set(motion), sorted(wavefront)[:8]
    for n, k in motion.items():
        print(n, k)
        assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] == 0, (n, k)
    assert motion["wf_gbuffer_motion<false>"]["vgpr"] < motion["wf_gbuffer_motion<true>"]["vgpr"]      # motion only: none of gbuffer_texels' registers
    assert wavefront["wf_gbuffer"]["scratch"] == 0                                                         # the G-buffer call's own kernel is still there


def test_pt_motion_kernel_has_only_the_traversal_stack(megakernel):
    for tl in ("true", "false"):
        m, g = megakernel[f"pt_motion_kernel<{tl}>"], megakernel[f"pt_gbuffer_kernel<{tl}>"]
        print(tl, m, g)
        assert g["scratch"] > 0 and m["scratch"] <= g["scratch"], (tl, m, g)
