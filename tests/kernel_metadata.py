"""What the kernel-resource tests read of hobbyrenderer_amd/csrc/build/<object> (no GPU needed): the gfx950 code object's notes as
{short kernel name: {lds, scratch, sgpr, vgpr}} and, on request, its disassembly per function. One reader and one name-shortening rule;
every object is unbundled, and every answer worked out, once per session (the answers are shared: read them, do not change them)."""
import atexit
import functools
import os
import re
import subprocess
import tempfile

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hobbyrenderer_amd", "csrc")


def short(mangled):
    """Mangled names -> pt_megakernel<true>, wf_extend<true, 16, 2, ...>: demangled, without namespace, return type and parameter list."""
    names = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    return [n.strip().replace("hrt::(anonymous namespace)::", "").replace("hrt::", "").replace("void ", "").split("(")[0] for n in names[:len(mangled)]]


@functools.lru_cache(maxsize=None)
def _code_object(obj):
    path = os.path.join(CSRC, "build", obj)
    if not os.path.exists(path) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip(f"{obj} or the LLVM tools are not here (the object is built by __graft_entry__.build())")
    t = tempfile.TemporaryDirectory()
    atexit.register(t.cleanup)
    fb, co = os.path.join(t.name, "fb"), os.path.join(t.name, "co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fb}", path])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}", f"--output={co}", "--unbundle"])
    return co


@functools.lru_cache(maxsize=None)
def kernels(obj):
    """{short kernel name: {lds, scratch, sgpr, vgpr}} of the object; skips the calling test when it or the LLVM tools are not there."""
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", _code_object(obj)], capture_output=True, text=True, check=True).stdout
    found = re.findall(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+).*?\.vgpr_count:\s+(\d+)", notes, re.S)
    return {n: {"lds": int(f[0]), "scratch": int(f[2]), "sgpr": int(f[3]), "vgpr": int(f[4])} for n, f in zip(short([f[1] for f in found]), found)}


@functools.lru_cache(maxsize=None)
def disassembly(obj):
    """{short function name: its instructions as llvm-objdump prints them} of the same object."""
    asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", _code_object(obj)], capture_output=True, text=True, check=True).stdout
    found = re.findall(r"\n[0-9a-f]+ <(\S+)>:\n(.*?)(?=\n[0-9a-f]+ <|\Z)", asm, re.S)
    return dict(zip(short([f[0] for f in found]), (f[1] for f in found)))
