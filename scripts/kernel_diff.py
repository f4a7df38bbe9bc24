#!/usr/bin/env python3
"""kernel_diff.py <object A> <object B>: do two builds of a HIP object hold the same gfx950 kernels? Compares, by kernel name, the symbol list,
the code-object metadata (registers, scratch, LDS, kernarg bytes) and the disassembly with addresses stripped (code objects of one source
differ in their __hip_cuid_ symbol and may order functions differently, so they cannot be compared as files). Exit status 1 on any difference."""
import os, re, subprocess, sys, tempfile

L = "/opt/rocm/lib/llvm/bin/"


def kernels(obj):
    with tempfile.TemporaryDirectory() as t:
        fb, co = os.path.join(t, "fb"), os.path.join(t, "co")
        subprocess.check_call([L + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, obj])
        subprocess.check_call([L + "clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + co, "--unbundle"])
        notes = subprocess.check_output([L + "llvm-readelf", "--notes", co]).decode()
        dis = subprocess.check_output([L + "llvm-objdump", "-d", "--no-show-raw-insn", co]).decode()
    meta = {}
    for m in re.finditer(r"- \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target)", notes, re.S):
        f = dict(re.findall(r"\.(name|vgpr_count|sgpr_count|agpr_count|private_segment_fixed_size|group_segment_fixed_size|kernarg_segment_size):\s+(\S+)", m.group(0)))
        meta[f.pop("name")] = f
    code = {}
    for m in re.finditer(r"^[0-9a-f]+ <(\S+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
        # drop the address comment of every line and name branch targets by their offset inside the function
        code[m.group(1)] = re.sub(r"\s*// [0-9A-F]+:.*$", "", re.sub(r"<\S+?(\+0x[0-9a-f]+)?>", r"<\1>", m.group(2)), flags=re.M)
    return meta, code


def main(a, b):
    (ma, ca), (mb, cb) = kernels(a), kernels(b)
    bad = 0
    for what, x, y in (("kernel", ma, mb), ("function", ca, cb)):
        for n in sorted(set(x) ^ set(y)):
            if not n.startswith("__hip_cuid_"):
                print(f"{what} only in {a if n in x else b}: {n}"); bad += 1
    for n in sorted(set(ma) & set(mb)):
        if ma[n] != mb[n]: print(f"metadata differs: {n}\n  {ma[n]}\n  {mb[n]}"); bad += 1
    for n in sorted(set(ca) & set(cb)):
        if ca[n] != cb[n]: print(f"disassembly differs: {n}"); bad += 1
    print(f"{len(ma)} / {len(mb)} kernels, {len(ca)} / {len(cb)} functions compared: {'identical' if not bad else str(bad) + ' differences'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
