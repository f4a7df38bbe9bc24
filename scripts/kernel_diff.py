#!/usr/bin/env python3
"""kernel_diff.py <object A> <object B>, or kernel_diff.py <A>... -- <B>...: do two builds hold the same gfx950 kernels? Each side is one
or more HIP objects (a directory stands for every *.hip.o in it); their kernels are pooled and compared BY NAME, so a kernel that moved to
another object between the builds is still compared. Compares the symbol list, the code-object metadata (registers, scratch, LDS, kernarg
bytes) and the disassembly with addresses stripped (code objects of one source differ in their __hip_cuid_ symbol and may order functions
differently, so they cannot be compared as files; for the same reason a pc-relative address is compared as the data symbol and offset it
lands in, not as the distance to it, and the padding behind a function's end is left out). Prints the kernel count of every object. Exit status 1 on any difference."""
import glob, os, re, subprocess, sys, tempfile

L = "/opt/rocm/lib/llvm/bin/"


def kernels(obj):
    with tempfile.TemporaryDirectory() as t:
        fb, co = os.path.join(t, "fb"), os.path.join(t, "co")
        subprocess.check_call([L + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, obj])
        subprocess.check_call([L + "clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + co, "--unbundle"])
        notes = subprocess.check_output([L + "llvm-readelf", "--notes", co]).decode()
        dis = subprocess.check_output([L + "llvm-objdump", "-d", "--no-show-raw-insn", co]).decode()
        syms = subprocess.check_output([L + "llvm-readelf", "-sW", co]).decode()
    meta = {}
    for m in re.finditer(r"- \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target)", notes, re.S):
        f = dict(re.findall(r"\.(name|vgpr_count|sgpr_count|agpr_count|private_segment_fixed_size|group_segment_fixed_size|kernarg_segment_size):\s+(\S+)", m.group(0)))
        meta[f.pop("name")] = f
    data = sorted((int(v, 16), int(z), n) for v, z, n in re.findall(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+OBJECT\s+\S+\s+\S+\s+\d+\s+(\S+)$", syms, re.M))

    def named(m):      # the data symbol a pc-relative address (s_getpc_b64; s_add_u32 lo, lo, literal) lands in, instead of the distance to it
        target = int(m.group(2), 16) + 4 + int(m.group(4), 16) - (1 << 32 if int(m.group(4), 16) >> 31 else 0)
        hit = [f"{n}+{target - v}" for v, z, n in data if v <= target < v + max(z, 1)]
        return m.group(1) + m.group(3) + "<" + (hit[0] if hit else "?" + m.group(4)) + ">" + m.group(5)

    code = {}
    for m in re.finditer(r"^[0-9a-f]+ <(\S+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
        body = re.sub(r"(s_getpc_b64 \S+\s*// ([0-9A-F]+):.*\n)(\s*s_add_u32 \S+ \S+ )0x([0-9a-f]+)(\s*//)", named, m.group(2))
        # drop the address comment of every line, name branch targets by their offset inside the function, drop the padding behind the end
        body = re.sub(r"\s*// [0-9A-F]+:.*$", "", re.sub(r"<\S+?(\+0x[0-9a-f]+)?>(?!\s*//)", r"<\1>", body), flags=re.M)
        code[m.group(1)] = re.sub(r"(\n\ts_nop 0|\n\t\t\.\.\.)*\s*\Z", "", body)
    return meta, code


def side(paths):
    """Pooled (metadata by kernel name, disassemblies by function name) of the objects; a name that several objects carry keeps every
    entry, and the sorted lists are compared."""
    objs = []
    for p in paths:
        objs += sorted(glob.glob(os.path.join(p, "*.hip.o"))) if os.path.isdir(p) else [p]
    meta, code, where = {}, {}, {}
    for o in objs:
        m, c = kernels(o)
        print(f"  {o}: {len(m)} kernels")
        for n in m:
            meta.setdefault(n, []).append(sorted(m[n].items())); where[n] = o
        for n, body in c.items():
            if not n.startswith("__hip_cuid_"): code.setdefault(n, []).append(body)
    return {n: sorted(v) for n, v in meta.items()}, {n: sorted(b) for n, b in code.items()}, where


def main(a, b):
    print("A:"); ma, ca, wa = side(a)
    print("B:"); mb, cb, wb = side(b)
    bad = 0
    for what, x, y in (("kernel", ma, mb), ("function", ca, cb)):
        for n in sorted(set(x) ^ set(y)):
            print(f"{what} only in {'A' if n in x else 'B'}: {n}"); bad += 1
    for n in sorted(set(ma) & set(mb)):
        if ma[n] != mb[n]: print(f"metadata differs: {n}\n  {ma[n]}\n  {mb[n]}"); bad += 1
    for n in sorted(set(ca) & set(cb)):
        if ca[n] != cb[n]: print(f"disassembly differs: {n}"); bad += 1
    moved = sorted(n for n in set(ma) & set(mb) if os.path.basename(wa[n]) != os.path.basename(wb[n]))
    if moved: print(f"{len(moved)} kernels changed object (compared all the same)")
    print(f"{len(ma)} / {len(mb)} kernels, {len(ca)} / {len(cb)} functions compared: {'identical' if not bad else str(bad) + ' differences'}")
    return 1 if bad else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--" in args: cut = args.index("--"); a, b = args[:cut], args[cut + 1:]
    elif len(args) == 2: a, b = args[:1], args[1:]
    else: sys.exit(__doc__)
    if not a or not b: sys.exit(__doc__)
    sys.exit(main(a, b))
