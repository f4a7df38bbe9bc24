"""The Python side of the C boundary against the headers themselves: every entry point's ctypes signature against its prototype, every
mirrored record against the header's sizeof / offsetof, every mirrored constant against the header's value. One C program, generated
from the mirrors and compiled against include/, prints the layout and constant facts; the prototypes are read from the header text.
Needs the built libraries and gcc; no GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hobbyrenderer_amd import native, scene_io, structs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# records of include/hobbyrt_scene.h and where their mirrors live
SCENE_RECORDS = {"HrscCookedMesh": scene_io._CookedMesh, "HrscSceneView": scene_io._SceneView, "HrscPrimitive": S.Primitive, "HrscMeshlet": S.Meshlet}
# integer constants of the headers that Python has no use for, so no mirror
UNMIRRORED = {"HRPT_OK", "HRPT_ERR_INVALID_ARGUMENT", "HRPT_ERR_NO_DEVICE", "HRPT_ERR_HIP", "HRPT_ERR_NO_SCENE", "HRPT_ERR_OUT_OF_MEMORY", "HRPT_ERR_UNSUPPORTED",
              "HRPT_TEXTURE_MAX_MIPS", "HRPT_TRANSMITTANCE_TEXTURE_WIDTH", "HRPT_TRANSMITTANCE_TEXTURE_HEIGHT", "HRPT_SCATTERING_TEXTURE_WIDTH",
              "HRPT_SCATTERING_TEXTURE_HEIGHT", "HRPT_SCATTERING_TEXTURE_DEPTH", "HRPT_IRRADIANCE_TEXTURE_WIDTH", "HRPT_IRRADIANCE_TEXTURE_HEIGHT",
              "HRSC_OK", "HRSC_ERR_INVALID_ARG", "HRSC_COOKED_MESH_MAGIC", "HRSC_COOKED_MESH_VERSION"}
SCALARS = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "int": C.c_int, "int32_t": C.c_int32, "float": C.c_float}
RETURNS = {"int": C.c_int, "void": None, "float": C.c_float, "const char*": C.c_char_p}


def _header(name):
    """The header's text without comments."""
    with open(os.path.join(ROOT, "include", name)) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)


PT_H, SCENE_H = _header("hobbyrt_pt.h"), _header("hobbyrt_scene.h")


def _prototypes(text, prefix):
    """{name: (return type, [(base type, pointer depth) per parameter])} of every `prefix`_* function the header declares."""
    out = {}
    for ret, name, params in re.findall(r"(?m)^\s*(const char\*|int|void|float)\s+(%s_\w+)\s*\(([^;{)]*)\)\s*;" % prefix, text):
        decls = [] if params.strip() in ("", "void") else [p.strip() for p in params.split(",")]
        parsed = []
        for p in decls:
            words = re.sub(r"\[[^\]]*\]|\*|\bconst\b", " ", p).split()
            parsed.append((" ".join(words[:-1] if len(words) > 1 else words), p.count("*") + p.count("[")))
        out[name] = (ret, parsed)
    return out


def _record_name(t):
    """The header's name of a mirror class: structs.X is HrptX, scene_io's are listed above."""
    if getattr(S, t.__name__, None) is t:
        return "Hrpt" + t.__name__
    return next((k for k, v in SCENE_RECORDS.items() if v is t), None)


def _argument_error(ctype, base, depth):
    """None when ctypes type `ctype` may stand for a C parameter of type `base` with `depth` stars, else what is wrong."""
    if depth == 0:
        return None if base in SCALARS and ctype is SCALARS[base] else f"scalar {base} declared as {ctype}"
    if ctype is C.c_void_p:
        return None
    if ctype is C.c_char_p:
        return None if depth == 1 and base in ("char", "uint8_t") else f"c_char_p for {base}{'*' * depth}"
    if not (isinstance(ctype, type) and issubclass(ctype, C._Pointer)):
        return f"pointer {base}{'*' * depth} declared as {ctype}"
    target = ctype._type_
    if target is C.c_void_p:
        return None if depth == 2 else f"POINTER(c_void_p) for {base}{'*' * depth}"
    if isinstance(target, type) and issubclass(target, C._Pointer):
        return _argument_error(target, base, depth - 1)
    if depth != 1:
        return f"POINTER({target.__name__}) for {base}{'*' * depth}"
    if issubclass(target, C.Structure):
        return None if _record_name(target) == base else f"POINTER({target.__name__}) for {base}*"
    return None if base in SCALARS and target is SCALARS[base] else f"POINTER({target.__name__}) for {base}*"


@pytest.mark.parametrize("header,prefix,binding", [(PT_H, "hrpt", native), (SCENE_H, "hrsc", scene_io)], ids=["hobbyrt_pt.h", "hobbyrt_scene.h"])
def test_signatures_agree_with_the_prototypes(header, prefix, binding):
    protos = _prototypes(header, prefix)
    assert sorted(protos) == sorted(binding.EXPORTS), "every prototype has one declaration, and every declaration a prototype"
    assert len(protos) == len(re.findall(r"\b%s_\w+\s*\(" % prefix, header)), "a prototype the parser did not read"
    wrong = []
    for name, (ret, params) in sorted(protos.items()):
        fn = getattr(binding.lib, name)
        if fn.restype is not RETURNS[ret]:
            wrong.append(f"{name}: returns {ret}, restype {fn.restype}")
        if fn.argtypes is None or len(fn.argtypes) != len(params):
            wrong.append(f"{name}: {len(params)} parameters, argtypes {fn.argtypes}")
            continue
        for k, (ctype, (base, depth)) in enumerate(zip(fn.argtypes, params)):
            err = _argument_error(ctype, base, depth)
            if err:
                wrong.append(f"{name}, argument {k}: {err}")
    assert not wrong, "\n".join(wrong)


def _mirrors():
    """{header typedef: mirror} for every ctypes.Structure / structured dtype of structs whose HrptX the header defines, and the scene records."""
    out = {}
    for name, v in vars(S).items():
        is_record = (isinstance(v, type) and issubclass(v, C.Structure)) or (isinstance(v, np.dtype) and v.fields)
        if is_record and re.search(r"\}\s*Hrpt%s\s*;" % name, PT_H):
            out["Hrpt" + name] = v
    out.update(SCENE_RECORDS)
    return out


def _fields(mirror):
    """[(field, offset, size)] of a mirror."""
    if isinstance(mirror, np.dtype):
        return [(f, mirror.fields[f][1], mirror.fields[f][0].itemsize) for f in mirror.names]
    return [(f, getattr(mirror, f).offset, getattr(mirror, f).size) for f, *_ in mirror._fields_]


def _constants():
    return sorted(set(re.findall(r"#define\s+(HR(?:PT|SC)_\w+)\s+\S", PT_H + SCENE_H)) | set(re.findall(r"\b(HR(?:PT|SC)_\w+)\s*=", PT_H + SCENE_H)))


@pytest.fixture(scope="module")
def header_facts(tmp_path_factory):
    """What the compiler says: {"sizeof HrptX": n, "HrptX.field": (offset, size), "HRPT_NAME": value}."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hobbyrt_scene.h"', "int main(void) {"]
    for ctype, mirror in _mirrors().items():
        lines.append(f'printf("sizeof {ctype} %zu\\n", sizeof({ctype}));')
        lines += [f'printf("{ctype}.{f} %zu %zu\\n", offsetof({ctype}, {f}), sizeof((({ctype}*)0)->{f}));' for f, _, _ in _fields(mirror)]
    lines += [f'printf("{name} %lld\\n", (long long)({name}));' for name in _constants()]
    d = tmp_path_factory.mktemp("contract")
    (d / "facts.c").write_text("\n".join(lines + ["return 0; }", ""]))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(d / "facts"), str(d / "facts.c")])
    facts = {}
    for line in subprocess.check_output([str(d / "facts")], text=True).splitlines():
        words = line.split()
        if words[0] == "sizeof":
            facts[f"sizeof {words[1]}"] = int(words[2])
        else:
            facts[words[0]] = (int(words[1]), int(words[2])) if "." in words[0] else int(words[1])
    return facts


def test_every_header_record_has_a_mirror():
    records = set(re.findall(r"typedef\s+struct\s+(Hr(?:pt|sc)\w+)\s*\{", PT_H + SCENE_H))
    assert len(records) >= 49 and records == set(_mirrors())


def test_layouts_agree_with_the_header(header_facts):
    wrong, checked = [], 0
    for ctype, mirror in _mirrors().items():
        size = mirror.itemsize if isinstance(mirror, np.dtype) else C.sizeof(mirror)
        if header_facts[f"sizeof {ctype}"] != size:
            wrong.append(f"sizeof {ctype}: header {header_facts[f'sizeof {ctype}']}, mirror {size}")
        for f, offset, fsize in _fields(mirror):
            checked += 1
            if header_facts[f"{ctype}.{f}"] != (offset, fsize):
                wrong.append(f"{ctype}.{f}: header (offset, size) {header_facts[f'{ctype}.{f}']}, mirror {(offset, fsize)}")
    assert not wrong, "\n".join(wrong)
    assert checked >= 378       # the fields of the 45 records of hobbyrt_pt.h the mirrors had when this test was written


def test_constants_agree_with_the_header(header_facts):
    wrong, unmirrored = [], set()
    for name in _constants():
        holder = scene_io if name.startswith("HRSC_") else S
        mirror = getattr(holder, name, getattr(holder, name[5:], None))
        if mirror is None:
            unmirrored.add(name)
        elif mirror != header_facts[name]:
            wrong.append(f"{name}: header {header_facts[name]}, mirror {mirror}")
    assert not wrong, "\n".join(wrong)
    assert unmirrored == UNMIRRORED


@pytest.fixture(scope="module")
def echo():
    """A foreign function `void* echo(void* p) { return p; }`: the argument goes through c_void_p's conversion as in every wrapper."""
    return C.CFUNCTYPE(C.c_void_p, C.c_void_p)(lambda p: p)


@pytest.mark.parametrize("given", [0x7F12_3456_7000, np.uint64(0x7F12_3456_7000), np.int64(0x7F12_3456_7000)], ids=["int", "np.uint64", "np.int64"])
def test_address_passes_a_48_bit_pointer_unchanged(echo, given):
    from hobbyrenderer_amd.native._lib import address
    assert type(address(given)) is int and echo(address(given)) == 0x7F12_3456_7000


@pytest.mark.parametrize("null", [0, None, np.uint64(0)], ids=["0", "None", "np.uint64(0)"])
def test_address_of_zero_and_none_is_null(echo, null):
    from hobbyrenderer_amd.native._lib import address
    assert address(null) is None and echo(address(null)) is None


def test_records_refuses_another_dtype_by_name():
    from hobbyrenderer_amd.native._lib import records
    light = np.zeros(2, S.GPULight)
    assert records(light, "GPULight") is light and records(light[::2], "GPULight").flags.c_contiguous
    assert records(np.zeros((), S.PathTracerConstants), "PathTracerConstants").nbytes == 768
    with pytest.raises(ValueError, match="PathTracerConstants"):
        records(np.zeros(768, np.uint8), "PathTracerConstants")
    with pytest.raises(ValueError, match="PerInstanceData"):
        records(np.zeros(3, S.GPULight), "PerInstanceData")
