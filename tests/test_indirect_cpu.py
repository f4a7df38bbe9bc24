"""Traced indirect lighting without a GPU: the host executors hrpt_indirect_rays_host / hrpt_indirect_resolve_host /
hrpt_indirect_compose_host against the NumPy statement of tests/indirect_reference.py, bit for bit, with each lobe flag alone and both;
thread-count invariance; the statement against its float64 formulation; unit directions; the argument errors; and the sanitizer build of the
host side (`make indirect_asan`, a stand-alone program)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from hobbyrenderer_amd import native, structs as S
import indirect_cases as IC
import indirect_reference as R
from test_temporal_cpu import u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hobbyrenderer_amd", "csrc")
SYMBOLS = ("hrpt_indirect_lighting", "hrpt_indirect_compose", "hrpt_read_indirect", "hrpt_get_indirect_device", "hrpt_indirect_lighting_device",
           "hrpt_indirect_compose_device", "hrpt_indirect_rays_device", "hrpt_indirect_resolve_device", "hrpt_indirect_rays_host", "hrpt_indirect_resolve_host", "hrpt_indirect_compose_host")
SIZES = pytest.mark.parametrize("size", IC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
LOBES = pytest.mark.parametrize("flags", IC.LOBES, ids=["diffuse", "specular", "both"])
SEED = 77
# Largest deviation of the float32 statement's dirD, dirS and wS from the float64 formulation over the cases of this file, relative to the
# largest value in play (1 for the unit directions, the largest weight component for wS); measured here, recorded in DESIGN.md section 29.
# The test holds the statement to four times it.
MEASURED_STATEMENT = 1.141e-5
# Share of hit pixels whose cull decision (dot(N, dir) > 0, maxcomp(wS) > 0) sits on a binary32 rounding and flips in binary64: left out of
# the comparison, capped here.
CULL_SHARE_CAP = 0.02


def same_bytes(got, want, what):
    a, b = u32(got), u32(want)
    if not np.array_equal(a, b):
        i = tuple(np.argwhere(a != b)[0])
        raise AssertionError(f"{what}: {int((a != b).sum())} of {a.size} words differ, first at {i}: {got[i]} != {want[i]}")


def test_symbols_are_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "hobbyrt_pt.h")).read()
    for name in SYMBOLS:
        assert name in native.EXPORTS and hasattr(native.lib, name) and f" {name}(" in header, name
    assert "#define HRPT_ABI_VERSION 3" in header and S.ABI_VERSION == 3
    assert (S.INDIRECT_DIFFUSE, S.INDIRECT_SPECULAR, S.INDIRECT_THREAD_PER_RAY, S.RADIANCE_SECONDARY) == (1, 2, 0x200, 0x1000)
    P, I = S.IndirectParams, S.IndirectImages      # that the C header says the same: test_binding_contract.py
    assert C.sizeof(P) == 16 and (P.frameSeed.offset, P.intensity.offset, P.reserved.offset) == (4, 8, 12)
    assert C.sizeof(I) == 56 and (I.depth.offset, I.diffuse.offset, I.specular.offset, I.colorInOut.offset) == (24, 32, 40, 48)


# ---------------------------------------------------------------- 1. rays
@SIZES
@LOBES
def test_rays_host_equals_reference(size, flags):
    c = IC.case(*size)
    got = native.indirect_rays_host(*c["planes"], c["cb"], S.IndirectParams(flags, SEED))
    ref = R.rays(*c["planes"], c["cb"], flags, SEED)
    assert got.shape == ((2 if flags == 3 else 1), size[1], size[0])
    assert got.tobytes() == ref.tobytes()
    assert (got["pad"] == 0).all()
    untraced = np.isnan(got["origin"]).all(-1)
    assert (u32(got["origin"][untraced]) == 0x7FC00000).all() and (got["direction"][untraced] == 0).all()
    assert (got["tmin"][untraced] == 0).all() and (got["tmax"][untraced] == 0).all() and (got["rng"][untraced] == 0).all()
    assert (got["tmin"][~untraced] == np.float32(1e-4)).all() and (got["tmax"][~untraced] == np.float32(1e10)).all()
    assert untraced[:, c["miss"]].all()
    # another seed is other draws
    if size != (1, 1):
        assert native.indirect_rays_host(*c["planes"], c["cb"], S.IndirectParams(flags, SEED + 1)).tobytes() != got.tobytes()


def test_the_cases_hold_what_they_are_there_for():
    c = IC.case(61, 37)
    A, N4, G, D = c["planes"]
    L = R.lobes(*c["planes"], c["cb"], SEED)
    sp = c["special"]
    assert set(sp) == set(IC.SPECIAL) and c["miss"].any() and not c["miss"].all()
    assert abs(c["miss"].mean() - 0.2) < 0.05
    metal = G[..., 3]
    assert (metal == 0).mean() > 0.25 and (metal == 1).mean() > 0.25 and ((metal > 0) & (metal < 1)).any()
    assert N4[..., 3].min() >= np.float32(0.04) and N4[..., 3].max() <= 1 and N4[..., 3].max() > 0.95 and N4[..., 3].min() < 0.1
    _, d, _ = R.primary_rays(c["cb"], 61, 37)
    facing = R._dot(N4[..., :3], -d)
    assert (facing[~c["miss"]] > 0).mean() > 0.3 and (facing[~c["miss"]] < 0).mean() > 0.3          # normals over the whole sphere
    x, y = sp["facing_away"]
    assert np.array_equal(N4[y, x, :3], d[y, x]) and not L["traced_s"][y, x]
    x, y = sp["grazing"]
    assert facing[y, x] == 0 and not L["traced_s"][y, x] and L["traced_d"][y, x] and abs(np.linalg.norm(N4[y, x, :3].astype(np.float64)) - 1) < 1e-6
    x, y = sp["black_metal"]
    assert (A[y, x, :3] == 0).all() and facing[y, x] > 0.99 and L["nds"][y, x] > 0 and L["wmax"][y, x] == 0 and not L["traced_s"][y, x] and not L["traced_d"][y, x]
    for k in ("plus_z", "minus_z"):
        x, y = sp[k]
        assert abs(N4[y, x, 2]) == 1 and L["traced_d"][y, x]
    assert L["traced_s"][sp["minus_z"][1], sp["minus_z"][0]]
    # metallic == 1 never traces a diffuse ray; both lobes trace somewhere and are culled somewhere else
    hit = ~c["miss"]
    assert not L["traced_d"][hit & (metal == 1)].any() and L["traced_d"][hit & (metal == 0)].all()
    assert 0 < L["traced_s"][hit].sum() < hit.sum()


# ---------------------------------------------------------------- 2. resolve and compose
@SIZES
@LOBES
def test_resolve_host_equals_reference(size, flags):
    c = IC.case(*size)
    rad = IC.radiance_for(c, flags)
    dif, spec = native.indirect_resolve_host(*c["planes"], c["cb"], rad, S.IndirectParams(flags, SEED), 3)
    rdif, rspec = R.resolve(*c["planes"], c["cb"], rad, flags, SEED)
    same_bytes(dif, rdif, f"diffuse {size} {flags}")
    same_bytes(spec, rspec, f"specular {size} {flags}")
    assert np.isfinite(dif).all() and np.isfinite(spec).all()
    assert (dif[c["miss"]] == 0).all() and (spec[c["miss"]] == 0).all()
    if not flags & S.INDIRECT_DIFFUSE:
        assert (dif == 0).all()
    if not flags & S.INDIRECT_SPECULAR:
        assert (spec == 0).all()
    if size != (1, 1):
        on = (rad[0, ..., 3] == 1) & ~c["miss"]
        plane = dif if flags & S.INDIRECT_DIFFUSE else spec
        assert on.any() and (plane[on][:, 3] == 1).all() and (plane[~on] == 0).all()
    if flags & S.INDIRECT_DIFFUSE:                     # demodulated: the radiance itself, no albedo and no weight
        on = dif[..., 3] == 1
        same_bytes(dif[on][:, :3], rad[0][on][:, :3], "the diffuse plane is the radiance")


@SIZES
def test_compose_host_equals_reference(size):
    c = IC.case(*size)
    A, _, G, D = c["planes"]
    dif, spec = R.resolve(*c["planes"], c["cb"], c["radiance"], 3, SEED)
    for intensity in (1.0, 0.35, 0.0):
        got = native.indirect_compose_host(c["color"], A, G, D, dif, spec, S.IndirectParams(3, SEED, intensity), 3)
        same_bytes(got, R.compose(c["color"], A, G, D, dif, spec, intensity), f"compose {size} {intensity}")
        assert np.array_equal(got[c["miss"]], c["color"][c["miss"]]) and np.array_equal(got[..., 3], c["color"][..., 3])
    if size != (1, 1):
        assert not np.array_equal(native.indirect_compose_host(c["color"], A, G, D, dif, spec, S.IndirectParams(3, SEED, 1.0)), c["color"])


def test_thread_count_does_not_matter():
    c = IC.case(61, 37)
    A, _, G, D = c["planes"]
    p = S.IndirectParams(3, SEED, 0.7)
    rays1 = native.indirect_rays_host(*c["planes"], c["cb"], p, 1)
    dif1, spec1 = native.indirect_resolve_host(*c["planes"], c["cb"], c["radiance"], p, 1)
    out1 = native.indirect_compose_host(c["color"], A, G, D, dif1, spec1, p, 1)
    for n in (2, 5, 16, 64, 0):
        assert native.indirect_rays_host(*c["planes"], c["cb"], p, n).tobytes() == rays1.tobytes(), n
        dif, spec = native.indirect_resolve_host(*c["planes"], c["cb"], c["radiance"], p, n)
        same_bytes(dif, dif1, f"{n} threads"); same_bytes(spec, spec1, f"{n} threads")
        same_bytes(native.indirect_compose_host(c["color"], A, G, D, dif, spec, p, n), out1, f"{n} threads")


# ---------------------------------------------------------------- 3. the statement itself
def test_statement_is_close_to_float64_and_its_directions_are_unit():
    worst, worst_unit, excluded, hits = 0.0, 0.0, 0, 0
    for size in IC.SIZES:
        c = IC.case(*size)
        a, b = R.lobes(*c["planes"], c["cb"], SEED), R.lobes(*c["planes"], c["cb"], SEED, F=np.float64)
        hit = a["hit"]
        # a pixel whose cull decision differs between binary32 and binary64 sits on that decision: left out, and counted
        same = hit & (a["traced_d"] == b["traced_d"]) & (a["traced_s"] == b["traced_s"])
        excluded += int((hit & ~same).sum()); hits += int(hit.sum())
        for key, mask in (("dir_d", same & a["traced_d"]), ("dir_s", same & a["traced_s"])):
            if mask.any():
                worst = max(worst, float(np.abs(a[key][mask].astype(np.float64) - b[key][mask]).max()))      # unit vectors: the largest value in play is 1
                worst_unit = max(worst_unit, float(np.abs(np.linalg.norm(a[key][mask].astype(np.float64), axis=-1) - 1).max()))
        mask = same & a["traced_s"]
        if mask.any():
            worst = max(worst, float(np.abs(a["w_s"][mask].astype(np.float64) - b["w_s"][mask]).max() / b["w_s"][mask].max()))
    print(f"statement vs float64: largest deviation {worst:.3e}; |dir| - 1 at most {worst_unit:.3e}; {excluded} of {hits} hit pixels on a cull decision")
    assert excluded <= CULL_SHARE_CAP * hits
    assert worst <= 4 * MEASURED_STATEMENT
    # a direction within that bound of the float64 formulation's, which is unit to the rounding of the float32 normal it starts from, is unit
    # within the same bound (measured: 7.9e-7)
    assert worst_unit <= 4 * MEASURED_STATEMENT


def test_draws_follow_the_definition():
    """s = pcg_hash(g + pcg_hash(frameSeed)), four draws, rng = s for the diffuse record and pcg_hash(s) for the specular one: against a
    scalar restatement in Python integers."""
    def pcg(v):
        state = (v * 747796405 + 2891336453) & 0xFFFFFFFF
        word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & 0xFFFFFFFF
        return (word >> 22) ^ word
    c = IC.case(33, 9)
    rays = native.indirect_rays_host(*c["planes"], c["cb"], S.IndirectParams(3, SEED))
    for (x, y) in ((0, 0), (32, 8), (7, 5), IC.SPECIAL["minus_z"]):
        s = pcg((y * 33 + x + pcg(SEED)) & 0xFFFFFFFF)
        for _ in range(4):
            s = pcg(s)
        if not np.isnan(rays["origin"][0, y, x]).any():
            assert int(rays["rng"][0, y, x]) == s
        if not np.isnan(rays["origin"][1, y, x]).any():
            assert int(rays["rng"][1, y, x]) == pcg(s)
    x, y = IC.SPECIAL["minus_z"]
    assert not np.isnan(rays["origin"][:, y, x]).any()


# ---------------------------------------------------------------- 4. errors
def test_argument_errors():
    lib = native.lib
    err = lambda: lib.hrpt_last_error(None).decode()
    c = IC.case(33, 9)
    W, H = 33, 9
    planes = [np.ascontiguousarray(p) for p in c["planes"]]
    dif, spec, color = (np.full((H, W, 4), 7.0, np.float32) for _ in range(3))
    rays = np.zeros((2, H, W), S.Ray); rays.view(np.uint8)[:] = 7
    rad = np.ascontiguousarray(c["radiance"])
    cb = np.ascontiguousarray(c["cb"])
    ptrs = [p.ctypes.data for p in planes]
    im = S.IndirectImages(*ptrs, dif.ctypes.data, spec.ctypes.data, color.ctypes.data)
    ok = S.IndirectParams(3, SEED, 1.0)
    ref = lambda v: C.byref(v) if v is not None else None
    ray = lambda images=im, w=W, h=H, constants=cb.ctypes.data, p=ok, r=rays.ctypes.data: lib.hrpt_indirect_rays_host(ref(images), w, h, constants, ref(p), r, 1)
    res = lambda images=im, w=W, h=H, constants=cb.ctypes.data, p=ok, r=rad.ctypes.data: lib.hrpt_indirect_resolve_host(ref(images), w, h, constants, ref(p), r, 1)
    com = lambda images=im, w=W, h=H, p=ok: lib.hrpt_indirect_compose_host(ref(images), w, h, ref(p), 1)
    rule = ": no lobe flag (HRPT_INDIRECT_DIFFUSE | HRPT_INDIRECT_SPECULAR), unknown flag bits, non-zero reserved or an intensity that is not finite"
    bad = [S.IndirectParams(0, 0, 1.0), S.IndirectParams(0x200, 0, 1.0), S.IndirectParams(3 | 4, 0, 1.0), S.IndirectParams(3 | 0x80000000, 0, 1.0),
           S.IndirectParams(3, 0, math.nan), S.IndirectParams(3, 0, math.inf), S.IndirectParams(3, 0, -math.inf)]
    p = S.IndirectParams(3, 0, 1.0); p.reserved = 1
    bad.append(p)
    for name, call in (("hrpt_indirect_rays_host", ray), ("hrpt_indirect_resolve_host", res), ("hrpt_indirect_compose_host", com)):
        for p in bad:
            assert call(p=p) == -1 and err() == name + rule, (name, p.flags)
        assert call(p=None) == -1 and err() == name + ": null argument"
        assert call(images=None) == -1 and err() == name + ": null images"
        for w, h in ((0, 9), (33, 0), (65536, 9)):
            assert call(w=w, h=h) == -1 and err() == name + ": size must be 1..65535"
    for name, call in (("hrpt_indirect_rays_host", ray), ("hrpt_indirect_resolve_host", res)):
        assert call(constants=None) == -1 and err() == name + ": null argument"
        for k in range(4):
            q = ptrs + [dif.ctypes.data, spec.ctypes.data, None]; q[k] = None
            assert call(images=S.IndirectImages(*q)) == -1 and err() == name + ": null image", k
    assert ray(r=None) == -1 and err() == "hrpt_indirect_rays_host: null image"
    assert res(r=None) == -1 and err() == "hrpt_indirect_resolve_host: null or aliased radiance"
    assert res(r=dif.ctypes.data) == -1 and err() == "hrpt_indirect_resolve_host: null or aliased radiance"
    # a flagged lobe needs its plane; the other plane may be absent
    assert res(images=S.IndirectImages(*ptrs, None, spec.ctypes.data, None)) == -1 and err() == "hrpt_indirect_resolve_host: null image for a flagged lobe"
    assert res(images=S.IndirectImages(*ptrs, dif.ctypes.data, None, None)) == -1 and err() == "hrpt_indirect_resolve_host: null image for a flagged lobe"
    alias = "hrpt_indirect_resolve_host: an output image must differ from every other image"
    for k in range(4):
        assert res(images=S.IndirectImages(*ptrs, ptrs[k], spec.ctypes.data, None)) == -1 and err() == alias
        assert res(images=S.IndirectImages(*ptrs, dif.ctypes.data, ptrs[k], None)) == -1 and err() == alias
    assert res(images=S.IndirectImages(*ptrs, dif.ctypes.data, dif.ctypes.data, None)) == -1 and err() == alias
    for k in (0, 2, 3, 4, 5, 6):
        q = ptrs + [dif.ctypes.data, spec.ctypes.data, color.ctypes.data]; q[k] = None
        assert com(images=S.IndirectImages(*q)) == -1 and err() == "hrpt_indirect_compose_host: null image", k
    for k in (0, 2, 3):
        q = ptrs + [dif.ctypes.data, spec.ctypes.data, ptrs[k]]
        assert com(images=S.IndirectImages(*q)) == -1 and err() == "hrpt_indirect_compose_host: colorInOut must differ from every other image"
    assert com(images=S.IndirectImages(*ptrs, dif.ctypes.data, spec.ctypes.data, dif.ctypes.data)) == -1
    assert com(images=S.IndirectImages(*ptrs, dif.ctypes.data, spec.ctypes.data, spec.ctypes.data)) == -1
    # an error changes nothing
    assert (dif == 7.0).all() and (spec == 7.0).all() and (color == 7.0).all() and (rays.view(np.uint8) == 7).all()
    # one lobe flagged: the other plane may be absent, and the call succeeds
    assert res(images=S.IndirectImages(*ptrs, dif.ctypes.data, None, None), p=S.IndirectParams(1, SEED), r=np.ascontiguousarray(rad[:1]).ctypes.data) == 0
    assert not (dif == 7.0).all() and (spec == 7.0).all()
    # the context calls on NULL
    assert lib.hrpt_indirect_lighting(None, cb.ctypes.data, C.byref(ok)) == -1
    assert lib.hrpt_indirect_compose(None, C.byref(ok)) == -1
    assert lib.hrpt_indirect_lighting_device(None, C.byref(im), W, H, cb.ctypes.data, C.byref(ok), None) == -1
    assert lib.hrpt_indirect_compose_device(None, C.byref(im), W, H, C.byref(ok), None) == -1
    assert lib.hrpt_read_indirect(None, 0, None, 0) == -1 and lib.hrpt_get_indirect_device(None, 0, None) == -1


@pytest.mark.parametrize("seed", [5, 6])
def test_host_side_is_clean_under_the_sanitizers(seed):
    """pt_indirect.h + the host executors + a driver with its own main, built with AddressSanitizer and UBSan (`make indirect_asan`), over
    every image size and lobe combination with misses, absent planes and hostile planes, radiance and constants on exactly sized heap arrays.
    Nothing is loaded into Python."""
    subprocess.check_call(["make", "-C", CSRC, "indirect_asan"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(CSRC, "build", "indirect_asan"), str(seed)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "no report" in r.stdout
