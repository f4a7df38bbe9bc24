"""The demodulate and compose stages without a GPU (hrpt_demodulate_host / hrpt_compose_host): the host executors of
csrc/pt_modulation.h against the NumPy restatement tests/modulation_reference.py, bit for bit on uint32 views with no pixel left out; the
properties the stages promise, checked on both; the probe of the factor; the argument errors; what the stages are for (a textured plane
through demodulate -> denoise -> compose against denoise alone); and the sanitizer build of the host side (`make modulation_asan`, a
stand-alone program)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hobbyrenderer_amd import native, structs as S
import denoise_cases as DC
import modulation_cases as MC
import modulation_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hobbyrenderer_amd", "csrc")
SYMBOLS = ("hrpt_demodulate_host", "hrpt_compose_host", "hrpt_demodulate_device", "hrpt_compose_device", "hrpt_demodulate", "hrpt_compose",
           "hrpt_read_modulation", "hrpt_get_modulation_device", "hrpt_modulation_probe", "hrpt_set_denoise_noise")
KEYS = ("color", "albedo", "normal", "geo", "depth")
EPS = 2.0 ** -24


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what):
    a, b = u32(got), u32(want)
    bad = (a != b).any(-1)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (x={x}, y={y}): {got[y, x]} != {want[y, x]}")


def lib_demodulate(c, floor=0.04, emissive=True, nthreads=3):
    return native.demodulate_host(*[c[k] for k in KEYS], c["view"], S.ModulationParams(floor), emissive=c["emissive"] if emissive else None, nthreads=nthreads)


def ref_demodulate(c, floor=0.04, emissive=True):
    return R.demodulate(*[c[k] for k in KEYS], c["view"], floor=floor, emissive=c["emissive"] if emissive else None)


_cases = {}


def case(w, h):
    if (w, h) not in _cases:
        _cases[(w, h)] = MC.case(w, h)
    return _cases[(w, h)]


def test_symbols_are_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "hobbyrt_pt.h")).read()
    for name in SYMBOLS:
        assert name in native.EXPORTS and hasattr(native.lib, name) and f" {name}(" in header, name
    assert "#define HRPT_ABI_VERSION 3" in header and S.ABI_VERSION == 3
    assert C.sizeof(S.ModulationParams) == 16 and C.sizeof(S.DemodulateImages) == 64 and C.sizeof(S.ComposeImages) == 32
    p = S.ModulationParams()
    assert p.floor == np.float32(0.04) and p.flags == 0 and list(p.reserved) == [0, 0]


# ---------------------------------------------------------------- 1. library == NumPy, bit for bit
@pytest.mark.parametrize("size", MC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("floor", MC.FLOORS)
def test_host_equals_reference(floor, size):
    w, h = size
    c = case(w, h)
    for emissive in (True, False):
        what = f"{w}x{h} floor={floor} emissive={emissive}"
        ref_col, ref_mod = ref_demodulate(c, floor, emissive)
        lib_col, lib_mod = lib_demodulate(c, floor, emissive)
        assert_same(lib_mod, ref_mod, what + ": modulation")
        assert_same(lib_col, ref_col, what + ": demodulated colour")
        e = c["emissive"] if emissive else None
        ref_back = R.compose(ref_col, ref_mod, e)
        assert_same(native.compose_host(lib_col, lib_mod, e, nthreads=3), ref_back, what + ": composed colour")
        # compose over an image the filters would have changed: any colour, not only demodulate's
        other = DC.TC.radiance(w, h, 77)
        assert_same(native.compose_host(other, lib_mod, e, nthreads=2), R.compose(other, ref_mod, e), what + ": composed, other colour")


def test_the_case_does_what_it_is_there_for():
    w, h = 64, 36
    c = case(w, h)
    hit, lit = c["hit"], c["lit"]
    assert (~hit).sum() > 100 and 20 < lit.sum() < 0.1 * hit.sum()
    assert ((c["emissive"][..., :3] > c["color"][..., :3]) & lit[..., None]).sum() > 10          # the clamp is exercised
    assert ((c["emissive"][..., :3] < c["color"][..., :3]) & lit[..., None]).sum() > 10
    a = c["albedo"][hit][:, :3]
    assert (a == 0).any() and (a == 1).any()
    nz = np.abs(c["normal"][..., 2][hit])
    assert (nz == 1).sum() >= 2 and ((nz > 0.9985) & (nz < 0.999)).any() and ((nz > 0.999) & (nz < 0.9995)).any()
    metal, rough = c["geo"][..., 3][hit], c["normal"][..., 3][hit]
    assert all((metal == np.float32(m)).any() for m in (0, 0.5, 1)) and all((rough == np.float32(r)).any() for r in (0.04, 1))
    assert ((rough >= 0.5) & (rough < 0.53)).any()
    _, mod = ref_demodulate(c, 0.04)
    assert (mod[hit][:, :3] == np.float32(0.04)).any()               # the default floor bites somewhere (dark metals) ...
    assert (mod[hit & (c["geo"][..., 3] == 0)][:, :3] >= np.float32(0.04)).all()


def test_in_place_and_thread_count_independence():
    w, h = 37, 23
    c = case(w, h)
    ref_col, ref_mod = ref_demodulate(c, 0.04)
    imgs = [np.ascontiguousarray(c[k], np.float32).copy() for k in KEYS]
    em, mod = c["emissive"].copy(), np.empty_like(imgs[0])
    im = S.DemodulateImages(*[a.ctypes.data for a in imgs], em.ctypes.data, imgs[0].ctypes.data, mod.ctypes.data)
    p = S.ModulationParams()
    assert native.lib.hrpt_demodulate_host(C.byref(im), w, h, c["view"].ctypes.data, C.byref(p), 2) == 0
    assert_same(imgs[0], ref_col, "demodulate in place: colour")
    assert_same(mod, ref_mod, "demodulate in place: modulation")
    cm = S.ComposeImages(imgs[0].ctypes.data, mod.ctypes.data, em.ctypes.data, imgs[0].ctypes.data)
    assert native.lib.hrpt_compose_host(C.byref(cm), w, h, 2) == 0
    assert_same(imgs[0], R.compose(ref_col, ref_mod, c["emissive"]), "compose in place")
    c = case(64, 36)
    one = lib_demodulate(c, nthreads=1)
    for n in (2, 3, 7, 64):
        got = lib_demodulate(c, nthreads=n)
        assert np.array_equal(u32(got[0]), u32(one[0])) and np.array_equal(u32(got[1]), u32(one[1])), n
        assert np.array_equal(u32(native.compose_host(one[0], one[1], c["emissive"], nthreads=n)), u32(native.compose_host(one[0], one[1], c["emissive"], nthreads=1)))
    for n in (0, -1, 1000):                                  # the clamp: one per hardware thread up to 16; at most 256, and no more than rows
        got = lib_demodulate(c, nthreads=n)
        assert np.array_equal(u32(got[0]), u32(one[0])) and np.array_equal(u32(got[1]), u32(one[1])), n
        assert np.array_equal(u32(native.compose_host(one[0], one[1], c["emissive"], nthreads=n)), u32(native.compose_host(one[0], one[1], c["emissive"], nthreads=1))), n


# ---------------------------------------------------------------- 2. properties, on the reference and on the library
@pytest.mark.parametrize("floor", MC.FLOORS)
def test_properties(floor):
    w, h = 64, 36
    c = case(w, h)
    hit, miss = c["hit"], ~c["hit"]
    color, em = c["color"], c["emissive"]
    for name, (col, mod) in (("library", lib_demodulate(c, floor)), ("reference", ref_demodulate(c, floor))):
        back = (native.compose_host if name == "library" else R.compose)(col, mod, em)
        # a miss passes through bit for bit with modulation (1, 1, 1, 0); alpha passes through everywhere
        assert np.array_equal(u32(col[miss]), u32(color[miss])) and np.array_equal(u32(back[miss]), u32(color[miss])), name
        assert (mod[miss] == np.float32([1, 1, 1, 0])).all() and (mod[hit][:, 3] == 1).all(), name
        assert np.array_equal(u32(col[..., 3]), u32(color[..., 3])) and np.array_equal(u32(back[..., 3]), u32(color[..., 3])), name
        m = mod[..., :3]
        assert (m >= np.float32(floor)).all() and np.isfinite(m).all(), name
        metal = c["geo"][..., 3]
        assert (m[hit & (metal == 0)] >= np.float32(0.04)).all(), name
        # M == F where metal == 1. A black metal has f0 = 0.04 + 1 * (0 - 0.04) = 0, so its factor is p = pow(1 - VoH, 5) itself (floored far
        # below); F of the real albedo follows from p by Schlick's formula, and the albedo term (albedo * 0) * (1 - F) adds nothing.
        metal1 = hit & (metal == 1)
        assert metal1.sum() > 100
        black = dict(c, albedo=np.zeros_like(c["albedo"]))
        p = (lib_demodulate if name == "library" else ref_demodulate)(black, 1e-30)[1][metal1][:, :3]
        f0 = (np.float32(0.04) + np.float32(1) * (c["albedo"][metal1][:, :3] - np.float32(0.04))).astype(np.float32)
        fresnel = (f0 + (np.float32(1) - f0) * p).astype(np.float32)
        assert np.array_equal(u32(np.maximum(fresnel, np.float32(floor))), u32(m[metal1])), name
        # the two round-trip bounds, on hits whose channel is a normal number with x >= E >= 0
        x, e = color[..., :3].astype(np.float64), em[..., :3].astype(np.float64)
        err = np.abs(back[..., :3].astype(np.float64) - x)
        ok = hit[..., None] & (x >= e) & (x > 1e-30) & np.isfinite(x)
        with_e, without_e = ok & (e > 0), ok & (e == 0)
        assert with_e.sum() > 20 and without_e.sum() > 1000
        print(f"{name} floor={floor}: round trip max err / x = {(err[with_e] / x[with_e]).max() / EPS:.2f} eps with E, "
              f"{(err[without_e] / x[without_e]).max() / EPS:.2f} eps without")
        assert (err[with_e] <= 5 * EPS * x[with_e]).all(), name
        assert (err[without_e] <= 3 * EPS * x[without_e]).all(), name
        # where emissive exceeds the colour the demodulated channel is exactly 0 and compose returns E
        over = hit[..., None] & (em[..., :3] > color[..., :3])
        assert over.sum() > 10 and (col[..., :3][over] == 0).all() and np.array_equal(u32(back[..., :3][over]), u32(em[..., :3][over])), name


# ---------------------------------------------------------------- 3. the probe: branches no camera produces reliably
PROBES = {
    "N = V = +z: Vlocal = (0, 0, 1), lensq == 0": ((0.0, 0.0, 1.0), (0.0, 0.0, 1.0)),
    "up = z (|N.z| < 0.999)": ((0.6, 0.0, 0.8), (0.0, 0.6, 0.8)),
    "up = x (|N.z| >= 0.999)": ((0.0, 0.0, -1.0), (0.28, 0.0, -0.96)),
    "grazing V": ((0.0, 1.0, 0.0), (0.9999995, 0.001, 0.0)),
    "V.N < 0": ((0.0, 1.0, 0.0), (0.6, -0.8, 0.0)),
}


@pytest.mark.parametrize("name", sorted(PROBES))
def test_probe_equals_reference(name):
    n, v = [np.float32(x) for x in PROBES[name]]
    albedo = np.float32([0.0, 0.5, 1.0])
    for rough in (0.04, 0.5, 1.0):
        for metal in (0.0, 0.5, 1.0):
            for floor in MC.FLOORS:
                lib = native.modulation_probe(albedo, n, v, rough, metal, floor)
                ref = R.factor(albedo, n, v, rough, metal, floor)
                assert np.array_equal(u32(lib), u32(ref)), (name, rough, metal, floor, lib, ref)
                assert np.isfinite(lib).all() and (lib >= np.float32(floor)).all()
    if name.startswith("N = V"):
        # H = (0, 0, 1) up to rounding, l = V, VoH = 1: pow(0, 5) = 0 and F = f0 exactly
        lib = native.modulation_probe(albedo, n, v, 0.5, 0.0, 1e-6)
        np.testing.assert_allclose(lib, np.float32(0.04) + albedo * (1 - np.float32(0.04)), rtol=1e-5)


def test_probe_null_pointers():
    v = np.float32([0, 0, 1])
    out = np.empty(3, np.float32)
    for k in range(4):
        args = [v.ctypes.data, v.ctypes.data, v.ctypes.data, out.ctypes.data]
        args[k] = None
        assert native.lib.hrpt_modulation_probe(args[0], args[1], args[2], 0.5, 0.0, 0.04, args[3]) == -1


# ---------------------------------------------------------------- 4. argument errors
def test_argument_errors():
    w, h = 37, 23
    c = case(w, h)
    imgs = dict(zip(KEYS, [np.ascontiguousarray(c[k], np.float32).copy() for k in KEYS]))
    imgs["emissive"] = c["emissive"].copy()
    out, mod = np.empty_like(imgs["color"]), np.empty_like(imgs["color"])
    view = c["view"]
    err = lambda: native.lib.hrpt_last_error(None)                 # noqa: E731
    text = lambda: err().decode()                                  # noqa: E731 -- the whole text, as the library has always worded it
    PARAMS = "hrpt_demodulate_host: floor must be finite and > 0, flags 0, reserved 0"

    def images(**kw):
        ptrs = {k: a.ctypes.data for k, a in imgs.items()}
        ptrs.update(colorOut=out.ctypes.data, modulationOut=mod.ctypes.data)
        ptrs.update(kw)
        return S.DemodulateImages(ptrs["color"], ptrs["albedo"], ptrs["normal"], ptrs["geo"], ptrs["depth"], ptrs["emissive"], ptrs["colorOut"], ptrs["modulationOut"])

    def call(im=None, ww=w, hh=h, v=view, p=None):
        im = im if im is not None else images()
        p = p if p is not None else S.ModulationParams()
        return native.lib.hrpt_demodulate_host(C.byref(im) if im != "null" else None, ww, hh, v.ctypes.data if v is not None else None,
                                               C.byref(p) if p != "null" else None, 1)
    assert call() == 0
    assert call(im="null") == -1 and call(v=None) == -1 and call(p="null") == -1
    for kw in (dict(im="null"), dict(v=None), dict(p="null")):
        assert call(**kw) == -1 and text() == "hrpt_demodulate_host: null argument", kw
    for k in KEYS + ("colorOut", "modulationOut"):
        assert call(im=images(**{k: None})) == -1, k
        assert text() == "hrpt_demodulate_host: null image (only emissive may be NULL)", k
    assert call(im=images(emissive=None)) == 0
    for k in KEYS + ("emissive",):                                 # forbidden aliasing
        assert call(im=images(modulationOut=imgs[k].ctypes.data)) == -1, k
        assert b"modulationOut must differ" in err()
        assert text() == "hrpt_demodulate_host: modulationOut must differ from every input", k
        assert call(im=images(colorOut=imgs[k].ctypes.data)) == (0 if k == "color" else -1), k
        assert k == "color" or text() == "hrpt_demodulate_host: colorOut may equal color, but no other input", k
    assert call(im=images(colorOut=mod.ctypes.data)) == -1
    assert text() == "hrpt_demodulate_host: modulationOut must differ from colorOut"
    wrong = view.copy(); wrong["m_ViewportSize"] = (w + 1, h)
    assert call(v=wrong) == -1 and b"m_ViewportSize" in err()
    assert text() == "hrpt_demodulate_host: view->m_ViewportSize does not match the image size"
    assert call(ww=0) == -1 and call(hh=0) == -1 and call(ww=65536) == -1 and call(hh=65536) == -1
    for ww, hh in ((0, h), (w, 0), (0, 0), (65536, h), (w, 65536)):       # reported before the view is compared with it
        assert call(ww=ww, hh=hh) == -1 and text() == "hrpt_demodulate_host: size must be 1..65535", (ww, hh)
    for floor in (float("nan"), float("inf"), -float("inf"), 0.0, -0.04):
        assert call(p=S.ModulationParams(floor)) == -1, floor
        assert b"floor" in err()
        assert text() == PARAMS, floor
    assert call(p=S.ModulationParams(1e-30)) == 0 and call(p=S.ModulationParams(3e38)) == 0
    assert call(p=S.ModulationParams(flags=1)) == -1 and call(p=S.ModulationParams(flags=0x80000000)) == -1
    assert text() == PARAMS
    for k in range(2):
        p = S.ModulationParams(); p.reserved[k] = 1
        assert call(p=p) == -1
        assert text() == PARAMS, k

    def cimages(**kw):
        ptrs = dict(color=imgs["color"].ctypes.data, modulation=mod.ctypes.data, emissive=imgs["emissive"].ctypes.data, colorOut=out.ctypes.data)
        ptrs.update(kw)
        return S.ComposeImages(ptrs["color"], ptrs["modulation"], ptrs["emissive"], ptrs["colorOut"])

    def ccall(im=None, ww=w, hh=h):
        im = im if im is not None else cimages()
        return native.lib.hrpt_compose_host(C.byref(im) if im != "null" else None, ww, hh, 1)
    assert ccall() == 0 and ccall(im="null") == -1
    assert text() == "hrpt_compose_host: null argument"
    for k in ("color", "modulation", "colorOut"):
        assert ccall(im=cimages(**{k: None})) == -1, k
        assert text() == "hrpt_compose_host: null image (only emissive may be NULL)", k
    assert ccall(im=cimages(emissive=None)) == 0
    assert ccall(im=cimages(colorOut=imgs["color"].ctypes.data)) == 0
    assert ccall(im=cimages(colorOut=mod.ctypes.data)) == -1 and ccall(im=cimages(colorOut=imgs["emissive"].ctypes.data)) == -1
    for k in (mod, imgs["emissive"]):
        assert ccall(im=cimages(colorOut=k.ctypes.data)) == -1 and text() == "hrpt_compose_host: colorOut may equal color, but not modulation or emissive"
    assert ccall(ww=0) == -1 and ccall(hh=0) == -1 and ccall(ww=65536) == -1
    for ww, hh in ((0, h), (w, 0), (0, 0), (65536, h), (w, 65536)):
        assert ccall(ww=ww, hh=hh) == -1 and text() == "hrpt_compose_host: size must be 1..65535", (ww, hh)
    # context calls on a NULL context
    p = S.ModulationParams()
    assert native.lib.hrpt_demodulate(None, view.ctypes.data, C.byref(p)) == -1 and native.lib.hrpt_compose(None) == -1
    assert native.lib.hrpt_demodulate_device(None, C.byref(images()), w, h, view.ctypes.data, C.byref(p), None) == -1
    assert native.lib.hrpt_compose_device(None, C.byref(cimages()), w, h, None) == -1
    assert native.lib.hrpt_read_modulation(None, out.ctypes.data, out.nbytes) == -1
    assert native.lib.hrpt_get_modulation_device(None, None) == -1 and native.lib.hrpt_set_denoise_noise(None, None) == -1


# ---------------------------------------------------------------- 5. what the stages are for
def test_a_texture_survives_the_denoiser_only_when_it_is_demodulated():
    """A textured non-metal plane at age 0 (DC.flat_plane(64, 36, 5) under the 2-texel checker albedo): Output = signal * Mf with an i.i.d.
    signal in [0.5, 1.5]. The denoiser's edge stops do not see albedo, so on Output itself it averages the checker away and ends WORSE
    than the raw image; between demodulate and compose it filters the signal alone. RMSE against mean(signal) * Mf over the interior
    (6-texel margin). Measured on the NumPy reference: with 0.0628, raw 0.1806, without 0.3873; the test asserts
    the ordering only."""
    c = MC.textured_plane()
    h, w = c["albedo"].shape[:2]
    signal = c["signal"]
    results = {}
    for name, demod, den, comp in (("library", native.demodulate_host, native.denoise_host, native.compose_host),
                                   ("reference", None, None, None)):
        if name == "library":
            mod = demod(np.ones((h, w, 4), np.float32), c["albedo"], c["normal"], c["geo"], c["depth"], c["view"])[1]
        else:
            mod = R.modulation(c["albedo"], c["normal"], c["geo"], c["depth"], c["view"])
        output = np.zeros((h, w, 4), np.float32)                 # alpha 0: the age the denoiser reads
        output[..., :3] = signal * mod[..., :3]
        if name == "library":
            d, m = demod(output, c["albedo"], c["normal"], c["geo"], c["depth"], c["view"])
            with_ = comp(den(d, c["depth"], c["normal"], c["geo"], c["view"], DC.params(3.0, 0)), m)
            without = den(output, c["depth"], c["normal"], c["geo"], c["view"], DC.params(3.0, 0))
        else:
            import denoise_reference as DR
            d, m = R.demodulate(output, c["albedo"], c["normal"], c["geo"], c["depth"], c["view"])
            with_ = R.compose(DR.denoise(d, c["depth"], c["normal"], c["geo"], c["view"], radius=3.0, frame=0), m)
            without = DR.denoise(output, c["depth"], c["normal"], c["geo"], c["view"], radius=3.0, frame=0)
        truth = signal.astype(np.float64).mean() * mod[..., :3].astype(np.float64)
        inner = (slice(6, -6), slice(6, -6))

        def rmse(img):
            return float(np.sqrt(((img[..., :3].astype(np.float64) - truth)[inner] ** 2).mean()))
        r = results[name] = (rmse(with_), rmse(output), rmse(without))
        print(f"{name}: rmse with demodulate/compose {r[0]:.4f}, raw {r[1]:.4f}, denoise alone {r[2]:.4f}")
        assert r[0] < r[1] < r[2], (name, r)
    assert results["library"] == results["reference"]            # the same bits give the same figures


# ---------------------------------------------------------------- 6. sanitizer build of the host side
@pytest.mark.parametrize("seed", [5, 6])
def test_host_side_is_clean_under_the_sanitizers(seed):
    """pt_modulation.h + the host executors + a driver with its own main, built with AddressSanitizer and UBSan (`make modulation_asan`),
    over random and hostile values (NaN, inf, negative albedo, zero normals, view depth 0) on exactly sized heap images. Nothing is loaded
    into Python."""
    subprocess.check_call(["make", "-C", CSRC, "modulation_asan"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(CSRC, "build", "modulation_asan"), str(seed)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "no report" in r.stdout
