"""The denoise stage without a GPU (hrpt_denoise_host): the host executor of csrc/pt_denoise.h against the NumPy
restatement tests/denoise_reference.py, bit for bit on uint32 views with no pixel left out; the properties the stage promises, checked on
both; the argument errors; and the sanitizer build of the host side (`make denoise_asan`, a stand-alone program)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hobbyrenderer_amd import native, structs as S
import denoise_cases as DC
import denoise_reference as R
from temporal_reference import _exp, _log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hobbyrenderer_amd", "csrc")
SYMBOLS = ("hrpt_denoise_host", "hrpt_denoise_device", "hrpt_denoise")
KEYS = ("input", "depth", "normal", "geo")


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what):
    a, b = u32(got), u32(want)
    bad = (a != b).any(-1)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (x={x}, y={y}): {got[y, x]} != {want[y, x]}")


def lib_call(c, radius=3.0, frame=0, noise=None, color=None, nthreads=3, **kw):
    return native.denoise_host(*[c[k] for k in KEYS], c["view"], DC.params(radius, frame, **kw), noise=noise, color=color, nthreads=nthreads)


def ref_call(c, radius=3.0, frame=0, noise=None, color=None, **kw):
    return R.denoise(*[c[k] for k in KEYS], c["view"], radius=radius, frame=frame, noise=noise, color=color, **kw)


def test_symbols_are_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "hobbyrt_pt.h")).read()
    for name in SYMBOLS:
        assert name in native.EXPORTS and hasattr(native.lib, name) and f" {name}(" in header, name
    assert "#define HRPT_ABI_VERSION 3" in header and S.ABI_VERSION == 3
    assert "#define HRPT_DENOISE_OUTPUT_ONLY 1u" in header and S.DENOISE_OUTPUT_ONLY == 1
    assert C.sizeof(S.DenoiseParams) == 40 and C.sizeof(S.DenoiseImages) == 64
    p = S.DenoiseParams()
    assert [p.radius, p.phi, p.lumaPhi, p.depthPhi, p.normalPhi, p.roughnessPhi] == [3.0, 0.5, 5.0, 2.0, 50.0, 50.0]
    assert (p.iterations, p.frame, p.flags, p.reserved) == (1, 0, 0, 0)


# ---------------------------------------------------------------- 1. library == NumPy, bit for bit
@pytest.mark.parametrize("size", DC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("radius", DC.RADII)
def test_host_equals_reference(radius, size):
    w, h = size
    c = DC.case(w, h)
    tile = DC.caller_tile()
    for frame in DC.FRAMES:
        for noise in (None, tile):
            what = f"{w}x{h} radius={radius} frame={frame} tile={'caller' if noise is not None else 'default'}"
            (ref, ref_col), d = ref_call(c, radius, frame, noise, c["color"], details=True)
            lib, lib_col = lib_call(c, radius, frame, noise, c["color"])
            assert_same(lib, ref, what + ": output")
            assert_same(lib_col, ref_col, what + ": colorOut")
            assert_same(lib_call(c, radius, frame, noise), ref, what + ": output without the colour pair")
            # the case does what it is there for
            hit = c["hit"]
            nu = np.stack([t[2] for t in d["taps"]])[:, hit]
            nv = np.stack([t[3] for t in d["taps"]])[:, hit]
            if radius >= 3:                                    # taps cross every image edge
                assert (nu < 0).any() and (nu > 1).any() and (nv < 0).any() and (nv > 1).any(), what
            if radius == 3:                                    # both ends of the clamp of the kernel size, and sizes in between
                disk = d["disk"][hit]
                assert (disk == 2).any() and (disk == 12).any() and ((disk > 2) & (disk < 12)).any()
    age = c["input"][..., 3][c["hit"]]
    assert (age == 0).any() and ((age > 0) & (age < 64)).any() and (age > 64).any()
    # With the age clamped at 64 and one image for both signals, a + a2 <= 128 and exp(-1.28) = 0.278: the 0.15 floor of the age falloff
    # is out of reach of every finite age (section 18); the smallest falloff is the clamp's.
    assert d["age_falloff"][c["hit"]].min() == _exp(np.float32(-128.0) * np.float32(0.01)) > 0.15


def test_three_chained_passes_with_doubling_radius():
    w, h = 37, 23
    c = DC.case(w, h)
    frame, iterations = 0xFFFFFFFF, 3                        # frame * iterations + i wraps
    lib_in = ref_in = c["input"]
    for i in range(iterations):
        radius, f = 3.0 * (1 << i), (frame * iterations + i) & 0xFFFFFFFF
        lib = native.denoise_host(lib_in, c["depth"], c["normal"], c["geo"], c["view"], DC.params(radius, f))
        ref = R.denoise(ref_in, c["depth"], c["normal"], c["geo"], c["view"], radius=radius, frame=f)
        assert_same(lib, ref, f"pass {i}")
        lib_in, ref_in = lib, ref
    assert np.array_equal(u32(ref[..., 3]), u32(c["input"][..., 3]))


@pytest.mark.parametrize("size", [(1, 1), (2, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiny_images(size):
    w, h = size
    c = DC.case(w, h)
    assert c["hit"].all()
    for radius in DC.RADII:
        for frame in (0, 4097):
            ref, ref_col = ref_call(c, radius, frame, None, c["color"])
            lib, lib_col = lib_call(c, radius, frame, None, c["color"])
            assert_same(lib, ref, f"{w}x{h} radius={radius} frame={frame}: output")
            assert_same(lib_col, ref_col, f"{w}x{h} radius={radius} frame={frame}: colorOut")


def test_color_out_may_be_color():
    w, h = 37, 23
    c = DC.case(w, h)
    imgs = [np.ascontiguousarray(c[k], np.float32).copy() for k in KEYS]
    color = c["color"].copy()
    out = np.empty_like(imgs[0])
    im = S.DenoiseImages(*[a.ctypes.data for a in imgs], None, out.ctypes.data, color.ctypes.data, color.ctypes.data)
    p = DC.params(3.0, 5)
    assert native.lib.hrpt_denoise_host(C.byref(im), w, h, c["view"].ctypes.data, C.byref(p), 2) == 0
    ref, ref_col = ref_call(c, 3.0, 5, None, c["color"])
    assert_same(out, ref, "in place: output")
    assert_same(color, ref_col, "in place: colorOut")


# ---------------------------------------------------------------- 2. properties, on the reference and on the library
def test_miss_passes_through_and_age_is_kept_unclamped():
    w, h = 64, 36
    c = DC.case(w, h)
    miss = ~c["hit"]
    assert miss.sum() > 100 and (c["input"][..., 3] > 64).sum() > 100
    for out, col in (lib_call(c, 3.0, 9, color=c["color"]), ref_call(c, 3.0, 9, color=c["color"])):
        assert np.array_equal(u32(out[miss]), u32(c["input"][miss]))
        assert np.array_equal(u32(col[miss][:, :3]), u32(c["input"][miss][:, :3]))
        assert np.array_equal(u32(col[..., 3]), u32(c["color"][..., 3]))             # alpha of colorOut is color's, hits and misses
        assert np.array_equal(u32(out[..., 3]), u32(c["input"][..., 3]))             # the age, unclamped, hits and misses
        assert np.array_equal(u32(out[..., :3]), u32(col[..., :3]))
        assert (u32(out[c["hit"]][:, :3]) != u32(c["input"][c["hit"]][:, :3])).any()  # and the hits were filtered


def test_a_pixel_whose_taps_all_miss_returns_itself_through_log_and_exp():
    w, h = 9, 9
    c = DC.flat_plane(w, h, 4, age=7.0)
    c["depth"][...] = (1e10, 1e10, 0.0, 0.0)
    c["depth"][4, 4] = (6.06, 6.0, 0.0, 0.0)                 # one hit in the middle: the disk is at least 2 texels wide, every tap leaves it
    want = _exp(_log(c["input"][4, 4, :3] + np.float32(1))) - np.float32(1)
    for radius in (0.5, 3.0):
        (ref, d) = ref_call(c, radius, 3, details=True)
        assert all((qx[4, 4], qy[4, 4]) != (4, 4) for qx, qy, _, _ in d["taps"]) and d["total"][4, 4] == 1
        for out in (lib_call(c, radius, 3), ref):
            assert np.array_equal(u32(out[4, 4, :3]), u32(want)) and out[4, 4, 3] == 7.0
            np.testing.assert_allclose(out[4, 4, :3], c["input"][4, 4, :3], rtol=4e-6)


def test_thread_count_independence():
    c = DC.case(64, 36)
    one = lib_call(c, 12.0, 2, nthreads=1)
    for n in (2, 3, 7, 64):
        assert np.array_equal(u32(lib_call(c, 12.0, 2, nthreads=n)), u32(one)), n
    for n in (0, -1, 1000):                                  # the clamp: one per hardware thread up to 16; at most 256, and no more than rows
        assert np.array_equal(u32(lib_call(c, 12.0, 2, nthreads=n)), u32(one)), n


def test_noise_reduction_on_a_flat_plane():
    """A flat plane at age 0 with i.i.d. radiance: one pass lowers the standard deviation over the interior. At age 0 every edge-stopping
    term is relaxed to 1 on a plane (w = 1), so the pass is a 9-texel mean in log space and the ratio is near 1/3; the figure is printed
    and recorded in section 18, the test only asks for strictly smaller."""
    w, h = 64, 36
    c = DC.flat_plane(w, h, 1)
    inner = (slice(4, -4), slice(4, -4), slice(0, 3))
    before = c["input"][inner].astype(np.float64).std()
    for name, out in (("library", lib_call(c)), ("reference", ref_call(c))):
        after = out[inner].astype(np.float64).std()
        print(f"{name}: std {before:.4f} -> {after:.4f}, ratio {after / before:.3f}")
        assert after < before


def test_edge_stop_between_two_half_planes():
    """Normals 90 degrees apart, radiance 0.1 against 10, age 64: across the edge normalDiff = 1 and w = 65^-1/2 = 0.124, so
    wBasicD <= lerp(e^-50, e^-10, 0.124) = 5.6e-6 and wDiff = 0.124 * (5.6e-6)^4.03 < 1e-20; what remains on the dark side is the fp32
    log / exp round trip, ~1e-6 relative at 0.1."""
    w, h = 64, 36
    c = DC.two_half_planes(w, h)
    dark = c["dark"]
    assert dark.sum() > 500
    ref, d = ref_call(c, 3.0, 1, details=True)
    crossing = np.zeros((h, w), bool)                        # dark pixels with a tap on the bright side: the case tests the edge
    for qx, qy, _, _ in d["taps"]:
        crossing |= dark & (qx >= w // 2) & c["hit"][qy, qx]
    assert crossing.sum() > 20
    np.testing.assert_allclose(ref[dark][:, :3], 0.1, rtol=1e-4)      # the reference first
    np.testing.assert_allclose(lib_call(c, 3.0, 1)[dark][:, :3], 0.1, rtol=1e-4)


# ---------------------------------------------------------------- 3. argument errors
def test_argument_errors():
    w, h = 37, 23
    c = DC.case(w, h)
    imgs = [np.ascontiguousarray(c[k], np.float32) for k in KEYS]
    tile = DC.caller_tile()
    out, color, cout = np.empty_like(imgs[0]), c["color"].copy(), np.empty_like(imgs[0])
    view = c["view"]

    def images(**kw):
        ptrs = dict(zip(KEYS, [a.ctypes.data for a in imgs]), noise=tile.ctypes.data, output=out.ctypes.data, color=color.ctypes.data, colorOut=cout.ctypes.data)
        ptrs.update(kw)
        return S.DenoiseImages(ptrs["input"], ptrs["depth"], ptrs["normal"], ptrs["geo"], ptrs["noise"], ptrs["output"], ptrs["color"], ptrs["colorOut"])

    def call(im=None, ww=w, hh=h, v=view, p=None):
        im = im if im is not None else images()
        p = p if p is not None else S.DenoiseParams()
        return native.lib.hrpt_denoise_host(C.byref(im) if im != "null" else None, ww, hh, v.ctypes.data if v is not None else None,
                                            C.byref(p) if p != "null" else None, 1)
    err = lambda: native.lib.hrpt_last_error(None).decode()          # noqa: E731 -- the whole text, as the library has always worded it
    PARAMS = ("hrpt_denoise_host: radius and phi must be finite and > 0, the other phis finite and >= 0, iterations 1..5 with "
              "radius * 2^(iterations - 1) finite, flags HRPT_DENOISE_* only, reserved 0")
    assert call() == 0
    assert call(im="null") == -1 and call(v=None) == -1 and call(p="null") == -1
    for kw in (dict(im="null"), dict(v=None), dict(p="null")):
        assert call(**kw) == -1 and err() == "hrpt_denoise_host: null argument", kw
    for k in KEYS + ("output",):
        assert call(im=images(**{k: None})) == -1, k
        assert err() == "hrpt_denoise_host: null image (only noise, and color with colorOut, may be NULL)", k
    assert call(im=images(noise=None)) == 0 and call(im=images(color=None, colorOut=None)) == 0
    assert call(im=images(color=None)) == -1 and call(im=images(colorOut=None)) == -1
    assert b"both" in native.lib.hrpt_last_error(None)
    assert err() == "hrpt_denoise_host: color and colorOut must both be NULL or both be set"
    assert call(im=images(output=imgs[0].ctypes.data)) == -1
    assert b"output must differ" in native.lib.hrpt_last_error(None)
    assert err() == "hrpt_denoise_host: output must differ from input"
    assert call(im=images(color=imgs[0].ctypes.data)) == -1 and call(im=images(colorOut=imgs[0].ctypes.data)) == -1
    assert err() == "hrpt_denoise_host: color and colorOut must differ from input"
    assert call(im=images(colorOut=color.ctypes.data)) == 0
    wrong = view.copy(); wrong["m_ViewportSize"] = (w + 1, h)
    assert call(v=wrong) == -1
    assert b"m_ViewportSize" in native.lib.hrpt_last_error(None)
    assert err() == "hrpt_denoise_host: view->m_ViewportSize does not match the image size"
    assert call(ww=0) == -1 and call(hh=0) == -1 and call(ww=65536) == -1
    for ww, hh in ((0, h), (w, 0), (0, 0), (65536, h), (w, 65536)):       # reported before the view is compared with it
        assert call(ww=ww, hh=hh) == -1 and err() == "hrpt_denoise_host: size must be 1..65535", (ww, hh)
    bad = (float("nan"), float("inf"), -float("inf"))
    for field in ("radius", "phi", "lumaPhi", "depthPhi", "normalPhi", "roughnessPhi"):
        for value in bad + (-0.5,):
            assert call(p=S.DenoiseParams(**{field: value})) == -1, (field, value)
            assert err() == PARAMS, (field, value)
        assert call(p=S.DenoiseParams(**{field: 0.0})) == (-1 if field in ("radius", "phi") else 0), field
    assert call(p=S.DenoiseParams(iterations=0)) == -1 and call(p=S.DenoiseParams(iterations=6)) == -1
    assert err() == PARAMS
    assert call(p=S.DenoiseParams(iterations=2)) == -1        # one pass per call here; hrpt_denoise iterates
    assert b"iterations" in native.lib.hrpt_last_error(None)
    assert err() == "hrpt_denoise_host: one pass per call, iterations must be 1 (hrpt_denoise iterates)"
    assert call(p=S.DenoiseParams(radius=3e38, iterations=1)) == 0
    assert call(p=S.DenoiseParams(flags=2)) == -1 and call(p=S.DenoiseParams(flags=0x80000000)) == -1
    assert err() == PARAMS
    assert call(p=S.DenoiseParams(flags=S.DENOISE_OUTPUT_ONLY)) == 0
    assert call(p=S.DenoiseParams(reserved=1)) == -1
    assert err() == PARAMS
    assert call(p=S.DenoiseParams(frame=0xFFFFFFFF)) == 0
    # context calls on a NULL context
    p = S.DenoiseParams()
    assert native.lib.hrpt_denoise(None, view.ctypes.data, C.byref(p)) == -1
    assert native.lib.hrpt_denoise_device(None, C.byref(images()), w, h, view.ctypes.data, C.byref(p), None) == -1


# ---------------------------------------------------------------- 4. sanitizer build of the host side
@pytest.mark.parametrize("seed", [5, 6])
def test_host_side_is_clean_under_the_sanitizers(seed):
    """pt_denoise.h + the host executor + a driver with its own main, built with AddressSanitizer and UBSan (`make denoise_asan`), over
    random radii and frames and hostile values on exactly sized heap images. Nothing is loaded into Python."""
    subprocess.check_call(["make", "-C", CSRC, "denoise_asan"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(CSRC, "build", "denoise_asan"), str(seed)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "no report" in r.stdout
