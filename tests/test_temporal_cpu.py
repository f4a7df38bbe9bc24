"""The temporal stage without a GPU (hrpt_temporal_host): the host executor of csrc/pt_temporal.h against the NumPy
restatement tests/temporal_reference.py, bit for bit on uint32 views with no pixel left out; the properties the stage promises, checked on
both; the argument errors; and the sanitizer build of the host side (`make temporal_asan`, a stand-alone program)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hobbyrenderer_amd import native, structs as S
import temporal_cases as TC
import temporal_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hobbyrenderer_amd", "csrc")
SYMBOLS = ("hrpt_temporal_host", "hrpt_temporal_device", "hrpt_temporal_accumulate", "hrpt_read_temporal_history",
           "hrpt_get_temporal_history_device", "hrpt_clear_accumulation")


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what):
    a, b = u32(got), u32(want)
    bad = (a != b).any(-1)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (x={x}, y={y}): {got[y, x]} != {want[y, x]}")


def both(c, history, linear, blend=None):
    """(library, reference) results of one call: each a (colorOut, historyOut) pair."""
    blend = c["blend"] if blend is None else blend
    lib = native.temporal_host(c["color"], c["motion"], c["depth"], c["normal"], history, c["view"], c["prev"], TC.params(blend, linear), nthreads=3)
    ref = R.temporal(c["color"], c["motion"], c["depth"], c["normal"], history, c["view"], c["prev"], blend=blend, linear=linear)
    return lib, ref


def test_symbols_are_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "hobbyrt_pt.h")).read()
    for name in SYMBOLS:
        assert name in native.EXPORTS and hasattr(native.lib, name) and f" {name}(" in header, name
    assert "#define HRPT_ABI_VERSION 3" in header and S.ABI_VERSION == 3
    assert C.sizeof(S.TemporalParams) == 16 and C.sizeof(S.TemporalImages) == 56
    p = S.TemporalParams()
    assert p.blend == np.float32(0.9) and p.flags == 0 and list(p.reserved) == [0, 0]
    assert (S.TEMPORAL_LINEAR, S.TEMPORAL_RESET) == (1, 2)


# ---------------------------------------------------------------- 1. library == NumPy, bit for bit
@pytest.mark.parametrize("size", TC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", TC.MOTIONS)
def test_host_equals_reference(name, size):
    w, h = size
    for jitter in (False, True):
        c = TC.case(name, w, h, jitter)
        for linear in (False, True):
            for hist in (None, c["history"]):
                lib, ref = both(c, hist, linear)
                what = f"{name} {w}x{h} jitter={jitter} linear={linear} history={hist is not None}"
                assert_same(lib[0], ref[0], what + ": colorOut")
                assert_same(lib[1], ref[1], what + ": historyOut")
        if name == "zero" and not jitter:
            continue
        # the case does what it is there for
        _, _, d = R.temporal(c["color"], c["motion"], c["depth"], c["normal"], c["history"], c["view"], c["prev"], blend=c["blend"], linear=True, details=True)
        hit = c["hit"]
        if name == "random":
            nu, nv = d["nojitter"]
            assert ((nu < 0) | (nu > 1) | (nv < 0) | (nv > 1))[hit].any() and (d["confidence"][hit] > 0).any()
            ru, rv = d["reproj"]
            assert (ru * w < 1.5)[hit].any() and (ru * w > w - 1.5)[hit].any() and (rv * h < 1.5)[hit].any() and (rv * h > h - 1.5)[hit].any()
        if name in ("integer", "capped"):          # the cap bites: pixels whose mix is the cap, not accumBlend
            cap = np.float32(1.0) + d["move"] * (np.float32(c["blend"]) - np.float32(1.0))
            assert ((d["mix"] == cap) & (d["confidence"] > 0.5) & hit).any() and ((d["mix"] < cap) & (d["mix"] > 0) & hit).any()
        if name == "capped":
            assert ((d["move"] > 0) & (d["move"] < 1))[hit].all()


def test_three_chained_frames_ping_pong():
    w, h = 37, 23
    for linear in (False, True):
        hist_lib = hist_ref = None
        for frame, name in enumerate(["zero", "subpixel", "random"]):
            c = TC.case(name, w, h, jitter=frame == 1)
            c["color"] = TC.radiance(w, h, 30 + frame)
            lib = native.temporal_host(c["color"], c["motion"], c["depth"], c["normal"], hist_lib, c["view"], c["prev"], TC.params(0.9, linear))
            ref = R.temporal(c["color"], c["motion"], c["depth"], c["normal"], hist_ref, c["view"], c["prev"], linear=linear)
            assert_same(lib[0], ref[0], f"frame {frame} linear={linear}: colorOut")
            assert_same(lib[1], ref[1], f"frame {frame} linear={linear}: historyOut")
            hist_lib, hist_ref = lib[1], ref[1]
        assert hist_ref[..., 3].max() > 1.5                  # ages grew across the chain


@pytest.mark.parametrize("size", [(1, 1), (2, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiny_images(size):
    w, h = size
    for name in ("zero", "subpixel", "random"):
        c = TC.case(name, w, h, jitter=True)
        assert c["hit"].all()
        for linear in (False, True):
            for hist in (None, c["history"]):
                lib, ref = both(c, hist, linear)
                assert_same(lib[0], ref[0], f"{name} {w}x{h}: colorOut")
                assert_same(lib[1], ref[1], f"{name} {w}x{h}: historyOut")


def test_color_out_may_be_color():
    c = TC.case("subpixel", 37, 23, True)
    imgs = [np.ascontiguousarray(c[k], np.float32).copy() for k in ("color", "motion", "depth", "normal", "history")]
    hout = np.empty_like(imgs[0])
    im = S.TemporalImages(*[a.ctypes.data for a in imgs], hout.ctypes.data, imgs[0].ctypes.data)
    p = TC.params(0.9, True)
    assert native.lib.hrpt_temporal_host(C.byref(im), 37, 23, c["view"].ctypes.data, c["prev"].ctypes.data, C.byref(p), 2) == 0
    ref = R.temporal(c["color"], c["motion"], c["depth"], c["normal"], c["history"], c["view"], c["prev"], linear=True)
    assert_same(imgs[0], ref[0], "in place: colorOut")
    assert_same(hout, ref[1], "in place: historyOut")


# ---------------------------------------------------------------- 2. properties, on the reference and on the library
def test_no_history_passes_the_input_through():
    for name in ("zero", "random"):
        c = TC.case(name, 37, 23, True)
        for pair in both(c, None, True):
            col, hist = pair
            assert np.array_equal(u32(col[..., :3]), u32(c["color"][..., :3])) and np.array_equal(u32(hist[..., :3]), u32(c["color"][..., :3]))
            assert not u32(hist[..., 3]).any()               # age +0 everywhere
        # the reference's space sends the input through log(1 + x) and exp(x) - 1: the same value up to the two functions' rounding. The
        # inputs stay below 255, so y = log(1 + x) < 5.55 and ulp(y) <= 4.8e-7; x + 1, log2, * ln 2, exp and - 1 round once or twice each at
        # that size or below: under 8 ulp(y) = 3.8e-6 of absolute error in y = relative error of exp(y), and 1e-6 absolute near x = 0.
        for pair in both(c, None, False):
            col, hist = pair
            np.testing.assert_allclose(col[..., :3][c["hit"]], c["color"][..., :3][c["hit"]], rtol=4e-6, atol=1e-6)
            assert not u32(hist[..., 3]).any()


def test_miss_pixels_pass_through_and_alpha_is_kept():
    c = TC.case("random", 64, 36, True)
    c["color"][..., 3] = np.random.default_rng(3).random((36, 64)).astype(np.float32)
    miss = ~c["hit"]
    assert miss.sum() > 100
    for linear in (False, True):
        for pair in both(c, c["history"], linear):
            col, hist = pair
            assert np.array_equal(u32(col[miss]), u32(c["color"][miss]))
            assert np.array_equal(u32(hist[miss][:, :3]), u32(c["color"][miss][:, :3])) and not u32(hist[miss][:, 3]).any()
            assert np.array_equal(u32(col[..., 3]), u32(c["color"][..., 3]))          # alpha of colorOut is color's, hits and misses


def test_static_linear_sequence_is_the_running_mean():
    """16 independent frames, no motion, linear space: the mean of the 16 within rtol 1e-4, age 15 within 1e-3. The resampling of a static
    pixel is not exactly the identity: uv * W comes back as px + 0.5 give or take one ulp, so f is 0, ~2^-19 or 1 - 2^-19 and a texel
    takes up to f / 2 of the difference of its two neighbours per frame (section 17). With neighbours of the same order as the pixel, as
    here, that is ~1e-6 per frame and inside the bound; next to a texel 50 times brighter it is not, which is why this test's frames
    carry no fireflies (the bit-exact tests keep them)."""
    w, h = 37, 23
    c = TC.case("zero", w, h, False)
    frames = [TC.radiance(w, h, 100 + k, fireflies=False) for k in range(16)]
    mean = np.mean([f[..., :3].astype(np.float64) for f in frames], 0)
    interior = c["hit"].copy()
    interior[:1] = interior[-1:] = False; interior[:, :1] = interior[:, -1:] = False
    for run in ("library", "reference"):
        hist = None
        for k, f in enumerate(frames):
            if run == "library":
                col, hist = native.temporal_host(f, c["motion"], c["depth"], c["normal"], hist, c["view"], c["prev"], TC.params(0.9, True))
            else:
                col, hist = R.temporal(f, c["motion"], c["depth"], c["normal"], hist, c["view"], c["prev"], linear=True)
        np.testing.assert_allclose(col[..., :3][interior], mean[interior], rtol=1e-4, err_msg=run)
        np.testing.assert_allclose(hist[..., 3][interior], 15.0, rtol=1e-3, err_msg=run)


def test_depth_discontinuity_gives_confidence_zero():
    """Motion that carries far-plane pixels onto the near box (view depth 11 against 2): the reconstructed positions are ~9 units apart, the
    disocclusion saturates, confidence 0, the output is the input and the age 0."""
    w, h = 64, 36
    c = TC.case("zero", w, h, False)
    x0 = w // 3
    col_from = x0 - 3
    c["motion"][:, col_from, 0] = 4.0                        # lands on the box's first columns
    rows = np.arange(h // 3 + 1, (2 * h) // 3 - 1)
    assert c["hit"][rows, col_from].any()
    rows = rows[c["hit"][rows, col_from] & c["hit"][rows, col_from + 4]]
    _, _, d = R.temporal(c["color"], c["motion"], c["depth"], c["normal"], c["history"], c["view"], c["prev"], linear=True, details=True)
    assert len(rows) > 3 and not d["confidence"][rows, col_from].any()
    assert (d["confidence"][rows, col_from - 3] == 1).all()  # its static neighbours on the plane validate fully
    for pair in both(c, c["history"], True):
        col, hist = pair
        assert np.array_equal(u32(col[rows, col_from, :3]), u32(c["color"][rows, col_from, :3]))
        assert not u32(hist[rows, col_from, 3]).any()


# ---------------------------------------------------------------- 3. argument errors
def test_argument_errors():
    w, h = 37, 23
    c = TC.case("zero", w, h, False)
    imgs = [np.ascontiguousarray(c[k], np.float32) for k in ("color", "motion", "depth", "normal", "history")]
    hout, cout = np.empty_like(imgs[0]), np.empty_like(imgs[0])
    view, prev = c["view"], c["prev"]

    def call(im=None, ww=w, hh=h, v=view, pv=prev, p=None):
        im = im if im is not None else S.TemporalImages(*[a.ctypes.data for a in imgs], hout.ctypes.data, cout.ctypes.data)
        p = p if p is not None else S.TemporalParams()
        return native.lib.hrpt_temporal_host(C.byref(im) if im != "null" else None, ww, hh, v.ctypes.data if v is not None else None,
                                             pv.ctypes.data if pv is not None else None, C.byref(p) if p != "null" else None, 1)
    err = lambda: native.lib.hrpt_last_error(None).decode()          # noqa: E731 -- the whole text, as the library has always worded it
    PARAMS = "hrpt_temporal_host: blend must be finite and in [0, 1], flags HRPT_TEMPORAL_* only, reserved 0"
    assert call() == 0
    assert call(im="null") == -1 and call(v=None) == -1 and call(pv=None) == -1 and call(p="null") == -1
    for kw in (dict(im="null"), dict(v=None), dict(pv=None), dict(p="null")):
        assert call(**kw) == -1 and err() == "hrpt_temporal_host: null argument", kw
    for k in range(7):
        if k == 4:
            continue                                         # historyIn may be NULL
        ptrs = [a.ctypes.data for a in imgs] + [hout.ctypes.data, cout.ctypes.data]
        ptrs[k] = None
        assert call(im=S.TemporalImages(*ptrs)) == -1, k
        assert err() == "hrpt_temporal_host: null image (only historyIn may be NULL)", k
    ptrs = [a.ctypes.data for a in imgs] + [imgs[4].ctypes.data, cout.ctypes.data]
    assert call(im=S.TemporalImages(*ptrs)) == -1            # historyOut == historyIn
    assert b"historyOut" in native.lib.hrpt_last_error(None)
    assert err() == "hrpt_temporal_host: historyOut must differ from historyIn"
    wrong = view.copy(); wrong["m_ViewportSize"] = (w + 1, h)
    assert call(v=wrong) == -1
    assert b"m_ViewportSize" in native.lib.hrpt_last_error(None)
    assert err() == "hrpt_temporal_host: view->m_ViewportSize does not match the image size"
    assert call(ww=0) == -1 and call(hh=0) == -1 and call(ww=65536) == -1
    for ww, hh in ((0, h), (w, 0), (0, 0), (65536, h), (w, 65536)):       # reported before the view is compared with it
        assert call(ww=ww, hh=hh) == -1 and err() == "hrpt_temporal_host: size must be 1..65535", (ww, hh)
    for blend in (-0.01, 1.01, float("nan"), float("inf"), -float("inf")):
        assert call(p=S.TemporalParams(blend)) == -1, blend
        assert err() == PARAMS, blend
    for blend in (0.0, 1.0):
        assert call(p=S.TemporalParams(blend)) == 0
    assert call(p=S.TemporalParams(0.9, 4)) == -1 and call(p=S.TemporalParams(0.9, 0x80000000)) == -1
    assert err() == PARAMS
    assert call(p=S.TemporalParams(0.9, S.TEMPORAL_LINEAR | S.TEMPORAL_RESET)) == 0
    p = S.TemporalParams(); p.reserved[1] = 1
    assert call(p=p) == -1
    assert err() == PARAMS
    # context calls on a NULL context
    assert native.lib.hrpt_temporal_accumulate(None, view.ctypes.data, prev.ctypes.data, C.byref(S.TemporalParams())) == -1
    assert native.lib.hrpt_clear_accumulation(None) == -1
    assert native.lib.hrpt_read_temporal_history(None, hout.ctypes.data, hout.nbytes) == -1
    assert native.lib.hrpt_get_temporal_history_device(None, None) == -1


def test_nthreads_is_clamped():
    """nthreads <= 0 means one per hardware thread up to 16, and no more than 256 (nor than rows) are started: the image is that of one."""
    c = TC.case("random", 37, 23, True)
    one = native.temporal_host(c["color"], c["motion"], c["depth"], c["normal"], c["history"], c["view"], c["prev"], TC.params(0.9, False), nthreads=1)
    for n in (0, -1, 1000):
        got = native.temporal_host(c["color"], c["motion"], c["depth"], c["normal"], c["history"], c["view"], c["prev"], TC.params(0.9, False), nthreads=n)
        assert np.array_equal(u32(got[0]), u32(one[0])) and np.array_equal(u32(got[1]), u32(one[1])), n


# ---------------------------------------------------------------- 4. sanitizer build of the host side
@pytest.mark.parametrize("seed", [5, 6])
def test_host_side_is_clean_under_the_sanitizers(seed):
    """pt_temporal.h + the host executor + a driver with its own main, built with AddressSanitizer and UBSan (`make temporal_asan`), over
    random motion fields of +-4 px and hostile values on exactly sized heap images. Nothing is loaded into Python."""
    subprocess.check_call(["make", "-C", CSRC, "temporal_asan"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(CSRC, "build", "temporal_asan"), str(seed)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "no report" in r.stdout
