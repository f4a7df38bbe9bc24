"""The upscale stage without a GPU (hrpt_upscale_host): the host executor of csrc/pt_upscale.h against the NumPy
restatement tests/upscale_reference.py, bit for bit on uint32 views with no pixel left out; the properties the stage promises, checked on
both; the argument errors; and the sanitizer build of the host side (`make upscale_asan`, a stand-alone program)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hobbyrenderer_amd import native, structs as S
import temporal_cases as TC
import upscale_cases as UC
import upscale_reference as R
from test_temporal_cpu import assert_same, u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hobbyrenderer_amd", "csrc")
SYMBOLS = ("hrpt_upscale_host", "hrpt_upscale_device", "hrpt_upscale", "hrpt_read_upscaled", "hrpt_get_upscaled_device",
           "hrpt_read_upscale_history", "hrpt_post_process_device")
SIZES = pytest.mark.parametrize("pair", UC.SIZE_PAIRS, ids=UC.pair_id)
MOTIONS = pytest.mark.parametrize("name", UC.MOTIONS)


def host(c, history, clamp=True, nthreads=3, **kw):
    return native.upscale_host(c["color"], c["depth"], c["motion"], history, c["display"], c["view"], c["prev"], UC.params(c, clamp, **kw), nthreads=nthreads)


def both(name, pair, jitter, with_history, clamp):
    """(library, reference) results of one case: each starts with the (colorOut, historyOut) pair."""
    c = UC.case(name, pair, jitter)
    return host(c, c["history"] if with_history else None, clamp), UC.reference(name, pair, jitter, with_history, clamp)


def test_symbols_are_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "hobbyrt_pt.h")).read()
    for name in SYMBOLS:
        assert name in native.EXPORTS and hasattr(native.lib, name) and f" {name}(" in header, name
    assert "#define HRPT_ABI_VERSION 3" in header and S.ABI_VERSION == 3
    assert C.sizeof(S.UpscaleParams) == 32 and C.sizeof(S.UpscaleImages) == 48
    p = S.UpscaleParams()
    assert list(p.jitter) == [0.0, 0.0] and p.kernel == np.float32(2.29) and p.maxHistory == 8.0 and p.flags == 0 and list(p.reserved) == [0, 0, 0]
    assert (S.UPSCALE_NO_CLAMP, S.UPSCALE_RESET) == (1, 2)
    assert (S.UpscaleParams.flags.offset, S.UpscaleImages.historyIn.offset) == (16, 24)      # that the C header says the same: test_binding_contract.py


# ---------------------------------------------------------------- 1. library == NumPy, bit for bit
@SIZES
@MOTIONS
def test_host_equals_reference(name, pair):
    for jitter in (False, True):
        for with_history in (False, True):
            for clamp in (True, False):
                lib, ref = both(name, pair, jitter, with_history, clamp)
                what = f"{name} {UC.pair_id(pair)} jitter={jitter} history={with_history} clamp={clamp}"
                assert_same(lib[0], ref[0], what + ": colorOut")
                assert_same(lib[1], ref[1], what + ": historyOut")


def test_the_cases_do_what_they_are_there_for():
    pair = UC.SIZE_PAIRS[2]
    (w, h), (W, H) = pair
    for jitter in (False, True):
        d = {name: UC.reference(name, pair, jitter, True, True)[2] for name in UC.MOTIONS}
        chosen = d["zero"]["tap"][0] >= 0
        assert 0 < (~chosen).sum() < chosen.sum()                               # all-miss neighbourhoods and hits
        assert (d["zero"]["blended"][chosen].all() if not jitter else d["zero"]["blended"].any()) and d["pan"]["blended"].any()
        assert not d["offscreen"]["blended"].any()
        assert 0 < d["random"]["blended"][chosen].sum() < chosen.sum()          # some reprojections leave the image, some do not
        ru, rv = d["random"]["reproj"]
        assert (ru * W < 1.5)[chosen].any() and (ru * W > W - 1.5)[chosen].any() and (rv * H < 1.5)[chosen].any() and (rv * H > H - 1.5)[chosen].any()
        c = UC.case("zero", pair, jitter)
        mi, mj = d["zero"]["tap"]
        centre_x = np.clip(np.floor((np.arange(W) + 0.5) * w / W - c["jitter"][0]), 0, w - 1)
        assert (mi[chosen] != np.broadcast_to(centre_x, (H, W))[chosen]).any()  # the nearest-depth tap is not always the centre one
    clamped, free = UC.reference("pan", pair, True, True, True), UC.reference("pan", pair, True, True, False)
    assert (u32(clamped[0]) != u32(free[0])).any()                              # the clamp bites (fireflies in the history)
    assert (UC.case("pan", pair, True)["history"][..., 3] > 8.0).any() and (clamped[1][..., 3] == 8.0).any()      # ... and so does maxHistory


@pytest.mark.parametrize("size", [((1, 1), (1, 1)), ((1, 1), (4, 4)), ((2, 3), (5, 3))], ids=UC.pair_id)
def test_tiny_images(size):
    for name in ("zero", "random"):
        for jitter in (False, True):
            for with_history in (False, True):
                lib, ref = both(name, size, jitter, with_history, True)
                assert_same(lib[0], ref[0], f"{name} {UC.pair_id(size)}: colorOut")
                assert_same(lib[1], ref[1], f"{name} {UC.pair_id(size)}: historyOut")


def test_three_chained_frames_ping_pong():
    pair = UC.SIZE_PAIRS[2]
    hist_lib = hist_ref = None
    for frame, (name, jitter) in enumerate([("zero", False), ("pan", True), ("random", True)]):
        c = UC.case(name, pair, jitter)
        lib = host(c, hist_lib)
        ref = R.upscale(c["color"], c["depth"], c["motion"], hist_ref, c["display"], c["view"], c["prev"], jitter=c["jitter"])
        assert_same(lib[0], ref[0], f"frame {frame}: colorOut")
        assert_same(lib[1], ref[1], f"frame {frame}: historyOut")
        hist_lib, hist_ref = lib[1], ref[1]
    assert hist_ref[..., 3].max() > 1.5                      # sample weight grew across the chain


def test_parameters_reach_the_arithmetic():
    """kernel and maxHistory other than the defaults, bit for bit; a kernel of 16 at 4x drives the far taps into the floor of the exponent."""
    for pair, kw in ((UC.SIZE_PAIRS[2], dict(kernel=0.5, maxHistory=2.5)), (((5, 4), (20, 16)), dict(kernel=16.0, maxHistory=0.0))):
        c = UC.case("pan", pair, True)
        lib = host(c, c["history"], **kw)
        ref = R.upscale(c["color"], c["depth"], c["motion"], c["history"], c["display"], c["view"], c["prev"], jitter=c["jitter"], kernel=kw["kernel"],
                        max_history=kw["maxHistory"], details=True)
        assert_same(lib[0], ref[0], f"{kw}: colorOut")
        assert_same(lib[1], ref[1], f"{kw}: historyOut")
        assert (ref[2]["beta"] > 0).all() and np.isfinite(ref[0]).all()


# ---------------------------------------------------------------- 2. properties, on the reference and on the library
def test_constant_image_with_equal_history_stays_constant():
    """Nine products and sums plus one lerp, each rounded to 2^-24: 2e-6 relative covers them."""
    pair = UC.SIZE_PAIRS[2]
    (w, h), (W, H) = pair
    value = np.array([0.7, 1.3, 0.2, 1.0], np.float32)
    for name in ("zero", "pan"):
        c = dict(UC.case(name, pair, True))
        c["color"] = np.broadcast_to(value, (h, w, 4)).copy()
        hist = np.broadcast_to(np.array([0.7, 1.3, 0.2, 5.0], np.float32), (H, W, 4)).copy()
        ref = R.upscale(c["color"], c["depth"], c["motion"], hist, c["display"], c["view"], c["prev"], jitter=c["jitter"])
        for col, history in (host(c, hist), ref[:2]):
            np.testing.assert_allclose(col[..., :3], np.broadcast_to(value[:3], (H, W, 3)), rtol=2e-6, atol=0)
            np.testing.assert_allclose(history[..., :3], np.broadcast_to(value[:3], (H, W, 3)), rtol=2e-6, atol=0)


@SIZES
def test_no_history_or_offscreen_gives_the_current_frame(pair):
    for jitter in (False, True):
        for name, with_history in (("random", False), ("offscreen", True)):
            for clamp in (True, False):
                lib, ref = both(name, pair, jitter, with_history, clamp)
                d = ref[2]
                chosen = d["tap"][0] >= 0
                assert not d["blended"].any()
                for col, hist in (lib[:2], ref[:2]):
                    assert np.array_equal(u32(col[..., :3]), u32(d["cur"])) and np.array_equal(u32(hist[..., :3]), u32(d["cur"]))
                    assert np.array_equal(u32(hist[..., 3][chosen]), u32(d["beta"][chosen]))


@SIZES
@MOTIONS
def test_clamp_and_weight_bounds(name, pair):
    for jitter in (False, True):
        for with_history in (False, True):
            lib, ref = both(name, pair, jitter, with_history, True)
            d = ref[2]
            assert (d["beta"] > 0).all() and (d["beta"] <= 1).all()
            lo, hi = np.nextafter(d["lo"], np.float32(-np.inf)), np.nextafter(d["hi"], np.float32(np.inf))
            for col, hist in (lib[:2], ref[:2]):
                assert ((col[..., :3] >= lo) & (col[..., :3] <= hi)).all()
                assert (hist[..., 3] <= 8.0).all() and (hist[..., 3] >= 0).all()


@SIZES
def test_all_miss_neighbourhood_passes_through(pair):
    c = UC.case("random", pair, True)
    lib, ref = both("random", pair, True, True, True)
    d = ref[2]
    none = d["tap"][0] < 0
    if c["hit"].all():
        assert not none.any()                                # 1 x 5: too small for the border of misses
        return
    assert none.sum() > 4
    for col, hist in (lib[:2], ref[:2]):
        assert np.array_equal(u32(col[none][:, :3]), u32(d["cur"][none])) and np.array_equal(u32(hist[none][:, :3]), u32(d["cur"][none]))
        assert not u32(hist[none][:, 3]).any()               # n' = +0


def test_alpha_is_the_nearest_texels():
    pair = UC.SIZE_PAIRS[1]
    (w, h), (W, H) = pair
    for jitter in (False, True):
        c = UC.case("pan", pair, jitter)
        lib, ref = both("pan", pair, jitter, True, True)
        bi = np.clip(np.floor((np.arange(W) + 0.5) * 0.5 - c["jitter"][0]), 0, w - 1).astype(int)
        bj = np.clip(np.floor((np.arange(H) + 0.5) * 0.5 - c["jitter"][1]), 0, h - 1).astype(int)
        want = c["color"][bj[:, None], bi[None, :], 3]
        assert np.array_equal(u32(lib[0][..., 3]), u32(want)) and np.array_equal(u32(ref[0][..., 3]), u32(want))


# ---- convergence at 2x: sixteen frames whose samples cycle over the four display pixels of every render texel
def mse(a, b):
    return float(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2))


def converge(run, pattern, clamp, pan):
    """Sixteen frames of `pattern` at 32 x 18 -> 64 x 36 through `run` ("library" or "reference"); pan: display pixels the content moves per
    frame. Returns (mse of the last colorOut, mse of the bilinear upsample of the last frame), both against the last frame's truth."""
    (w, h), (W, H) = (32, 18), (64, 36)
    view, prev = TC.views(w, h, False)
    depth = np.zeros((h, w, 4), np.float32); depth[..., 0] = 5.05; depth[..., 1] = 5.0
    motion = np.zeros((h, w, 4), np.float32); motion[..., 0] = -pan / 2.0; motion[..., 3] = 1.0        # this -> last frame, in render pixels
    hist = None
    for k in range(16):
        jitter = UC.CYCLE[k % 4]
        t = UC.truth(pattern, W, H, shift=pan * k)
        frame = UC.frame_of(t, jitter)
        if run == "library":
            col, hist = native.upscale_host(frame, depth, motion, hist, (W, H), view, prev, S.UpscaleParams(jitter=jitter, flags=0 if clamp else S.UPSCALE_NO_CLAMP))
        else:
            col, hist = R.upscale(frame, depth, motion, hist, (W, H), view, prev, jitter=jitter, clamp=clamp)
    return mse(col, t), mse(R.bilinear_upsample(frame, (W, H)), t)


CONVERGENCE = [("checkerboard", UC.checkerboard, False), ("sinusoid", UC.sinusoid, True)]


@pytest.mark.parametrize("pan", [0, 4], ids=["static", "pan"])
@pytest.mark.parametrize("label,pattern,clamp", CONVERGENCE, ids=[c[0] for c in CONVERGENCE])
def test_sixteen_jittered_frames_beat_the_bilinear_upsample(label, pattern, clamp, pan):
    """At 2x with jitter (+-0.25, +-0.25) every sample lies on a display pixel centre, and each display pixel is sampled exactly once in
    four frames. (a) a one-pixel checkerboard without the clamp, (b) a sinusoid of period 6 display pixels with it; static, and under a
    uniform pan of 2 render pixels per frame with exact motion vectors. The resolved image must be below HALF the mean squared error of
    the bilinear upsample of the last single frame. Measured ratios (both executors give the same to the digits shown) are in DESIGN.md
    section 24."""
    for run in ("reference", "library"):
        got, bilinear = converge(run, pattern, clamp, pan)
        print(f"{label} pan={pan} {run}: mse {got:.5f}, bilinear {bilinear:.5f}, ratio {got / bilinear:.4f}")
        assert got < 0.5 * bilinear, (run, got, bilinear)


# ---------------------------------------------------------------- 3. housekeeping
def test_thread_count_invariance():
    c = UC.case("random", UC.SIZE_PAIRS[2], True)
    one = host(c, c["history"], nthreads=1)
    for n in (2, 3, 7, 0, -1, 1000):
        got = host(c, c["history"], nthreads=n)
        assert np.array_equal(u32(got[0]), u32(one[0])) and np.array_equal(u32(got[1]), u32(one[1])), n


def test_argument_errors():
    pair = UC.SIZE_PAIRS[2]
    (w, h), (W, H) = pair
    c = UC.case("zero", pair, False)
    imgs = [np.ascontiguousarray(c[k], np.float32).copy() for k in ("color", "depth", "motion", "history")]
    hout, cout = np.full((H, W, 4), 7.0, np.float32), np.full((H, W, 4), 7.0, np.float32)
    view, prev = c["view"], c["prev"]

    def call(im=None, ww=w, hh=h, WW=W, HH=H, v=view, pv=prev, p=None):
        im = im if im is not None else S.UpscaleImages(*[a.ctypes.data for a in imgs], hout.ctypes.data, cout.ctypes.data)
        p = p if p is not None else S.UpscaleParams()
        return native.lib.hrpt_upscale_host(C.byref(im) if im != "null" else None, ww, hh, WW, HH, v.ctypes.data if v is not None else None,
                                            pv.ctypes.data if pv is not None else None, C.byref(p) if p != "null" else None, 1)
    err = lambda: native.lib.hrpt_last_error(None).decode()          # noqa: E731
    PARAMS = ("hrpt_upscale_host: jitter must be finite and in [-0.5, 0.5], kernel finite and in (0, 16], maxHistory finite and >= 0, "
              "flags HRPT_UPSCALE_* only, reserved 0")
    for kw in (dict(im="null"), dict(v=None), dict(pv=None), dict(p="null")):
        assert call(**kw) == -1 and err() == "hrpt_upscale_host: null argument", kw
    for k in range(6):
        if k == 3:
            continue                                         # historyIn may be NULL
        ptrs = [a.ctypes.data for a in imgs] + [hout.ctypes.data, cout.ctypes.data]
        ptrs[k] = None
        assert call(im=S.UpscaleImages(*ptrs)) == -1 and err() == "hrpt_upscale_host: null image (only historyIn may be NULL)", k
    base = [a.ctypes.data for a in imgs]
    assert call(im=S.UpscaleImages(*base, imgs[3].ctypes.data, cout.ctypes.data)) == -1 and err() == "hrpt_upscale_host: historyOut must differ from historyIn"
    for alias in (imgs[3], hout):
        assert call(im=S.UpscaleImages(*base, hout.ctypes.data, alias.ctypes.data)) == -1
        assert err() == "hrpt_upscale_host: colorOut must differ from historyIn and historyOut"
    for kw in (dict(ww=0), dict(hh=0), dict(WW=0), dict(HH=0), dict(ww=65536), dict(HH=65536)):       # reported before ratio and view
        assert call(**kw) == -1 and err() == "hrpt_upscale_host: size must be 1..65535", kw
    for kw in (dict(WW=w - 1), dict(HH=h - 1), dict(WW=4 * w + 1), dict(HH=4 * h + 1)):
        assert call(**kw) == -1 and err() == "hrpt_upscale_host: the display size must lie between the render size and four times it, per axis", kw
    wrong = view.copy(); wrong["m_ViewportSize"] = (W, H)     # the display size is not the view's
    assert call(v=wrong) == -1 and err() == "hrpt_upscale_host: view->m_ViewportSize does not match the image size"
    nan, inf = float("nan"), float("inf")
    bad = [dict(jitter=(0.51, 0.0)), dict(jitter=(0.0, -0.51)), dict(jitter=(nan, 0.0)), dict(jitter=(0.0, inf)), dict(kernel=0.0), dict(kernel=-1.0),
           dict(kernel=16.5), dict(kernel=nan), dict(kernel=inf), dict(maxHistory=-0.5), dict(maxHistory=nan), dict(maxHistory=inf), dict(flags=4),
           dict(flags=0x80000000)]
    for kw in bad:
        assert call(p=S.UpscaleParams(**kw)) == -1 and err() == PARAMS, kw
    for k in range(3):
        p = S.UpscaleParams(); p.reserved[k] = 1
        assert call(p=p) == -1 and err() == PARAMS, k
    assert (hout == 7.0).all() and (cout == 7.0).all()        # bad input changes nothing
    for kw in (dict(jitter=(0.5, -0.5)), dict(kernel=16.0), dict(maxHistory=0.0), dict(flags=S.UPSCALE_NO_CLAMP | S.UPSCALE_RESET)):
        assert call(p=S.UpscaleParams(**kw)) == 0, kw
    assert call(im=S.UpscaleImages(*base[:3], None, hout.ctypes.data, cout.ctypes.data)) == 0
    # context calls on a NULL context
    p = S.UpscaleParams()
    assert native.lib.hrpt_upscale(None, W, H, view.ctypes.data, prev.ctypes.data, C.byref(p)) == -1
    assert native.lib.hrpt_upscale_device(None, None, w, h, W, H, view.ctypes.data, prev.ctypes.data, C.byref(p), None) == -1
    assert native.lib.hrpt_read_upscaled(None, hout.ctypes.data, hout.nbytes) == -1
    assert native.lib.hrpt_read_upscale_history(None, hout.ctypes.data, hout.nbytes) == -1
    assert native.lib.hrpt_get_upscaled_device(None, None) == -1
    assert native.lib.hrpt_post_process_device(None, None, None, 0, None, None) == -1


def test_ratio_limits_are_inclusive():
    for pair in (((3, 2), (12, 8)), ((3, 2), (3, 2)), ((3, 2), (12, 2))):
        lib, ref = both("zero", pair, True, True, True)
        assert_same(lib[0], ref[0], UC.pair_id(pair))


def test_staged_window_holds_every_tap():
    """What upscale_resolve_staged relies on (csrc/pt_upscale.hip): along an axis the base texel never decreases, and every tap of a tile
    of 32 (8) display pixels lies within 36 (12) texels of the tile's first base texel minus one. Checked in float32, as the kernel
    computes it, over 593 size pairs at ratios from 1 to 4 and jitters at, inside and next to the limits."""
    rng = np.random.default_rng(1)
    sizes = [(w, W) for w in list(range(1, 70)) + [959, 960, 1280, 1920, 16383, 65535 // 4, 65535]
             for W in sorted({w, w + 1, 2 * w - 1, 2 * w, 3 * w, 4 * w - 1, 4 * w, int(w * 1.5) + 1}) if w <= W <= 4 * w and W <= 65535]
    assert len(sizes) == 593
    widest = 0
    for w, W in sizes:
        for j in (-0.5, 0.5, 0.0, 0.3125, -0.4375, 0.49999997, -0.49999997, float(rng.uniform(-0.5, 0.5))):
            _, b = R._base(W, w, np.float32(j))
            assert (np.diff(b) >= 0).all()
            for tile, window in ((32, 36), (8, 12)):
                origin = b[(np.arange(W) // tile) * tile] - 1
                for d in (-1, 0, 1):
                    local = np.clip(b + d, 0, w - 1) - origin
                    assert local.min() >= 0 and local.max() < window, (w, W, j, tile)
                    widest = max(widest, int(local.max()))
    assert widest == 33                                      # 34 of the 35 texels the argument allows for are reached, at 1x


# ---------------------------------------------------------------- 4. sanitizer build of the host side
@pytest.mark.parametrize("seed", [5, 6])
def test_host_side_is_clean_under_the_sanitizers(seed):
    """pt_upscale.h + the host executor + a driver with its own main, built with AddressSanitizer and UBSan (`make upscale_asan`), over
    random motion fields and hostile values on exactly sized heap images at every scale ratio. Nothing is loaded into Python."""
    subprocess.check_call(["make", "-C", CSRC, "upscale_asan"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(CSRC, "build", "upscale_asan"), str(seed)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "no report" in r.stdout
