"""The CPU oracle's post chain (or_post_process) held to the float64 statement of tests/post_reference.py on the cases of
tests/post_cases.py, in SDR and in HDR at 600 and 1000 nits; before that, the statement itself held to answers derivable by hand.

The bounds (post_reference.SDR_ABS, HDR_ABS, HDR_REL, EXPOSURE_REL, BAND) were fixed from what this file measures; the measuring tests print
their figures (-s shows them). tests/test_post_reference_gpu.py holds the device to the same constants through `check_against_statement`."""
import functools
import math

import numpy as np
import pytest

from oracle.binding import post_process
import post_cases as PC
import post_reference as R

f32, f64 = np.float32, np.float64
MODES = list(PC.MODES)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def ebits(e):
    return int(f32(e).view(np.uint32))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(None)
def oracle_single(name, mode):
    """One pass of the oracle over a single-frame case from exposure 1: dict(img, params, e_in, disp, e, hist). Computed once, read-only."""
    make, kw = PC.SINGLE[name]
    img, p = make(), PC.params(mode, **kw)
    disp, e, hist = post_process(img, p, 1.0)
    _frozen(disp, hist)
    return dict(img=img, params=p, e_in=f32(1.0), disp=disp, e=f32(e), hist=hist)


@functools.lru_cache(None)
def oracle_sequence(name, mode):
    """The oracle over the frames of a sequence with one exposure carried along: a tuple of the dicts above."""
    frames, kw = PC.SEQUENCES[name]
    p, e, out = PC.params(mode, **kw), f32(1.0), []
    for img in frames():
        disp, e2, hist = post_process(img, p, float(e))
        _frozen(disp, hist)
        out.append(dict(img=img, params=p, e_in=e, disp=disp, e=f32(e2), hist=hist))
        e = f32(e2)
    return tuple(out)


@functools.lru_cache(None)
def bounds_of(name):
    make = PC.SINGLE[name][0]
    return _frozen(*R.histogram_bounds(make()))


def errors(run, disp, e, hist):
    """The distances of one pass's results (float32 display, float32 exposure, histogram) from the statement. The exposure is compared with
    adapt() of the histogram that came with it and the display with tonemap() at the exposure that came with it, so no error is counted twice."""
    img, p = run["img"], run["params"]
    n = img.shape[0] * img.shape[1]
    e_ref = R.adapt(hist, n, p, run["e_in"])
    # relative to the larger of the old and the new exposure: the update is a float32 lerp, current + (target - current) * weight, whose
    # roundings are in units of its larger operand (from 6.9 down to 0.0028 in one step, half an ulp of 6.9 is 1e-4 of the result)
    out = dict(exposure_rel=abs(float(e) - e_ref) / max(abs(e_ref), abs(float(run["e_in"]))), sdr_abs=0.0, hdr_abs=0.0, hdr_rel=0.0)
    mask = R.tonemap_domain(img, e)
    ref = R.tonemap(img, e, p)[mask][:, :3]
    err = np.abs(np.asarray(disp, f64)[mask][:, :3] - ref)
    if p.hdrDisplay:
        low = np.abs(ref) <= 1.0
        out["hdr_abs"] = float(err[low].max(initial=0.0))
        out["hdr_rel"] = float((err[~low] / np.abs(ref[~low])).max(initial=0.0))
        out["display_excess"] = float((err - (R.HDR_ABS + R.HDR_REL * np.abs(ref))).max(initial=-1.0))
    else:
        out["sdr_abs"] = float(err.max(initial=0.0))
        out["display_excess"] = out["sdr_abs"] - R.SDR_ABS
    return out


def check_histogram(run, hist, sure, maybe, what):
    img, p = run["img"], run["params"]
    hist = np.asarray(hist, np.int64)
    if not p.autoExposure:
        assert not hist.any(), f"{what}: manual exposure leaves the histogram zero"
        return
    assert hist.sum() == img.shape[0] * img.shape[1], f"{what}: the histogram counts every pixel once"
    bad = np.flatnonzero((hist < sure) | (hist > sure + maybe))
    assert bad.size == 0, f"{what}: bins {bad[:8]} hold {hist[bad[:8]]}, legal {sure[bad[:8]]} ... {(sure + maybe)[bad[:8]]}"


def check_against_statement(run, disp, e, hist, sure, maybe, what):
    """What the oracle and the device are both held to. Returns the measured distances."""
    check_histogram(run, hist, sure, maybe, what)
    disp = np.asarray(disp)
    assert (disp[..., 3] == 1.0).all(), f"{what}: display alpha is 1"
    if not run["params"].autoExposure:
        assert ebits(e) == ebits(run["params"].manualExposure), f"{what}: manual exposure is copied as bits"
    m = errors(run, disp, e, hist)
    print(f"{what}: " + " ".join(f"{k}={v:.3e}" for k, v in m.items()))
    assert m["exposure_rel"] <= R.EXPOSURE_REL, f"{what}: exposure is {m['exposure_rel']:.3e} (relative to the larger of old and new) from the statement"
    assert m["display_excess"] <= 0.0, f"{what}: display exceeds its bound by {m['display_excess']:.3e} (sdr_abs {m['sdr_abs']:.3e}, hdr_abs {m['hdr_abs']:.3e}, hdr_rel {m['hdr_rel']:.3e})"
    return m


# ---------------------------------------------------------------- 1. the statement's known answers
def _grey(v):
    img = np.ones((1, np.size(v), 4), f32)
    img[0, :, :3] = np.asarray(v, f32).reshape(-1, 1)
    return img


def test_statement_sdr_toe_and_shoulder():
    x = np.array([1e-4, 0.001, 0.005, 0.01, 0.02, 0.0223], f32)           # 6.25 x^2 <= 0.0031308 up to x = 0.02238
    got = R.tonemap(_grey(x), 1.0, PC.params("sdr"))[0]
    xs = x.astype(f64)
    assert np.allclose(got[:, :3], (12.92 * 6.25 * xs * xs)[:, None], rtol=1e-11, atol=0) and (got[:, 3] == 1).all()
    big = R.tonemap(_grey([1e3, 1e6, 1e12]), 1.0, PC.params("sdr"))[0, :, 0]
    assert (np.diff(big) > 0).all() and big[-1] <= 1.0 and 1.0 - big[-1] < 1e-11                # peak -> infinity: display -> 1
    mid = R.tonemap(_grey([0.5]), 1.0, PC.params("sdr"))[0, 0, 0]                                # 0.08 <= x, peak 0.46 < 0.76: sRGB of x - 0.04
    assert abs(mid - (1.055 * 0.46 ** (1 / 2.4) - 0.055)) < 1e-15
    assert R.tonemap(_grey([0.5]), 0.5, PC.params("sdr"))[0, 0, 0] == R.tonemap(_grey([0.25]), 1.0, PC.params("sdr"))[0, 0, 0]


def test_statement_hdr_passthrough_and_limit():
    img = np.ones((1, 3, 4), f32)
    img[0, :, :3] = [[0.25, 1.0, 0.5], [1.0, 1.0, 1.0], [0.0, 0.3, 0.9]]
    for mode, top in (("hdr600", 7.5), ("hdr1000", 12.5)):
        got = R.tonemap(img, 1.0, PC.params(mode))
        assert np.array_equal(got[..., :3], img[..., :3].astype(f64))                            # lum <= 1 passes unchanged, 1 included
        far = R.tonemap(_grey([2.0, 1e3, 1e9, 1e30]), 1.0, PC.params(mode))[0, :, 0]
        assert (np.diff(far) > 0).all() and far[-1] <= top and top - far[-1] < 1e-12
        assert abs(far[0] - (1 + (top - 1) / top)) < 1e-15                                       # lum 2: 1 + h / (1 + h)


def test_statement_bins():
    k = np.arange(1, 255)
    lum = R.bin_centre(k)
    img = np.ones((1, 254, 4), f32)
    img[0, :, :3] = (lum / PC.WEIGHTS.sum())[:, None]
    assert np.array_equal(R.bins(img), k)                                                        # bin centres land in their bins
    pos, below = R.bin_position(img)
    assert np.abs(pos - (k + 0.5)).max() < 1e-4 and not below.any()
    nan, inf, fmax = f32(np.nan), f32(np.inf), np.finfo(f32).max
    px = [[nan, 1, 1], [nan, nan, nan], [inf, 1, 1], [fmax, fmax, fmax], [2.0 ** 21] * 3, [-inf, 1, 1], [1, -3, 1], [0, 0, 0],
          [-0.0] * 3, [1e-39] * 3, [0.00009] * 3, [0.0002] * 3, [0.00098] * 3, [0.0011] * 3]
    img = np.ones((1, len(px), 4), f32)
    img[0, :, :3] = px
    assert R.bins(img).tolist() == [1, 1, 255, 255, 255, 0, 0, 0, 0, 0, 0, 1, 1, 2]


def test_statement_adaptation_closed_form():
    for k in (0, 1, 2, 100, 200, 255):
        hist = np.zeros(256, np.int64); hist[k] = 1000
        value = -10.0 if k == 0 else -10.0 + 30.0 * (k - 1) / 254.0
        assert abs(float(R.bin_value(k)) - value) < 1e-14
        p = PC.params("sdr", dt=0.1, speed=5.0)
        target = 1.0 / (2.0 ** min(max(value + 3.0, -7.0), 23.0) * 1.2)                          # avg = value; EV100 = value + log2(8)
        want = 1.0 + (target - 1.0) * (1.0 - math.exp(-float(f32(0.1)) * 5.0))
        assert abs(R.adapt(hist, 1000, p, 1.0) - want) <= 1e-14 * want       # dt arrives as float32: 0.1f * 5 is not 0.5
        assert R.adapt(hist, 1000, PC.params("sdr", dt=0.0), 0.625) == 0.625
        assert R.adapt(hist, 1000, PC.params("sdr", auto=0, manual=0.37), 1.0) == float(f32(0.37))
    hist = np.zeros(256, np.int64); hist[100] = 7
    p = PC.params("sdr", dt=10.0, speed=5.0, comp=2.0, evmin=3.0, evmax=3.0)
    assert abs(R.adapt(hist, 7, p, 1.0) - 1.0 / (2.0 * 1.2)) < 1e-15                              # EV100 = 3 - 2; 1 - exp(-50) = 1


def test_statement_histogram_bounds():
    sure, maybe, exact = R.histogram_bounds(PC.ladder())
    assert not maybe.any() and np.array_equal(sure, exact)
    want = np.zeros(256, np.int64)
    want[1:255] = 1 + np.arange(1, 255) % 7
    want[1] += 2; want[255] = 3; want[0] = 5
    assert np.array_equal(exact, want)
    edge = np.ones((1, 3, 4), f32)
    edge[0, 0, :3] = f32(2.0 ** (-10 + 30 * (112 - 1) / 254) / PC.WEIGHTS.sum())                 # on the boundary between bins 111 and 112
    edge[0, 1, :3] = f32(0.0001)                                                                 # on the threshold between bins 0 and 1
    edge[0, 2, :3] = 0.3                                                                         # inside a bin
    sure, maybe, exact = R.histogram_bounds(edge)
    assert sure.sum() == 1 and maybe[111] == 1 and maybe[112] == 1 and maybe[0] == 1 and maybe[1] == 1 and maybe.sum() == 4


# ---------------------------------------------------------------- 2. the cases are what they claim to be
def test_ambiguity_cap():
    """The band is held by this cap: widening it to hide a wrong bin makes more pixels ambiguous than a case may have."""
    def share(images):
        amb = sum(int((a | b).sum()) for a, b in map(R.ambiguous, images))
        return amb / sum(i.shape[0] * i.shape[1] for i in images)
    assert share([PC.ladder()]) == 0.0
    shares = {"random": share([PC.random()]), "stride": share([PC.stride()]), "sequence": share(PC.sequence_frames())}
    print("ambiguous shares:", shares)
    assert all(s <= R.AMBIGUOUS_CAP for s in shares.values()), shares
    assert R.BAND == 1e-4 and R.AMBIGUOUS_CAP == 1e-3


def test_cases_reach_the_edges():
    b = R.bins(PC.random())
    assert (b == 0).any() and (b == 1).any() and (b == 255).any() and len(np.unique(b)) > 200
    assert PC.STRIDE_N == PC.stride().shape[1] and PC.STRIDE_N > 2 * 2048 * 256 and PC.STRIDE_N % 256 != 0
    black = np.concatenate([R.bins(f) for f in PC.black_frames()])
    assert not black.any()
    bp = PC.breakpoints()[0, :, :3].astype(f64)
    for v in (0.08, 1.0):
        assert (bp.min(-1) < v).any() and (bp == f64(f32(v))).any() and (bp.min(-1) > v).any()
    sdr = R.tonemap(PC.breakpoints(), 1.0, PC.params("sdr"))[0, :, :3]
    lin = 0.0031308 * 12.92
    assert ((sdr > 0) & (sdr < lin)).any() and (sdr > lin).any()
    for mode, top in (("hdr600", 7.5), ("hdr1000", 12.5)):
        hdr = R.tonemap(PC.breakpoints(), 1.0, PC.params(mode))[0, :, :3]
        assert (hdr >= f64(np.nextafter(f32(top), f32(0)))).any() and hdr.max() <= top           # the clamp region is reached
    for img in [PC.ladder(), PC.random(), PC.nonfinite(), PC.stride(), PC.breakpoints()]:
        assert not img.flags.writeable and (img.shape[0] * img.shape[1]) % 256 != 0


# ---------------------------------------------------------------- 3. the oracle against the statement
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(PC.SINGLE))
def test_oracle_single_frame(name, mode):
    run = oracle_single(name, mode)
    sure, maybe, exact = bounds_of(name)
    check_against_statement(run, run["disp"], run["e"], run["hist"], sure, maybe, f"oracle {name} {mode}")
    if name == "ladder":
        assert np.array_equal(run["hist"], exact)                    # no ambiguous pixel: the only legal histogram


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(PC.SEQUENCES))
def test_oracle_sequence(name, mode):
    runs = oracle_sequence(name, mode)
    for i, run in enumerate(runs):
        sure, maybe, _ = R.histogram_bounds(run["img"])
        check_against_statement(run, run["disp"], run["e"], run["hist"], sure, maybe, f"oracle {name}[{i}] {mode}")
    es = [ebits(r["e"]) for r in runs]
    if name == "dt0":
        assert all(e == ebits(1.0) for e in es)                  # dt = 0: the exposure does not move a bit
    elif name == "manual":
        assert all(e == ebits(0.37) for e in es)
    elif name == "black":
        target = 1.0 / (2.0 ** -7.0 * 1.2)                           # everything in bin 0: EV100 = -10 + 3, clamped at evmin = -7
        assert all(r["hist"][0] == r["hist"].sum() for r in runs)
        assert all(abs(float(r["e"]) - (float(r["e_in"]) + (target - float(r["e_in"])) * (1 - math.exp(-0.5)))) < 1e-5 * target for r in runs)
    else:
        assert len(set(es)) == len(es)               # different frames move the exposure


@pytest.mark.parametrize("mode", MODES)
def test_oracle_nonfinite(mode):
    run = oracle_single("nonfinite", mode)
    img, disp = run["img"], run["disp"]
    assert not np.isfinite(img[..., :3]).all(-1).all() and (disp[..., 3] == 1.0).all()
    if mode == "sdr":
        assert np.isfinite(disp).all() and (disp[..., :3] >= 0).all() and (disp[..., :3] <= 1).all()
    # the histogram rules, pixel by pixel: each special pixel alone in an image of its own
    flat = img.reshape(-1, 4)
    special = flat[~np.isfinite(flat[:, :3]).all(-1) | (np.abs(flat[:, :3]) == np.finfo(f32).max).any(-1)]
    assert len(special) == 24
    for px in special:
        one = np.ascontiguousarray(px.reshape(1, 1, 4))
        _, _, hist = post_process(one, run["params"], 1.0)
        assert hist.sum() == 1 and hist[int(R.bins(one)[0])] == 1, px


def test_oracle_threshold_is_strict():
    """A float32 luminance equal to the constant 0.0001 is not below it: bin 1 (by the clamp), and one step lower bin 0."""
    img, lum = PC.threshold()
    t = f32(0.0001)
    for px, l in zip(img.reshape(-1, 4), lum):
        _, _, hist = post_process(np.ascontiguousarray(px.reshape(1, 1, 4)), PC.params("sdr"), 1.0)
        assert hist.sum() == 1 and hist[0 if l < t else 1] == 1, (px, l)


def test_band_measurement():
    """Every pixel of every case within 3e-4 of a bin boundary, alone through the oracle: where float32 lands in another bin than binary64,
    the pixel is within BAND of the boundary. Prints the figures recorded next to post_reference.BAND."""
    images = [PC.random(), PC.stride(), PC.ladder(), PC.nonfinite()] + list(PC.sequence_frames())
    near = disagree = 0
    farthest = 0.0
    p = PC.params("sdr")
    for img in images:
        flat = img.reshape(-1, 4)
        near_b, near_t = R.ambiguous(img, 3e-4)
        _, raw, _, _ = R._positions(img)
        want = R.bins(img)
        for i in np.flatnonzero(near_b | near_t):
            one = np.ascontiguousarray(flat[i].reshape(1, 1, 4))
            _, _, hist = post_process(one, p, 1.0)
            near += 1
            if int(hist.argmax()) != want[i]:
                disagree += 1
                if near_b[i]:
                    farthest = max(farthest, abs(raw[i] - np.rint(raw[i])))
                else:
                    assert near_t[i] and abs(R.luminance(one)[0, 0] / R.LUM_THRESHOLD - 1) <= R.THRESHOLD_REL
    print(f"band: {near} pixels within 3e-4 of a boundary, {disagree} in another bin than binary64, the farthest {farthest:.2e} from its boundary")
    assert near > 300 and farthest <= R.BAND


def test_measured_maxima():
    """The largest distances of the oracle from the statement over all cases and modes: what post_reference's constants are 4 x of. A
    figure far above the recorded one means the statement or the oracle moved."""
    worst = dict(sdr_abs=0.0, hdr_abs=0.0, hdr_rel=0.0, exposure_rel=0.0)
    runs = [oracle_single(n, m) for n in PC.SINGLE for m in MODES] + [r for n in PC.SEQUENCES for m in MODES for r in oracle_sequence(n, m)]
    for run in runs:
        m = errors(run, run["disp"], run["e"], run["hist"])
        for k in worst:
            worst[k] = max(worst[k], m[k])
    print("measured maxima:", {k: f"{v:.3e}" for k, v in worst.items()})
    for k, bound in (("sdr_abs", R.SDR_ABS), ("hdr_abs", R.HDR_ABS), ("hdr_rel", R.HDR_REL), ("exposure_rel", R.EXPOSURE_REL)):
        assert worst[k] <= bound and bound <= 4.0 * 1.5 * max(worst[k], 1e-9), (k, worst[k], bound)     # 4 x the recorded maximum, and the record is current
