"""NumPy float64 statement of the HDR post chain (hrpt_post_process) -- TEST INFRASTRUCTURE.

Written from the definition: the reference's three shaders (LuminanceHistogram.hlsl, ExposureAdaptation.hlsl, Tonemap.hlsl) with the log
range -10 ... 20 its HDR renderer drives them with. It shares no code with the kernels of the post chain or with the CPU oracle, was not
derived from either, calls neither, and uses none of the project's deterministic math: the inputs are the float32 images and parameters
widened exactly, everything after that is binary64 with np.log2, np.exp2, np.power and math.exp.

The definition
  luminance   lum = 0.2126 r + 0.7152 g + 0.0722 b
  bin         0 when lum < 0.0001 (the float32 constant, widened); else floor(clamp((log2(lum) + 10) / 30, 0, 1) * 254 + 1), in 1 ... 255
  adaptation  bin 0 stands for log-luminance -10, bin k >= 1 for -10 + 30 (k - 1) / 254; avg = sum(count * value) / max(n, 1);
              EV100 = log2(2^avg * 100 / 12.5), clamped to [evMin, evMax], minus the compensation; target = 1 / (2^EV100 * 1.2);
              exposure' = exposure + (target - exposure) * (1 - exp(-dt * speed)). Manual mode: exposure' = manualExposure, histogram zero.
  SDR tonemap c = rgb * exposure'; x = min channel; offset = x - 6.25 x^2 when x < 0.08, else 0.04; c -= offset; peak = max channel;
              when peak >= 0.76: d = 0.24, newPeak = 1 - d^2 / (peak + d - 0.76), c *= newPeak / peak,
              g = 1 - 1 / (0.15 (peak - newPeak) + 1), c = lerp(c, newPeak, g); then per channel the sRGB curve
              saturate(v <= 0.0031308 ? 12.92 v : 1.055 v^(1/2.4) - 0.055). Alpha 1.
  HDR tonemap c = rgb * exposure'; m = maxNits / 80; lum = max channel; unchanged when lum <= 1; else h = m - 1, e = lum - 1,
              c = min(c * ((1 + e h / (e + h)) / lum), m). Alpha 1.

Non-finite and negative input is part of the definition: min, max and clamp return the operand that is not NaN, and saturate(NaN) = 0.
So, for the histogram, a NaN luminance lands in bin 1 (NaN < 0.0001 is false, log2 gives NaN, the clamp's max returns its 0), +Inf lands in
bin 255, and -Inf, negative, zero and subnormal luminance land in bin 0. A negative channel makes `offset` negative and so a bright SDR
pixel; a NaN channel passes through the HDR path. The tonemap of this file is compared with float32 code only on input inside its domain
(`tonemap_domain`): every channel finite and, after exposure, within +-2^100, beyond which float32 products of the definition (value times
exposure, excess times headroom) overflow where binary64 ones do not.

Positions and bands: `bin_position` is the real-valued position whose floor is the bin. A float32 evaluation (float32 luminance, a log2
good to 1.2e-7 relative + 3e-7 absolute, the rounding of logLum * 254 + 1) moves it by 2-4e-5 at most, so a pixel whose position lies within
BAND of an integer boundary, or whose luminance lies within 4e-7 relative of the 0.0001 threshold, may legally land in either neighbouring
bin: `histogram_bounds` counts those into `maybe` and all others into `sure`."""
import math

import numpy as np

f64 = np.float64

MIN_LOG, MAX_LOG = -10.0, 20.0
LUM_THRESHOLD = f64(np.float32(0.0001))
THRESHOLD_REL = 4e-7

# ---- what float32 code is held to. Fixed from the CPU oracle against this statement (tests/test_post_reference_cpu.py measures them again
# ---- on every run and prints them), never from a device run; the device is held to the same constants.
# Band, in bin positions. Derivation: 2-4e-5 (above). Measured 2026-10-20 over all cases of post_cases.py: 428 pixels within 3e-4 of a
# boundary, 2 of them in another bin than binary64 puts them, the farthest 3.56e-6 from its boundary.
BAND = 1e-4
AMBIGUOUS_CAP = 1e-3            # a condition, not a tolerance: the share of ambiguous pixels a case may have (0 on the ladder)
# Display and exposure: 4 x the largest distance of the CPU oracle from this statement over all cases and display modes, measured 2026-10-20.
SDR_ABS = 4 * 2.73e-7           # absolute; measured 2.728e-7
HDR_ABS = 4 * 2.17e-7           # absolute, where |ref| <= 1; measured 2.163e-7. The bound is HDR_ABS + HDR_REL * |ref|
HDR_REL = 4 * 2.84e-7           # relative, where |ref| > 1 (up to maxNits / 80); measured 2.834e-7
EXPOSURE_REL = 4 * 2.61e-7      # relative to the larger of the old and the new exposure (the update is a float32 lerp); measured 2.603e-7

TONEMAP_DOMAIN_MAX = 2.0 ** 100


def _wide(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, "the statement takes float32 input and widens it itself"
    return a.astype(f64)


def _clamp(x, lo, hi):           # min / max return the operand that is not NaN
    return np.fmin(np.fmax(x, lo), hi)


def _saturate(x):                # saturate(NaN) = 0
    return np.where(x > 0, np.where(x < 1, x, 1.0), 0.0)


def luminance(hdr):
    c = _wide(hdr)
    with np.errstate(invalid="ignore", over="ignore"):
        return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def _positions(hdr):
    """(clamped position in [1, 255], unclamped position, lum < threshold, lum), flat."""
    lum = luminance(hdr).ravel()
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (np.log2(lum) - MIN_LOG) / (MAX_LOG - MIN_LOG)
    return _clamp(t, 0.0, 1.0) * 254.0 + 1.0, t * 254.0 + 1.0, lum < LUM_THRESHOLD, lum


def bin_position(hdr):
    """Per pixel: clamp((log2(lum) + 10) / 30, 0, 1) * 254 + 1, whose floor is the bin of a pixel not below the threshold, and the mask
    lum < 0.0001 of the pixels that go to bin 0 whatever their position. Flat arrays."""
    pos, _, below, _ = _positions(hdr)
    return pos, below


def bins(hdr):
    """The bin of every pixel, exactly as binary64 evaluates the definition."""
    pos, below = bin_position(hdr)
    return np.where(below, 0, np.floor(pos).astype(np.int64))


def ambiguous(hdr, band=BAND):
    """(near a bin boundary, near the threshold): the pixels float32 code may put into the neighbouring bin. Boundaries are the integers
    2 ... 255 of the unclamped position, so a clamped pixel far outside the range is not ambiguous."""
    _, raw, below, lum = _positions(hdr)
    with np.errstate(invalid="ignore"):
        near_t = np.abs(lum / LUM_THRESHOLD - 1.0) <= THRESHOLD_REL
        m = np.rint(raw)
        near_b = (np.abs(raw - m) <= band) & (m >= 2) & (m <= 255) & ~below & ~near_t
    return near_b, near_t


def histogram_bounds(hdr, band=BAND):
    """(sure, maybe, exact), 256 entries each. exact: the binary64 histogram. A legal float32 histogram h sums to n and has
    sure[k] <= h[k] <= sure[k] + maybe[k] in every bin: an ambiguous pixel counts into `maybe` of both neighbouring bins, every other
    pixel into `sure` of its bin."""
    _, raw, _, _ = _positions(hdr)
    b = bins(hdr)
    near_b, near_t = ambiguous(hdr, band)
    exact = np.bincount(b, minlength=256)
    sure = np.bincount(b[~(near_b | near_t)], minlength=256)
    maybe = np.zeros(256, np.int64)
    m = np.rint(raw[near_b]).astype(np.int64)                      # the boundary between bins m - 1 and m
    maybe += np.bincount(m, minlength=256) + np.bincount(m - 1, minlength=256)
    maybe[0] += int(near_t.sum()); maybe[1] += int(near_t.sum())   # 0.0001 < 2^-10: the threshold separates bin 0 from bin 1
    return sure, maybe, exact


def bin_value(k):
    """The log2 luminance bin k stands for in the adaptation."""
    k = np.asarray(k, f64)
    return np.where(k == 0, MIN_LOG, MIN_LOG + (k - 1.0) / 254.0 * (MAX_LOG - MIN_LOG))


def bin_centre(k):
    """The luminance in the middle (in log2) of bin k = 1 ... 254."""
    return np.exp2(MIN_LOG + (MAX_LOG - MIN_LOG) * (np.asarray(k, f64) - 0.5) / 254.0)


def adapt(histogram, n, params, exposure):
    """The exposure after one pass over an integer histogram of an n-pixel image; the weighted sum is exact (integers)."""
    p = params
    if not p.autoExposure:
        return float(np.float32(p.manualExposure))
    h = [int(v) for v in np.asarray(histogram).ravel()]
    assert len(h) == 256
    steps = sum(c * (k - 1) for k, c in enumerate(h) if k >= 1)               # sum of count * (k - 1), an integer
    total = MIN_LOG * sum(h) + steps * (MAX_LOG - MIN_LOG) / 254.0
    avg = total / max(float(n), 1.0)
    ev = math.log2(2.0 ** avg * 100.0 / 12.5)
    ev = float(_clamp(ev, f64(np.float32(p.exposureValueMin)), f64(np.float32(p.exposureValueMax))))
    ev -= float(np.float32(p.exposureCompensation))
    target = 1.0 / (2.0 ** ev * 1.2)
    cur = float(np.float32(exposure))
    return cur + (target - cur) * (1.0 - math.exp(-float(np.float32(p.deltaTimeSeconds)) * float(np.float32(p.adaptationSpeed))))


def tonemap_domain(hdr, exposure):
    """The pixels on which float32 code is compared with `tonemap`: see the module docstring."""
    c = _wide(hdr)[..., :3]
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.isfinite(c) & (np.abs(c * float(exposure)) <= TONEMAP_DOMAIN_MAX)).all(-1)


def _sdr(c):
    x = np.fmin(c[..., 0], np.fmin(c[..., 1], c[..., 2]))
    offset = np.where(x < 0.08, x - 6.25 * x * x, 0.04)
    c = c - offset[..., None]
    peak = np.fmax(c[..., 0], np.fmax(c[..., 1], c[..., 2]))
    d = 1.0 - 0.76
    new_peak = 1.0 - d * d / (peak + d - 0.76)
    g = 1.0 - 1.0 / (0.15 * (peak - new_peak) + 1.0)
    k = (c * (new_peak / peak)[..., None])
    k = k + (new_peak[..., None] - k) * g[..., None]
    t = np.where((peak < 0.76)[..., None], c, k)
    curve = 1.055 * np.power(np.where(t > 0, t, 0.0), 1.0 / 2.4) - 0.055     # only taken where t > 0.0031308
    return _saturate(np.where(t <= 0.0031308, t * 12.92, curve))


def _hdr(c, max_nits):
    m = float(np.float32(max_nits)) / 80.0
    lum = np.fmax(c[..., 0], np.fmax(c[..., 1], c[..., 2]))
    h, e = m - 1.0, lum - 1.0
    new_lum = 1.0 + e * h / (e + h)
    out = np.fmin(c * (new_lum / lum)[..., None], m)
    return np.where((lum <= 1.0)[..., None], c, out)


def tonemap(hdr, exposure, params):
    """The display image, float64 [..., 4], for the exposure the pass left (float32, widened)."""
    c = _wide(hdr)[..., :3] * float(np.float32(exposure))
    with np.errstate(all="ignore"):
        rgb = _hdr(c, params.maxDisplayNits) if params.hdrDisplay else _sdr(c)
    return np.concatenate([rgb, np.ones(rgb.shape[:-1] + (1,))], -1)
