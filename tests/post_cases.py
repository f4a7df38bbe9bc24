"""Inputs for the post-chain tests that reach the edges a rendered frame never does -- TEST INFRASTRUCTURE.

Deterministic and seeded; every array is float32 [H, W, 4] (alpha 1) and read-only. Pixel counts are no multiple of 256 unless a case
exists for the opposite reason (`counts`). `params()` builds the S.PostParams of a pass; MODES are the three display modes every case is
run in."""
import functools

import numpy as np

from hobbyrenderer_amd import structs as S
import post_reference as R

f32 = np.float32
WEIGHTS = np.array([0.2126, 0.7152, 0.0722])
MODES = {"sdr": (0, 80.0), "hdr600": (1, 600.0), "hdr1000": (1, 1000.0)}
STRIDE_N = 2 * 524288 + 773           # the launch caps the grid at 2048 blocks of 256 threads: two full trips, 773 threads make a third
COUNTS = (1, 63, 64, 65, 255, 256, 257)


def params(mode="sdr", auto=1, manual=1.0, dt=0.016, speed=5.0, evmin=-7.0, evmax=23.0, comp=0.0):
    hdr, nits = MODES[mode]
    return S.PostParams(auto, manual, dt, speed, evmin, evmax, comp, hdr, nits)


def _image(rgb, shape=None):
    rgb = np.asarray(rgb, f32).reshape(-1, 3)
    img = np.ones((len(rgb), 4), f32)
    img[:, :3] = rgb
    img = img.reshape(shape + (4,) if shape else (1, len(rgb), 4))
    img.setflags(write=False)
    return img


def _with_luminance(rng, lum):
    """Pixels of the given luminances (float64) with random chroma, uniform in [0.05, 1] per channel."""
    chroma = rng.uniform(0.05, 1.0, (len(lum), 3))
    return chroma * (np.asarray(lum) / (chroma @ WEIGHTS))[:, None]


def _random_rgb(seed, n, lo=-16.0, hi=22.0):
    rng = np.random.default_rng(seed)
    return _with_luminance(rng, np.exp2(rng.uniform(lo, hi, n)))


@functools.lru_cache(None)
def ladder():
    """Every bin on purpose: 1 + (k mod 7) pixels at the centre of bin k = 1 ... 254, bin 1 by the clamp, bin 255 and bin 0 each in every
    way the definition names. No pixel is ambiguous (asserted), so the binary64 histogram is the only legal answer. 2^20 is itself the
    boundary between bins 254 and 255, so its pixel sits 2^-13 above it in log2 (7 bands)."""
    rng = np.random.default_rng(20261020)
    k = np.repeat(np.arange(1, 255), 1 + np.arange(1, 255) % 7)
    rows = [_with_luminance(rng, R.bin_centre(k)),
            _with_luminance(rng, [0.0003, 0.0009]),                                    # bin 1 by the clamp: 0.0001 <= lum < 2^-10
            _with_luminance(rng, [2.0 ** (20 + 2.0 ** -13), 2.0 ** 21, 1e30]),         # bin 255, by value and by the clamp
            [[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [0.5, -0.25, 0.5], [1e-39, 1e-39, 1e-39],      # bin 0: zero, -0, negative, subnormal
             [0.00009, 0.00009, 0.00009]]]                                             # ... and just below 0.0001
    rgb = np.concatenate([np.asarray(r, np.float64) for r in rows])
    img = _image(rgb[rng.permutation(len(rgb))])
    near_b, near_t = R.ambiguous(img)
    assert not near_b.any() and not near_t.any(), "the ladder must hold no ambiguous pixel"
    assert img.shape[1] % 256 != 0
    return img


@functools.lru_cache(None)
def random():
    """61 x 37, luminance log-uniform over 2^-16 ... 2^22 (both clamp ends, bin 0 by the threshold), random chroma."""
    return _image(_random_rgb(1, 61 * 37), (37, 61))


def _around(v):
    v = f32(v)
    return [v, np.nextafter(v, f32(-np.inf)), np.nextafter(v, f32(np.inf)), v * f32(0.97), v * f32(0.99), v * f32(1.01), v * f32(1.03)]


@functools.lru_cache(None)
def breakpoints():
    """Every branch value of the two tonemappers: a pixel at the value, its two float32 neighbours and 1 % and 3 % either side, once with the
    other channels equal and once different. Run with manual exposure 1, so the values arrive unscaled.
    SDR: 0.08 (minimum channel), 0.76 (peak after the 0.04 offset), 0.0031308 (tonemapped value). HDR: 1.0 (maximum channel), and
    luminances (maxNits / 80 - 1) * 2^j, where the compressed peak rounds up to maxNits / 80 and the clamp takes over."""
    px = []
    for s in _around(0.08):
        px += [[s, s, s], [s, 0.3, 0.5]]
    for s in _around(0.76):
        t = f32(s + f32(0.04))
        px += [[t, t, t], [0.2, t, 0.5]]
    for s in _around(0.0031308):
        g = f32(np.sqrt(np.float64(s) / 6.25))                   # grey below 0.08: the toe leaves 6.25 g^2
        px += [[g, g, g], [0.2, f32(s + f32(0.04)), 0.1]]
    for s in _around(1.0):
        px += [[s, s, s], [0.3, s, 0.6]]
    for nits in (600.0, 1000.0):
        for j in range(16, 32, 2):
            s = f32((nits / 80.0 - 1.0) * 2.0 ** j)
            px += [[s, s, s], [s * f32(0.999), s, -s]]
    px.append([0.25, 0.5, 0.75])                                  # 113 pixels
    img = _image(px)
    assert img.shape[1] % 256 != 0
    return img


@functools.lru_cache(None)
def nonfinite():
    """NaN, +Inf, -Inf and FLT_MAX in one channel and in all three, among ordinary pixels."""
    rgb = _random_rgb(2, 19 * 11, -6.0, 6.0).astype(f32)
    specials = [f32(np.nan), f32(np.inf), f32(-np.inf), np.finfo(f32).max]
    at = np.random.default_rng(3).permutation(len(rgb))[:6 * len(specials)].reshape(len(specials), 6)
    for v, idx in zip(specials, at):
        for ch in range(3):
            rgb[idx[ch], ch] = v
        rgb[idx[3]] = v
        rgb[idx[4], (0, 2)] = v
        rgb[idx[5], 1] = -v
    return _image(rgb, (11, 19))


@functools.lru_cache(None)
def threshold():
    """Red-only pixels around 0.0001 / 0.2126, one float32 step apart. With green and blue zero the float32 luminance is one rounded product,
    fl32(0.2126f * r), whatever the order or contraction of the dot product, so it is known exactly: some pixels give exactly the float32
    constant 0.0001 (asserted), which `lum < 0.0001` sends to bin 1, their lower neighbours go to bin 0. Returns (image, that luminance)."""
    w, t = f32(0.2126), f32(0.0001)
    r = (f32(t / w).view(np.uint32) + np.arange(-8, 9)).astype(np.uint32).view(f32)
    lum = (r * w).astype(f32)
    assert (lum == t).any() and (lum < t).any() and (lum > t).any()
    rgb = np.zeros((len(r), 3), f32)
    rgb[:, 0] = r
    lum.setflags(write=False)
    return _image(rgb), lum


@functools.lru_cache(None)
def stride():
    """STRIDE_N pixels as one row, of the `random` recipe: the smallest size at which a wrong stride, a wrong bound or a lost tail shows."""
    return _image(_random_rgb(4, STRIDE_N))


@functools.lru_cache(None)
def counts(n):
    """The first n pixels of `random`, around the wave and block sizes."""
    img = random().reshape(-1, 4)[:n].reshape(1, n, 4)
    img.setflags(write=False)
    return img


@functools.lru_cache(None)
def sequence_frames():
    """Four different small images for one exposure buffer: dark, bright, wide, and mid-grey with highlights."""
    return (_image(_random_rgb(10, 23 * 17, -9.0, -3.0), (17, 23)), _image(_random_rgb(11, 23 * 17, 2.0, 9.0), (17, 23)),
            _image(_random_rgb(12, 31 * 9, -16.0, 22.0), (9, 31)), _image(_random_rgb(13, 13 * 29, -3.0, 4.0), (29, 13)))


@functools.lru_cache(None)
def black_frames():
    """Every pixel in bin 0 (zero, tiny, negative luminance): EV100 is clamped at evmin."""
    rng = np.random.default_rng(14)
    rgb = rng.uniform(0.0, 0.00009, (4, 15 * 7, 3))
    rgb[1] = 0.0
    rgb[2, ::3, 1] = -0.5
    return tuple(_image(f, (7, 15)) for f in rgb)


# name -> (frames, keyword arguments of params()); the exposure buffer starts at 1 and is carried from frame to frame
SEQUENCES = {
    "defaults": (sequence_frames, {}),
    "dt0": (sequence_frames, dict(dt=0.0)),
    "fast": (sequence_frames, dict(dt=10.0, speed=5.0)),
    "ev3": (sequence_frames, dict(evmin=3.0, evmax=3.0, dt=0.1)),
    "comp+2": (sequence_frames, dict(comp=2.0, dt=0.1)),
    "comp-2": (sequence_frames, dict(comp=-2.0, dt=0.1)),
    "black": (black_frames, dict(dt=0.1)),
    "manual": (sequence_frames, dict(auto=0, manual=0.37)),
}

# name -> (image, keyword arguments of params()): the single-frame cases, each run in every mode of MODES from exposure 1
SINGLE = {
    "ladder": (ladder, {}),
    "random": (random, {}),
    "breakpoints": (breakpoints, dict(auto=0, manual=1.0)),
    "nonfinite": (nonfinite, {}),
    "stride": (stride, {}),
    "threshold": (lambda: threshold()[0], {}),
}
SINGLE.update({f"counts{n}": (functools.partial(counts, n), {}) for n in COUNTS})
