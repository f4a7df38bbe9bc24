"""The reference's blue-noise tile as a fixture (tests/golden/blue_noise_rg_64.png, a byte copy of its data file external/LDR_RG01_0.png,
which src/CommonResources.cpp:575 loads at run time) and native.noise_tile_from_png: what the file decodes to, that it IS blue noise and
the library's built-in default tile is not, and that hrpt_denoise_host given the tile equals the NumPy reference given the same tile."""
import os

import numpy as np

from hobbyrenderer_amd import native, scene_io
import denoise_cases as DC
import denoise_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "blue_noise_rg_64.png")
REFERENCE_FILE = "/root/reference/external/LDR_RG01_0.png"


def low_frequency_share(channel, radius=8):
    """Share of the spectral power (mean removed, DC excluded) at a radius of at most `radius` cycles per tile."""
    c = channel.astype(np.float64)
    p = np.abs(np.fft.fft2(c - c.mean())) ** 2
    f = np.fft.fftfreq(c.shape[0]) * c.shape[0]
    r = np.hypot(f[:, None], f[None, :])
    p[0, 0] = 0.0
    return float(p[r <= radius].sum() / p.sum())


def test_fixture_decodes_to_a_64x64_rg_tile():
    data = open(FIXTURE, "rb").read()
    assert len(data) == 11339
    if os.path.exists(REFERENCE_FILE):                             # where the reference tree is present: a byte copy of its file
        assert data == open(REFERENCE_FILE, "rb").read()
    rgba = scene_io.decode_image(data)
    assert rgba.shape == (64, 64, 4) and rgba.dtype == np.uint8
    assert (rgba[..., 2] == 0).all() and (rgba[..., 3] == 255).all()
    tile = native.noise_tile_from_png(FIXTURE)
    assert tile.shape == (64, 64, 2) and tile.dtype == np.float32
    want = (rgba[..., :2].astype(np.float64) / 255.0).astype(np.float32)          # correctly rounded: float64 quotient of two small integers, rounded once
    assert np.array_equal(tile.view(np.uint32), want.view(np.uint32))
    assert tile.min() >= 0 and tile.max() <= 1 and len(np.unique(rgba[..., 0])) > 200


def test_the_fixture_is_blue_noise_and_the_default_tile_is_not():
    tile = native.noise_tile_from_png(FIXTURE)
    default = R.default_tile()
    for k in range(2):
        blue, white = low_frequency_share(tile[..., k]), low_frequency_share(default[..., k])
        print(f"channel {k}: share of power at radius <= 8: fixture {blue:.2e}, default tile {white:.2e}")
        assert blue < 1e-3
        assert white >= 10 * blue


def test_denoise_host_with_the_tile_equals_the_reference_with_it():
    w, h = 37, 23
    c = DC.case(w, h)
    tile = native.noise_tile_from_png(FIXTURE)
    for frame in (0, 5):
        lib = native.denoise_host(c["input"], c["depth"], c["normal"], c["geo"], c["view"], DC.params(3.0, frame), noise=tile)
        ref = R.denoise(c["input"], c["depth"], c["normal"], c["geo"], c["view"], radius=3.0, frame=frame, noise=tile)
        assert np.array_equal(lib.view(np.uint32), ref.view(np.uint32)), frame
        default = native.denoise_host(c["input"], c["depth"], c["normal"], c["geo"], c["view"], DC.params(3.0, frame))
        assert not np.array_equal(lib.view(np.uint32), default.view(np.uint32))
