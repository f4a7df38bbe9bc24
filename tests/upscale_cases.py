"""Synthetic inputs of the upscale-stage tests (tests/test_upscale_cpu.py, tests/test_upscale_gpu.py): a render-size frame in the layout
hrpt_render / hrpt_render_motion_vectors write it -- the depth plane of tests/temporal_cases.py (a far tilted plane, a near box, a border of
misses on two sides wide enough for all-miss neighbourhoods, a few isolated misses), radiance with fireflies and a random alpha, a motion
plane -- and a display-size history whose sample weights straddle the default maxHistory. The reference result of a case is computed once
and shared by every test that asks for it."""
import functools

import numpy as np

from hobbyrenderer_amd import structs as S
import temporal_cases as TC
import upscale_reference as R

F = np.float32
# (w, h) -> (W, H): 1x plain TAA, 2x, a non-integer ratio, 3x, many and partial 32 x 8 tiles, an image narrower than a tap footprint
SIZE_PAIRS = [((16, 9), (16, 9)), ((20, 12), (40, 24)), ((37, 23), (55, 34)), ((33, 17), (99, 51)), ((100, 60), (200, 120)), ((1, 5), (3, 5))]
MOTIONS = ["zero", "pan", "random", "offscreen"]
JITTER = (0.3125, -0.4375)               # the non-zero one; exactly representable, so that the statement's sums are easy to follow by hand


def pair_id(pair):
    (w, h), (W, H) = pair
    return f"{w}x{h}-{W}x{H}"


def motion_plane(name, w, h, hit, seed=2):
    """.xy in render pixels, this -> last frame; .z the change of view depth, .w the valid flag (neither is read by the stage)."""
    rng = np.random.default_rng(seed)
    mv = np.zeros((h, w, 4), np.float32)
    if name == "pan":
        mv[..., 0], mv[..., 1] = 1.37, -0.62
    elif name == "random":                      # +-4 px per texel: history taps over every image edge, some reprojections outside [0, 1]
        mv[..., :2] = rng.uniform(-4.0, 4.0, (h, w, 2)).astype(np.float32)
    elif name == "offscreen":                   # every reprojection leaves the image
        mv[..., 0] = -(w + 3.0)
    else:
        assert name == "zero"
    mv[..., 2] = rng.uniform(-0.1, 0.1, (h, w)).astype(np.float32)
    mv[..., 3] = 1.0
    mv[~hit] = 0.0
    return mv


def history(W, H, seed):
    c = TC.radiance(W, H, seed)
    c[..., 3] = np.random.default_rng(seed + 1).uniform(0.0, 12.0, (H, W)).astype(np.float32)
    return c


@functools.lru_cache(maxsize=None)
def case(name, pair, jitter):
    """jitter False: zero jitter and equal m_PixelOffset in the two views; True: JITTER and differing offsets."""
    (w, h), (W, H) = pair
    depth, _, hit = TC.planes(w, h)
    view, prev = TC.views(w, h, jitter)
    color = TC.radiance(w, h, 10)
    color[..., 3] = np.random.default_rng(3).random((h, w)).astype(np.float32)
    c = dict(color=color, depth=depth, motion=motion_plane(name, w, h, hit), hit=hit, view=view, prev=prev, history=history(W, H, 20),
             size=(w, h), display=(W, H), jitter=JITTER if jitter else (0.0, 0.0))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)             # shared between tests: nobody edits a case in place
    return c


def params(c, clamp=True, extra_flags=0, **kw):
    return S.UpscaleParams(jitter=c["jitter"], flags=(0 if clamp else S.UPSCALE_NO_CLAMP) | extra_flags, **kw)


@functools.lru_cache(maxsize=None)
def reference(name, pair, jitter, with_history, clamp):
    """(colorOut, historyOut, details) of the NumPy restatement for a case, computed once per process."""
    c = case(name, pair, jitter)
    out = R.upscale(c["color"], c["depth"], c["motion"], c["history"] if with_history else None, c["display"], c["view"], c["prev"],
                    jitter=c["jitter"], clamp=clamp, details=True)
    for a in out[:2]:
        a.setflags(write=False)
    return out


# ---- the convergence construction: a truth image at the display size, frames that sample it where their jittered samples lie ----
CYCLE = [(-0.25, -0.25), (0.25, -0.25), (-0.25, 0.25), (0.25, 0.25)]      # at 2x every sample lies exactly on a display pixel centre


def checkerboard(x, y):
    return ((x + y) % 2).astype(np.float32)


def sinusoid(x, y):
    return (0.5 + 0.5 * np.sin(2.0 * np.pi * x / 6.0) + 0.0 * y).astype(np.float32)


def truth(pattern, W, H, shift=0):
    """[H, W, 4] display-size image of pattern(x - shift, y), alpha 1."""
    y, x = np.mgrid[0:H, 0:W]
    t = np.ones((H, W, 4), np.float32)
    t[..., :3] = pattern(x - shift, y)[..., None]
    return t


def frame_of(truth_image, jitter):
    """The 2x-smaller frame whose texel (i, j) is the truth at the display pixel its sample (i + 0.5 + jx, j + 0.5 + jy) * 2 falls on."""
    ox, oy = int(jitter[0] > 0), int(jitter[1] > 0)
    return np.ascontiguousarray(truth_image[oy::2, ox::2])
