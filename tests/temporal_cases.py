"""Synthetic inputs of the temporal-stage tests (tests/test_temporal_cpu.py, tests/test_temporal_gpu.py): planes in the layout
hrpt_render_gbuffer / hrpt_render_motion_vectors write them, without a scene. A far tilted plane (view depth 9..13) with a near box in the
middle (view depth 2: depth and normal edges, and a discontinuity large enough for confidence 0) and a border of misses on two sides plus
a few isolated ones; radiance, history and motion from a seeded generator."""
import numpy as np

from hobbyrenderer_amd import scenes, structs as S

F = np.float32
SIZES = [(37, 23), (64, 36)]
MOTIONS = ["zero", "integer", "subpixel", "random", "capped"]
BLEND = {"capped": 0.5}                  # the others use the default 0.9


def views(w, h, jitter):
    """(view, prevView) with the camera position filled in (scenes.planar_view leaves it zero); jitter: differing m_PixelOffset."""
    view, pos = scenes.planar_view(w, h, position=(0.3, 1.2, -4.0), yaw=0.1, pitch=0.15)
    view["m_CameraDirectionOrPosition"] = (pos[0], pos[1], pos[2], 1.0)
    prev = view.copy()
    if jitter:
        view["m_PixelOffset"] = (0.25, -0.125)
        prev["m_PixelOffset"] = (-0.3125, 0.4375)
    return view, prev


def planes(w, h, seed=1):
    """depth (t, viewDepth, u, v), normal (N, roughness), and the hit mask."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    vd = (9.0 + 4.0 * x / max(w - 1, 1) + 0.5 * y / max(h - 1, 1)).astype(np.float32)
    normal = np.zeros((h, w, 4), np.float32)
    n = np.array([0.2, 0.9, -0.38]); n /= np.linalg.norm(n)
    normal[..., :3] = n
    box = (x >= w // 3) & (x < (2 * w) // 3) & (y >= h // 3) & (y < (2 * h) // 3)
    vd[box] = 2.0
    normal[box, :3] = (0.0, 0.0, -1.0)
    normal[..., 3] = 0.5
    hit = np.ones((h, w), bool)
    if w > 4 and h > 4:
        hit[:, :2] = False; hit[-2:, :] = False
        hit &= rng.random((h, w)) > 0.02
    depth = np.zeros((h, w, 4), np.float32)
    depth[..., 0] = vd * F(1.01); depth[..., 1] = vd
    depth[..., 2:] = rng.random((h, w, 2), np.float32)
    depth[~hit] = (1e10, 1e10, 0.0, 0.0)
    normal[~hit] = 0.0
    return depth, normal, hit


def motion_plane(name, w, h, hit, seed=2):
    rng = np.random.default_rng(seed)
    mv = np.zeros((h, w, 4), np.float32)
    if name == "integer":
        mv[..., 0], mv[..., 1] = 3.0, -2.0
    elif name == "subpixel":
        mv[..., 0], mv[..., 1] = 0.37, -1.62
    elif name == "random":                      # +-4 px per pixel: taps over every image edge, reprojection outside [0, 1]
        mv[..., :2] = rng.uniform(-4.0, 4.0, (h, w, 2)).astype(np.float32)
    elif name == "capped":                      # 1 < |motion| < 2: moveFactor strictly between 0 and 1
        mv[..., 0], mv[..., 1] = 1.25, 0.75
    else:
        assert name == "zero"
    mv[..., 2] = rng.uniform(-0.1, 0.1, (h, w)).astype(np.float32)
    mv[..., 3] = 1.0
    mv[~hit] = 0.0
    return mv


def radiance(w, h, seed, fireflies=True):
    rng = np.random.default_rng(seed)
    c = np.ones((h, w, 4), np.float32)
    c[..., :3] = (rng.random((h, w, 3)) * (4.0, 1.0, 0.25)).astype(np.float32)
    if fireflies:
        c[rng.random((h, w)) < 0.01, :3] *= F(50.0)       # what the anti-ringing clamp is for
    return c


def history(w, h, seed):
    """A history image with ages 0..30, so that accumBlend exceeds the motion cap at some pixels and not at others."""
    c = radiance(w, h, seed)
    c[..., 3] = np.random.default_rng(seed + 1).uniform(0.0, 30.0, (h, w)).astype(np.float32)
    return c


def case(name, w, h, jitter):
    depth, normal, hit = planes(w, h)
    view, prev = views(w, h, jitter)
    return dict(color=radiance(w, h, 10), motion=motion_plane(name, w, h, hit), depth=depth, normal=normal, hit=hit, view=view, prev=prev,
                history=history(w, h, 20), blend=BLEND.get(name, 0.9))


def params(blend, linear, extra_flags=0):
    return S.TemporalParams(blend, (S.TEMPORAL_LINEAR if linear else 0) | extra_flags)
