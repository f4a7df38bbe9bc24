"""Synthetic planes, light lists, motion and histories for the resampled-lighting tests (test_restir_cpu.py, test_restir_gpu.py) -- TEST
INFRASTRUCTURE.

A case is deferred_cases' case (its planes, constants, nine lights, atmosphere images) with the light list extended to 40 and to 520 lights
(520 crosses HRPT_RESTIR_LDS_MAX_LIGHTS), a motion plane, a history (reservoirs and keys) and two visibility planes. Pixels are edited so that
the branches no camera produces reliably are in frame (SPECIAL, at sizes that hold them): deferred_cases' light exactly at X; a pixel at which
every light is culled (a zero normal: dot(N, L) == 0 for all of them); a previous pixel off-screen; a motion texel with w == 0; a history
record whose light index is not below the light count, and an empty one. The light counts 0 and 1 are cases of their own."""
import functools

import numpy as np

from hobbyrenderer_amd import structs as S
import deferred_cases as DC

f32 = np.float32
SIZES = DC.SIZES
LIGHT_COUNTS = [0, 1, 9, 40, 520]
SPECIAL = {"all_culled": (8, 5), "off_screen": (0, 0), "motion_w0": (2, 1), "history_light_out_of_range": (3, 2), "history_empty": (4, 2)}


@functools.lru_cache(maxsize=None)
def lights(count, width, height):
    """deferred_cases' nine lights of that size followed by seeded point and spot lights about the surfaces, S.GPULight [count]."""
    base = DC.case(width, height)["lights"]
    rng = np.random.default_rng(77)
    out = [base[i] for i in range(min(count, 9))]
    for k in range(9, count):
        spot = k % 3 == 0
        out.append(DC._light(S.LIGHT_SPOT if spot else S.LIGHT_POINT, position=(rng.uniform(-2.5, 2.5), rng.uniform(-1.5, 3.0), rng.uniform(-4.0, 1.5)),
                             direction=(rng.uniform(-0.5, 0.5), -1.0, rng.uniform(-0.5, 0.5)), color=tuple(rng.uniform(0.2, 1.0, 3)), intensity=rng.uniform(1.0, 6.0),
                             range_=0.0 if k % 2 else rng.uniform(3.0, 6.0), inner=0.4, outer=1.1))
    a = np.array(out, S.GPULight) if out else np.zeros(0, S.GPULight)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(width, height, count):
    """dict: planes, cb (m_LightCount = count), lights [count], motion, history (reservoirs, keys), sun_radiance, sky, visibility [2, H, W],
    special, miss. Read-only: shared between tests."""
    c = DC.case(width, height)
    H, W = height, width
    rng = np.random.default_rng(5 + 1000 * width + height)
    planes = [np.array(p) for p in c["planes"]]
    special = {k: p for k, p in SPECIAL.items() if p[0] < W and p[1] < H}
    miss = c["miss"].copy()
    for x, y in special.values():
        if miss[y, x]:                                       # a special pixel is a hit
            miss[y, x] = False
            planes[4][y, x, :2] = 3.5
    if "all_culled" in special:
        x, y = special["all_culled"]
        planes[1][y, x, :3] = 0.0
    cb = DC.with_lights(c["cb"], count)
    motion = np.zeros((H, W, 4), f32)
    moving = rng.uniform(size=(H, W)) < 0.5
    motion[..., :2] = np.where(moving[..., None], rng.uniform(-2.5, 2.5, (H, W, 2)), 0.0)
    motion[..., 2] = rng.uniform(-0.4, 0.4, (H, W)) * (rng.uniform(size=(H, W)) < 0.7)
    motion[..., 3] = np.where(rng.uniform(size=(H, W)) < 0.9, 1.0, 0.0)
    for name, m in (("off_screen", (-3.0, -2.0, 0.0, 1.0)), ("motion_w0", (0.0, 0.0, 0.0, 0.0)), ("history_light_out_of_range", (0.0, 0.0, 0.0, 1.0)),
                    ("history_empty", (0.0, 0.0, 0.0, 1.0))):
        if name in special:
            motion[special[name][1], special[name][0]] = m
    hres = np.zeros((H, W), S.RestirReservoir)
    hres["light"] = rng.integers(0, max(count, 1), (H, W))
    hres["W"], hres["M"], hres["pHat"] = rng.uniform(0.0, 2.0, (H, W)), rng.integers(1, 40, (H, W)), rng.uniform(0.01, 1.0, (H, W))
    hres["light"][rng.uniform(size=(H, W)) < 0.1] = S.RESTIR_EMPTY
    if "history_light_out_of_range" in special:
        hres["light"][special["history_light_out_of_range"][1], special["history_light_out_of_range"][0]] = count + 5
    if "history_empty" in special:
        hres["light"][special["history_empty"][1], special["history_empty"][0]] = S.RESTIR_EMPTY
    hkey = np.concatenate([planes[1][..., :3], planes[4][..., 1:2]], -1).astype(f32)
    far = rng.uniform(size=(H, W)) < 0.15
    hkey[..., 3] = np.where(far, hkey[..., 3] * f32(1.5), hkey[..., 3])          # a depth that fails the test
    vis = rng.uniform(size=(2, H, W))
    vis = np.where(vis < 0.3, 0.0, np.where(vis < 0.7, 1.0, vis)).astype(f32)
    out = dict(planes=tuple(planes), cb=cb, lights=lights(count, width, height), motion=motion, history=(hres, hkey), sun_radiance=c["sun_radiance"], sky=c["sky"], visibility=vis,
               special=special, miss=miss)
    for v in planes + [motion, hres, hkey, vis]:
        v.setflags(write=False)
    return out


def params(flags=0, seed=1, **kw):
    p = S.RestirParams(flags, seed)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# ---- the scene of the unbiasedness tests ------------------------------------------------------------------------------------------------
FLOOR_SIZE = (33, 25)
FLOOR_LIGHTS = 40


def floor_scene(luts):
    """A floor with three blockers under 40 point and spot lights (indices 0..39: the spots first, as the scene sorts them; the default sun
    follows at index 40 and is left out with m_LightCount = 40)."""
    from hobbyrenderer_amd import scenes
    rng = np.random.default_rng(41)
    b = scenes.SceneBuilder()
    quad, cube = b.add_mesh(*scenes.generate_floor_quad()), b.add_mesh(*scenes.generate_default_cube())
    grey = b.add_material(m_BaseColor=(0.7, 0.7, 0.7, 1))
    b.add_instance(quad, grey, scenes._mat((8, 1, 8)))
    for pos, size in (((-0.9, 0.35, 0.2), (0.5, 0.7, 0.5)), ((0.7, 0.25, -0.4), (0.6, 0.5, 0.4)), ((0.1, 0.5, 1.0), (0.4, 1.0, 0.4))):
        b.add_instance(cube, grey, scenes._mat(size, None, pos))
    for k in range(FLOOR_LIGHTS):
        pos = (rng.uniform(-2.0, 2.0), rng.uniform(0.8, 2.2), rng.uniform(-1.5, 2.0))
        color, intensity = tuple(rng.uniform(0.3, 1.0, 3)), float(rng.uniform(0.5, 4.0))
        if k % 4 == 0:
            b.add_light(S.LIGHT_SPOT, position=pos, direction=(rng.uniform(-0.4, 0.4), -1.0, rng.uniform(-0.4, 0.4)), color=color, intensity=2.0 * intensity, inner=0.3, outer=0.8)
        else:
            b.add_light(S.LIGHT_POINT, position=pos, color=color, intensity=intensity, range_=0.0 if k % 3 else 6.0)
    return b.finalize(luts)


def floor_constants(sc):
    """The camera of the unbiasedness tests: no jitter, m_LightCount = 40."""
    import math
    from hobbyrenderer_amd import scenes
    view, pos = scenes.planar_view(*FLOOR_SIZE, position=(0.0, 2.2, -3.2), pitch=math.radians(32.0))
    cb = scenes.fill_constants(view, pos, sc, 0, 1)
    cb["m_Jitter"] = (0.0, 0.0)
    cb["m_LightCount"] = FLOOR_LIGHTS
    return cb
