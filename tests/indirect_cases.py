"""Synthetic planes for the traced-indirect-lighting tests (test_indirect_cpu.py, test_indirect_gpu.py) -- TEST INFRASTRUCTURE.

A case is four float32 [H, W, 4] planes as hrpt_render_gbuffer would leave them (unit normals over the whole sphere, roughness in [0.04, 1],
metallic exactly 0 on a third of the pixels and exactly 1 on another third, t in [2, 6], a fifth of the pixels missed), constants with a
jitter that is no Halton point, a colour image, and random radiance with w in {0, 1} for both lobes. Five pixels are edited so that the
branches no camera produces reliably are in frame (SPECIAL): a normal equal to the primary-ray direction (N == -V: facing away exactly), a
unit normal with dot(N, V) == 0 exactly in binary32, a base colour of 0 on a metal, and normals along +z and -z (the other branch of
tangent_frame)."""
import functools

import numpy as np

from hobbyrenderer_amd import scenes, structs as S
import indirect_reference as R

f32 = np.float32
SIZES = [(1, 1), (33, 9), (61, 37)]
SPECIAL = {"facing_away": (5, 3), "grazing": (12, 4), "black_metal": (20, 6), "plus_z": (27, 2), "minus_z": (30, 7)}      # (x, y) at sizes that hold them
LOBES = [S.INDIRECT_DIFFUSE, S.INDIRECT_SPECULAR, S.INDIRECT_DIFFUSE | S.INDIRECT_SPECULAR]


def constants(width, height):
    view, pos = scenes.planar_view(width, height, position=(0.0, 0.0, -5.0))
    cb = np.zeros((), S.PathTracerConstants)
    cb["m_View"] = view
    cb["m_CameraPos"] = (pos[0], pos[1], pos[2], 1.0)
    cb["m_MaxBounces"] = 2
    cb["m_Jitter"] = (0.25, -0.125)
    cb["m_SunDirection"] = (0.0, 1.0, 0.0)
    cb["m_CosSunAngularRadius"] = 1.0
    return cb


def _perpendicular_unit(v, rng):
    """A float32 vector n, unit to rounding, whose binary32 dot product with v, summed left to right, is exactly 0."""
    for _ in range(4000):
        a = rng.normal(size=3)
        n = np.cross(v.astype(np.float64), a)
        n = (n / np.linalg.norm(n)).astype(f32)
        if R._dot(n, v) == 0:
            return n
    raise AssertionError("no exactly perpendicular float32 normal found")


@functools.lru_cache(maxsize=None)
def case(width, height, seed=23):
    """dict: planes (albedo, normal, geo_normal, depth), cb, color, radiance [2, H, W, 4], special, miss. Read-only: shared between tests."""
    rng = np.random.default_rng(seed + 1000 * width + height)
    H, W = height, width
    n = rng.normal(size=(H, W, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    albedo = rng.uniform(0.0, 1.0, (H, W, 4)).astype(f32)
    normal = np.concatenate([n, rng.uniform(0.04, 1.0, (H, W, 1))], -1).astype(f32)
    pick = rng.uniform(size=(H, W))
    metal = np.where(pick < 1 / 3, 0.0, np.where(pick < 2 / 3, 1.0, rng.uniform(size=(H, W))))
    t = rng.uniform(2.0, 6.0, (H, W)).astype(f32)
    miss = rng.uniform(size=(H, W)) < 0.2
    special = {k: p for k, p in SPECIAL.items() if p[0] < W and p[1] < H}
    for x, y in special.values():
        miss[y, x] = False
    if W * H == 1:
        miss[:] = False
    t[miss] = R.MISS
    depth = np.zeros((H, W, 4), f32)
    depth[..., 0], depth[..., 1] = t, t
    cb = constants(W, H)
    _, d, _ = R.primary_rays(cb, W, H)
    if "facing_away" in special:
        x, y = special["facing_away"]
        normal[y, x, :3] = d[y, x]                                    # N == d == -V
    if "grazing" in special:
        x, y = special["grazing"]
        normal[y, x, :3] = _perpendicular_unit(-d[y, x], rng)
        metal[y, x] = 0.0                                            # the diffuse record is traced, the specular one is not
    if "black_metal" in special:
        x, y = special["black_metal"]
        albedo[y, x, :3] = 0.0
        metal[y, x] = 1.0
        normal[y, x, :3] = -d[y, x]                                   # faces the camera: F0 == 0 is what culls
    if "plus_z" in special:
        x, y = special["plus_z"]
        normal[y, x, :3] = (0.0, 0.0, 1.0)
    if "minus_z" in special:
        x, y = special["minus_z"]
        normal[y, x, :3] = (0.0, 0.0, -1.0)                           # faces the camera
        metal[y, x] = 0.5
    geo = np.concatenate([normal[..., :3], metal[..., None]], -1).astype(f32)
    color = rng.uniform(0.0, 2.0, (H, W, 4)).astype(f32)
    radiance = rng.uniform(0.0, 3.0, (2, H, W, 4)).astype(f32)
    radiance[..., 3] = np.where(rng.uniform(size=(2, H, W)) < 0.7, 1.0, 0.0)
    out = dict(planes=(albedo, normal, geo, depth), cb=cb, color=color, radiance=radiance, special=special, miss=miss)
    for v in out["planes"] + (color, radiance):
        v.setflags(write=False)
    return out


def radiance_for(c, flags):
    """The radiance records of a call with `flags`: [lobes, H, W, 4], diffuse first."""
    pick = [k for k, bit in enumerate((S.INDIRECT_DIFFUSE, S.INDIRECT_SPECULAR)) if flags & bit]
    return np.ascontiguousarray(c["radiance"][pick])
