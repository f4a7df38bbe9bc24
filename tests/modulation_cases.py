"""Synthetic inputs of the demodulate / compose tests (tests/test_modulation_cpu.py, tests/test_modulation_gpu.py), built on
tests/denoise_cases.py: its planes (the far tilted plane with the near box, misses on two sides and isolated ones, roughness 0.04 / 0.5 / 1
in bands, metallic 0 / 0.5 / 1 per region) and its colour image, plus what these stages read: an albedo plane with a 2-texel checker whose
channels include exact 0 and 1, an emissive plane on about 5 % of the hits, some of it above the colour so that the clamp is exercised, and
a handful of pixels whose normal is exactly +-z or just either side of |N.z| = 0.999, the threshold of the tangent frame's `up` choice."""
import numpy as np

import denoise_cases as DC

F = np.float32
SIZES = [(37, 23), (64, 36), (1, 1), (2, 3)]
FLOORS = [0.04, 0.5, 1e-6]
CHECKER = ((1.0, 0.5, 0.0), (0.0, 0.25, 1.0))


def checker_albedo(w, h):
    """[H, W, 4]: squares of 2 x 2 texels alternating between the two CHECKER colours, alpha 1."""
    y, x = np.mgrid[0:h, 0:w]
    odd = (((x // 2) + (y // 2)) & 1).astype(bool)
    a = np.ones((h, w, 4), np.float32)
    a[..., :3] = np.where(odd[..., None], np.float32(CHECKER[1]), np.float32(CHECKER[0]))
    return a


def special_normals():
    out = [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0)]
    for z in (0.9989, 0.9991, -0.9989, -0.9991):
        s = float(np.sqrt(1.0 - z * z))
        out += [(s, 0.0, z), (0.0, -s, z)]
    return np.asarray(out, np.float32)


def case(w, h, seed=1):
    c = DC.case(w, h, seed)
    hit = c["hit"]
    rng = np.random.default_rng(seed + 30)
    albedo = checker_albedo(w, h)
    y, x = np.mgrid[0:h, 0:w]
    free = (x >= (3 * w) // 4) & (y < h // 4)                          # a corner of free albedo, some of it dark (the floor's business on metals)
    albedo[free, :3] = (rng.random((h, w, 3)).astype(np.float32) ** 3)[free]
    albedo[~hit] = 0.0

    normal, geo = c["normal"].copy(), c["geo"].copy()
    special = special_normals()
    where = np.argwhere(hit)
    count = min(len(special), len(where) // 2)
    picks = where[np.linspace(0, len(where) - 1, count).astype(int)] if count else np.zeros((0, 2), int)
    for (py, px), n in zip(picks, special):
        normal[py, px, :3] = n
        geo[py, px, :3] = n

    color = c["color"].copy()
    emissive = np.zeros((h, w, 4), np.float32)
    lit = hit & (rng.random((h, w)) < 0.05)
    if w * h > 1 and not lit.any():
        lit[tuple(where[-1])] = True
    scale = rng.uniform(0.2, 1.5, (h, w, 3)).astype(np.float32)           # above 1: emissive exceeds the colour, the clamp bites
    emissive[lit, :3] = (color[..., :3] * scale)[lit]
    emissive[hit, 3] = 1.0
    return dict(color=color, albedo=albedo, normal=normal, geo=geo, depth=c["depth"], emissive=emissive, hit=hit, lit=lit, view=c["view"],
                special=picks)


def textured_plane(w=64, h=36, seed=5):
    """The experiment the stages exist for: DC.flat_plane at age 0 (a non-metal, i.i.d. signal in [0.5, 1.5]) under the checker albedo. The
    caller multiplies the signal by the factor of this case to get the radiance a path tracer would hand over."""
    c = DC.flat_plane(w, h, seed, age=0.0)
    c["albedo"] = checker_albedo(w, h)
    c["signal"] = c["input"][..., :3].copy()
    return c
