"""Synthetic inputs of the denoise-stage tests (tests/test_denoise_cpu.py, tests/test_denoise_gpu.py), built on tests/temporal_cases.py: its
far tilted plane with the near box, the border of misses on two sides and the isolated ones; roughness and metallic varied per region (the
geo-normal plane carries metallic in .w); an input image of seeded radiance with 1 % fireflies and ages 0-300, so that both the clamp at 64
and the 0.15 floor of the age falloff are hit; a caller noise tile; and the two analytic scenes of the property tests."""
import numpy as np

from hobbyrenderer_amd import structs as S
import temporal_cases as TC

F = np.float32
SIZES = TC.SIZES
FRAMES = [0, 1, 4095, 4096, 0xFFFFFFFF]
RADII = [0.5, 3.0, 12.0]


def view(w, h):
    return TC.views(w, h, False)[0]


def caller_tile(seed=7):
    return np.random.default_rng(seed).random((64, 64, 2), np.float32)


def case(w, h, seed=1):
    depth, normal, hit = TC.planes(w, h, seed)
    y, x = np.mgrid[0:h, 0:w]
    # roughness: three vertical bands (0.04, 0.5, 1) with a little per-pixel variation inside the middle one; metallic: top half 0, bottom half 1,
    # and 0.5 on the box
    rough = np.where(x < w // 4, 0.04, np.where(x < (3 * w) // 4, 0.5, 1.0)).astype(np.float32)
    rough += (np.random.default_rng(seed + 5).random((h, w)) * 0.02).astype(np.float32) * (rough == F(0.5))
    normal[..., 3] = rough
    geo = normal.copy()
    metal = np.where(y < h // 2, 0.0, 1.0).astype(np.float32)
    box = (x >= w // 3) & (x < (2 * w) // 3) & (y >= h // 3) & (y < (2 * h) // 3)
    metal[box] = 0.5
    geo[..., 3] = metal
    normal[~hit] = 0.0
    geo[~hit] = 0.0
    inp = TC.radiance(w, h, seed + 10)
    rng = np.random.default_rng(seed + 11)
    age = rng.uniform(0.0, 300.0, (h, w)).astype(np.float32)
    age[rng.random((h, w)) < 0.3] = 0.0                      # fresh pixels: disocclusions, a camera cut
    inp[..., 3] = age
    color = TC.radiance(w, h, seed + 12)
    color[..., 3] = np.random.default_rng(seed + 13).random((h, w)).astype(np.float32)
    return dict(input=inp, depth=depth, normal=normal, geo=geo, hit=hit, view=view(w, h), color=color)


def params(radius=3.0, frame=0, iterations=1, flags=0, **kw):
    return S.DenoiseParams(radius=radius, frame=frame, iterations=iterations, flags=flags, **kw)


def flat_plane(w, h, seed, age=0.0):
    """A fronto-parallel plane at view depth 6 filling the image, normal towards the camera of views(), constant roughness and metallic, i.i.d.
    radiance, one age."""
    v = view(w, h)
    depth = np.zeros((h, w, 4), np.float32)
    depth[..., 0] = 6.06; depth[..., 1] = 6.0
    normal = np.zeros((h, w, 4), np.float32)
    normal[..., :3] = plane_normal(v)
    normal[..., 3] = 0.5
    geo = normal.copy(); geo[..., 3] = 0.0
    inp = np.ones((h, w, 4), np.float32)
    inp[..., :3] = np.random.default_rng(seed).uniform(0.5, 1.5, (h, w, 3)).astype(np.float32)
    inp[..., 3] = age
    return dict(input=inp, depth=depth, normal=normal, geo=geo, view=v)


def plane_normal(v):
    """Unit normal of the surfaces of constant view depth, facing the camera: minus the view direction, from the view's own matrices."""
    m = np.asarray(v["m_MatClipToWorld"], np.float64)

    def world(z):
        hpos = np.array([0.0, 0.0, z, 1.0]) @ m
        return hpos[:3] / hpos[3]
    d = world(0.02) - world(0.05)                              # reversed Z: the smaller z is the farther point
    return (-d / np.linalg.norm(d)).astype(np.float32)


def two_half_planes(w, h):
    """Two half-planes at one view depth whose normals differ by 90 degrees (left: n, right: a unit vector perpendicular to n), radiance 0.1 on the
    left and 10 on the right, age 64, with a border of misses."""
    c = flat_plane(w, h, 3, age=64.0)
    n = c["normal"][0, 0, :3].astype(np.float64)
    t = np.cross(n, (0.0, 1.0, 0.0)); t /= np.linalg.norm(t)
    right = np.zeros((h, w), bool); right[:, w // 2:] = True
    c["normal"][right, :3] = t.astype(np.float32)
    c["geo"][..., :3] = c["normal"][..., :3]
    c["input"][..., :3] = 0.1
    c["input"][right, :3] = 10.0
    hit = np.ones((h, w), bool)
    hit[:1] = hit[-1:] = False; hit[:, :1] = hit[:, -1:] = False
    c["depth"][~hit] = (1e10, 1e10, 0.0, 0.0)
    c["hit"], c["dark"] = hit, hit & ~right
    return c
