"""Synthetic inputs of the probe-volume tests (tests/test_probes_cpu.py, tests/test_probes_gpu.py): the three grids, traced-ray arrays in the
layout hrpt_trace_radiance / hrpt_trace_rays leave them (random radiance, misses, untraced rays at positions 0, 63, 64 and last, one probe
whose rays are all untraced), atlases to blend into, and query points on probes, between them, outside the volume and non-finite. The
reference result of a case is computed once and shared by every test that asks for it."""
import functools

import numpy as np

from hobbyrenderer_amd import native, structs as S
import probes_reference as R

F = np.float32
GRIDS = [(1, 1, 1), (3, 2, 2), (2, 1, 5)]
RAY_COUNTS = [1, 32, 100, 1024]
SEEDS = [0, 7, 0xDEADBEEF]
# (grid, rays per probe, hysteresis, exponent, with history): every ray count, both hysteresis values and exponents, with and without history
BLEND_CASES = [((3, 2, 2), 100, 0.97, 50.0, True), ((3, 2, 2), 100, 0.0, 1.0, True), ((3, 2, 2), 100, 0.97, 1.0, False), ((2, 1, 5), 32, 0.0, 50.0, False),
               ((1, 1, 1), 1, 0.97, 50.0, True), ((1, 1, 1), 1024, 0.97, 50.0, True), ((2, 1, 5), 257, 0.5, 8.0, True)]


def grid_id(g):
    return "x".join(str(c) for c in g)


def blend_id(c):
    return f"{grid_id(c[0])}-n{c[1]}-h{c[2]}-e{c[3]}-{'history' if c[4] else 'first'}"


def volume(grid, rays=100, hysteresis=0.97, exponent=50.0, max_distance=3.0, normal_bias=0.05, view_bias=0.02):
    return native.probe_volume((-1.25, 0.5, -2.0), (1.0, 0.75, 1.5), grid, rays, hysteresis=hysteresis, max_ray_distance=max_distance,
                               distance_exponent=exponent, normal_bias=normal_bias, view_bias=view_bias)


def traced(vol, seed=1):
    """(radiance [P * N, 4], hits [P * N]) as the two trace calls would leave them."""
    rng = np.random.default_rng(seed)
    n, P = int(vol["raysPerProbe"]), R.probe_count(vol)
    rad = np.concatenate([rng.uniform(0.0, 4.0, (P, n, 3)), np.ones((P, n, 1))], -1).astype(np.float32)
    for k in (0, 63, 64, n - 1):
        if k < n and P > 1:
            rad[0, k] = 0.0                       # untraced: (0, 0, 0, 0)
    if P > 2:
        rad[2] = 0.0                              # a probe without a traced ray keeps its old texels
    hits = np.zeros((P, n), S.RayHit)
    hits["hit"] = rng.random((P, n)) < 0.8
    hits["t"] = rng.uniform(0.05, 6.0, (P, n)).astype(np.float32)            # beyond maxRayDistance = 3 as well: clamped
    hits["t"][hits["hit"] == 0] = 0.0
    return rad.reshape(P * n, 4), hits.reshape(P * n)


def atlases(vol, seed=3):
    """Plausible atlases with correct borders: irradiance [P, 8, 8, 4] and distance [P, 16, 16, 2] with mean d^2 >= (mean d)^2."""
    rng = np.random.default_rng(seed)
    P = R.probe_count(vol)
    irr = np.concatenate([rng.uniform(0.0, 2.0, (P, 8, 8, 3)), np.ones((P, 8, 8, 1))], -1).astype(np.float32)
    d = rng.uniform(0.2, 3.0, (P, 16, 16)).astype(np.float32)
    dist = np.stack([d, d * d * rng.uniform(1.0, 1.5, (P, 16, 16)).astype(np.float32)], -1).astype(np.float32)
    return R.fill_border(irr), R.fill_border(dist)


@functools.lru_cache(maxsize=None)
def blend_case(case):
    grid, n, hysteresis, exponent, history = case
    vol = volume(grid, n, hysteresis, exponent)
    _, dirs = R.rays(vol, 11, S.Ray)
    rad, hits = traced(vol)
    irr, dist = atlases(vol)
    c = dict(vol=vol, dirs=dirs, radiance=rad, hits=hits, irradiance=irr, distance=dist, history=history)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def blend_reference(case):
    c = blend_case(case)
    out = R.blend(c["vol"], c["dirs"], c["radiance"], c["hits"], c["irradiance"], c["distance"], c["history"])
    for a in out:
        a.setflags(write=False)
    return out


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def points(vol, count=4096, seed=5, hostile=True):
    """S.ProbePoint records: random points in and around the volume, points exactly on probes, points far outside, and (hostile) records
    with a NaN or an infinity in each of the nine coordinates."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(vol["counts"], np.float64)
    o, sp = np.asarray(vol["origin"], np.float64), np.asarray(vol["spacing"], np.float64)
    extent = np.maximum(counts - 1, 0) * sp
    pos = o - 0.6 * sp + rng.random((count, 3)) * (extent + 1.2 * sp)
    on = R.probe_positions(vol)
    pos[:len(on)] = on                                                        # on probes: probePos - X == 0
    pos[len(on):len(on) + 16] = o + extent + sp * rng.uniform(3.0, 50.0, (16, 3))       # far outside
    pts = native.probe_points(pos.astype(np.float32), unit(rng.normal(size=(count, 3))), unit(rng.normal(size=(count, 3))))
    if hostile:
        raw = pts.view(np.float32).reshape(count, 12)
        for j, col in enumerate((0, 1, 2, 4, 5, 6, 8, 9, 10)):
            raw[count - 1 - 2 * j, col] = np.nan
            raw[count - 2 - 2 * j, col] = np.inf if j % 2 else -np.inf
    return pts


@functools.lru_cache(maxsize=None)
def query_case(grid):
    vol = volume(grid)
    irr, dist = atlases(vol)
    pts = points(vol)
    ref = R.query(vol, irr, dist, pts)
    for a in (irr, dist, pts, ref):
        a.setflags(write=False)
    return dict(vol=vol, irradiance=irr, distance=dist, points=pts, reference=ref)
