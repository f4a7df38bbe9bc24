"""The irradiance probe volume without a GPU: the host executors hrpt_probes_rays_host / _blend_host / _query_host
against the NumPy statement of tests/probes_reference.py, bit for bit; the properties the definition promises (unit directions, the border
rule and what it buys, constant atlases, the inactive visibility term); the statement against its float64 formulation; thread-count
invariance; the argument errors; and the sanitizer build of the host side (`make probes_asan`, a stand-alone program)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hobbyrenderer_amd import native, structs as S
import probes_cases as PC
import probes_reference as R
from test_temporal_cpu import u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hobbyrenderer_amd", "csrc")
SYMBOLS = ("hrpt_probes_create", "hrpt_probes_destroy", "hrpt_probes_update", "hrpt_probes_query", "hrpt_probes_shade_gbuffer", "hrpt_read_probe_irradiance",
           "hrpt_get_probe_irradiance_device", "hrpt_probes_read", "hrpt_probes_get_device", "hrpt_probes_write", "hrpt_probes_rays_host",
           "hrpt_probes_blend_host", "hrpt_probes_blend_device", "hrpt_probes_query_host")
GRIDS = pytest.mark.parametrize("grid", PC.GRIDS, ids=PC.grid_id)
EPS = 2.0 ** -24
# Largest deviation of the float32 statement from the float64 formulation on the cases of this file, measured here and recorded in DESIGN.md
# section 26 (relative to the largest value of the texel / the result): the tests hold the statement to four times these.
MEASURED_DISTANCE_BLEND = 1.14e-6
MEASURED_QUERY = 3.05e-6


def same_bytes(got, want, what):
    a, b = u32(got), u32(want)
    if not np.array_equal(a, b):
        i = np.argwhere(a != b)[0]
        raise AssertionError(f"{what}: {int((a != b).sum())} of {a.size} words differ, first at {tuple(i)}: {got[tuple(i)]} != {want[tuple(i)]}")


def host_blend(c, nthreads=3):
    return native.probes_blend_host(c["vol"], c["dirs"], c["radiance"], c["hits"], c["irradiance"], c["distance"], c["history"], nthreads)


def test_symbols_are_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "hobbyrt_pt.h")).read()
    for name in SYMBOLS:
        assert name in native.EXPORTS and hasattr(native.lib, name) and f" {name}(" in header, name
    assert "#define HRPT_ABI_VERSION 3" in header and S.ABI_VERSION == 3
    assert S.ProbeVolume.itemsize == 64 and S.ProbePoint.itemsize == 48 and (S.PROBES_RESET, S.PROBES_DEVICE_POINTERS) == (1, 0x100)
    fields = {k: S.ProbeVolume.fields[k][1] for k in S.ProbeVolume.names}      # that the C header says the same: test_binding_contract.py
    assert (fields["counts"], fields["distanceExponent"], fields["pad"], S.ProbePoint.fields["view"][1]) == (32, 48, 60, 32)


# ---------------------------------------------------------------- 1. rays
@GRIDS
@pytest.mark.parametrize("n", PC.RAY_COUNTS)
def test_rays_host_equals_reference(grid, n):
    vol = PC.volume(grid, n)
    for seed in PC.SEEDS:
        rays, dirs = native.probes_rays_host(vol, seed)
        ref_rays, ref_dirs = R.rays(vol, seed, S.Ray)
        assert rays.tobytes() == ref_rays.tobytes() and dirs.tobytes() == ref_dirs.tobytes(), seed
        assert (rays["tmin"] == 0).all() and (rays["tmax"] == np.float32(1e10)).all() and (rays["pad"] == 0).all()


def test_directions_are_unit_vectors_and_the_rotation_is_orthonormal():
    for seed in PC.SEEDS + [1, 2, 3, 0xFFFFFFFF]:
        Rm = R.rotation(seed).astype(np.float64)
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(Rm) - 1.0) <= 1e-6, seed
        for n in PC.RAY_COUNTS:
            _, dirs = native.probes_rays_host(PC.volume((1, 1, 1), n), seed)
            length = np.linalg.norm(dirs[:, :3].astype(np.float64), axis=1)
            assert np.abs(length - 1.0).max() <= 2 * 2.0 ** -23, (seed, n)            # 2 ulp of 1
    _, a = native.probes_rays_host(PC.volume((1, 1, 1), 100), 1)
    _, b = native.probes_rays_host(PC.volume((1, 1, 1), 100), 2)
    assert not np.array_equal(a, b)                                                     # the seed turns the set
    d = a[:, :3].astype(np.float64)
    assert np.abs(d.mean(0)).max() < 0.02                                               # ... which covers the sphere evenly


# ---------------------------------------------------------------- 2. blend
@pytest.mark.parametrize("case", PC.BLEND_CASES, ids=PC.blend_id)
def test_blend_host_equals_reference(case):
    got, ref = host_blend(PC.blend_case(case)), PC.blend_reference(case)
    same_bytes(got[0], ref[0], "irradiance")
    same_bytes(got[1], ref[1], "distance")


def test_the_blend_cases_do_what_they_are_there_for():
    case = PC.BLEND_CASES[0]
    c, (irr, dist) = PC.blend_case(case), PC.blend_reference(case)
    n = int(c["vol"]["raysPerProbe"])
    rad, hits = c["radiance"].reshape(-1, n, 4), c["hits"].reshape(-1, n)
    assert (rad[0, [0, 63, 64, n - 1], 3] == 0).all() and (rad[0, 1:63, 3] == 1).all() and (rad[2, :, 3] == 0).all()
    assert (hits["hit"] == 0).any() and (hits["t"] > c["vol"]["maxRayDistance"]).any()
    same_bytes(irr[2], c["irradiance"][2], "a probe without a traced ray keeps its irradiance")
    same_bytes(dist[2], c["distance"][2], "... and its distances")
    assert not np.array_equal(irr[1], c["irradiance"][1]) and (irr[[0, 1] + list(range(3, 12)), 1:-1, 1:-1, 3] == 1).all()
    assert (dist[[0, 1], 1:-1, 1:-1, 0] <= c["vol"]["maxRayDistance"]).all()
    # the untraced rays take no part: giving them radiance and a hit changes nothing
    rad2, hits2 = c["radiance"].copy().reshape(-1, n, 4), c["hits"].copy().reshape(-1, n)
    rad2[0, [0, 63, 64, n - 1], :3] = 1000.0
    hits2["t"][0, [0, 63, 64, n - 1]] = 0.001
    got = native.probes_blend_host(c["vol"], c["dirs"], rad2.reshape(-1, 4), hits2.reshape(-1), c["irradiance"], c["distance"], True)
    same_bytes(got[0], irr, "irradiance"); same_bytes(got[1], dist, "distance")
    # history: hysteresis 0 stores the new value whatever the atlas held; without history the hysteresis is not read
    first = list(case); first[4] = False
    zero = list(case); zero[2] = 0.0
    a, b = PC.blend_reference(tuple(first)), PC.blend_reference(tuple(zero))
    keep = [0, 1] + list(range(3, 12))
    same_bytes(a[0][keep], b[0][keep], "irradiance"); same_bytes(a[1][keep], b[1][keep], "distance")


@pytest.mark.parametrize("case", PC.BLEND_CASES[:2] + PC.BLEND_CASES[4:5], ids=PC.blend_id)
def test_every_border_texel_is_the_byte_copy_of_its_source(case):
    for tiles in host_blend(PC.blend_case(case)):
        T = tiles.shape[1]
        for y in range(T):
            for x in range(T):
                sx, sy = R.border_source(x, y, T)
                assert 1 <= sx <= T - 2 and 1 <= sy <= T - 2
                assert np.array_equal(u32(tiles[:, y, x]), u32(tiles[:, sy, sx])), (x, y)


def lookup_error(interior, border):
    """Largest error of the bilinear lookup of a tile filled from f(d) = d.x, over 200 000 random directions, in float64 up to the lookup."""
    rng = np.random.default_rng(0)
    d = rng.normal(size=(200000, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    tiles = np.zeros((1, interior + 2, interior + 2, 1), np.float32)
    tiles[0, 1:-1, 1:-1, 0] = R.texel_directions(interior)[:, 0].reshape(interior, interior)
    got = R.lookup(border(tiles), np.zeros(len(d), np.int64), d, interior)[:, 0]
    return float(np.abs(got.astype(np.float64) - d[:, 0]).max())


def test_the_border_rule_keeps_the_lookup_accurate():
    """Section 26: with the border rule a bilinear lookup of a tile filled from a smooth function of direction (here d.x, amplitude 1) is
    within 0.05 at I = 14; a clamped border is worse than 0.08. Measured here: 0.048 (I = 14) and 0.095 (I = 6) with the rule, 0.108
    (I = 14) clamped."""
    rule14, rule6, clamped14 = lookup_error(14, R.fill_border), lookup_error(6, R.fill_border), lookup_error(14, R.clamp_border)
    print("lookup error: rule I=14", rule14, "rule I=6", rule6, "clamped I=14", clamped14)
    assert rule14 <= 0.05 and clamped14 > 0.08 and rule6 <= 0.1


# ---------------------------------------------------------------- 3. query
@GRIDS
def test_query_host_equals_reference(grid):
    q = PC.query_case(grid)
    got = native.probes_query_host(q["vol"], q["irradiance"], q["distance"], q["points"], 3)
    same_bytes(got, q["reference"], "query")
    P = R.probe_count(q["vol"])
    assert (got[P:P + 16] != 0).any(-1).all() and (got[P:P + 16, 3] == 0).all()          # far outside: the clamped answer, inside = 0
    assert (got[-18:] == 0).all() and np.isfinite(got).all()                             # non-finite records answer (0, 0, 0, 0)
    if grid == (3, 2, 2):
        assert 100 < (got[:, 3] == 1).sum() < 4000                                       # points inside and outside the box


@GRIDS
def test_a_point_on_a_probe_without_bias_is_inside_and_finite(grid):
    vol = PC.volume(grid, normal_bias=0.0, view_bias=0.0)
    irr, dist = PC.atlases(vol)
    pos = R.probe_positions(vol)
    pts = native.probe_points(pos, PC.unit(np.ones((len(pos), 3))), PC.unit(np.ones((len(pos), 3)) * [1, -1, 1]))
    got = native.probes_query_host(vol, irr, dist, pts)
    same_bytes(got, R.query(vol, irr, dist, pts), "query")
    assert (got[:, 3] == 1).all() and np.isfinite(got).all() and (got[:, :3] > 0).all()


@GRIDS
def test_constant_atlases_give_pi_times_the_constant(grid):
    """(sum w M) / (sum w) * pi with every lookup returning M: under 32 roundings of 2^-24 each (a constant bilinear lookup 6, eight
    products and sums 16, the quotient and the factor pi 2), whatever the weights are."""
    vol = PC.volume(grid)
    P = R.probe_count(vol)
    M = np.array([0.25, 1.5, 3.0], np.float32)
    irr = np.ones((P, 8, 8, 4), np.float32); irr[..., :3] = M
    dist = np.zeros((P, 16, 16, 2), np.float32); dist[..., 0] = 0.4; dist[..., 1] = 0.2       # short distances: the visibility term is active
    pts = PC.points(vol, 1024, hostile=False)
    got = native.probes_query_host(vol, irr, dist, pts)
    want = np.pi * M.astype(np.float64)
    assert np.abs(got[:, :3] / want - 1.0).max() <= 32 * EPS


@GRIDS
def test_visibility_is_inactive_at_the_maximum_ray_distance(grid):
    """Distances at maxRayDistance (what an update in empty space stores) with every point nearer than that to its probes: dl > m never
    holds, and the result equals the statement with the term removed."""
    vol = PC.volume(grid, max_distance=1000.0)
    irr, _ = PC.atlases(vol)
    dist = np.zeros((R.probe_count(vol), 16, 16, 2), np.float32); dist[..., 0] = 1000.0; dist[..., 1] = 1000.0 * 1000.0
    pts = PC.points(vol, 2048, hostile=False)
    got = native.probes_query_host(vol, irr, dist, pts)
    same_bytes(got, R.query(vol, irr, dist, pts, visibility=False), "query without the visibility term")
    near = np.zeros_like(dist); near[..., 0] = 0.01; near[..., 1] = 0.0001
    assert not np.array_equal(native.probes_query_host(vol, irr, near, pts), got)        # ... and the term does act where a probe sees less far


# ---------------------------------------------------------------- 4. the statement against float64
@pytest.mark.parametrize("case", PC.BLEND_CASES, ids=PC.blend_id)
def test_blend_statement_against_float64(case):
    """Irradiance: sequential summation of non-negative terms, relative error (N - 1 + 2) u per sum, doubled for the quotient of two such
    sums and with the weight's own three roundings: 4 (N + 8) 2^-24 of the largest channel value. Distance: hrt_pow dominates; four times
    the measured deviation. With history the new value enters with the factor 1 - hysteresis and three more roundings, inside the same bounds."""
    c = PC.blend_case(case)
    irr, dist = PC.blend_reference(case)
    irr64, dist64 = R.blend64(c["vol"], c["dirs"], c["radiance"], c["hits"], c["irradiance"], c["distance"], c["history"])
    n, P = int(c["vol"]["raysPerProbe"]), R.probe_count(c["vol"])
    live = np.isfinite(irr64).all(-1)
    got = irr[:, 1:-1, 1:-1, :3].reshape(P, 36, 3).astype(np.float64)
    dev = np.abs(got - irr64)[live].max() / 4.0                                       # radiance is drawn from [0, 4)
    print("irradiance blend: relative deviation", dev, "bound", 4 * (n + 8) * EPS)
    assert dev <= 4 * (n + 8) * EPS
    live = np.isfinite(dist64).all(-1)
    got = dist[:, 1:-1, 1:-1].reshape(P, 196, 2).astype(np.float64)
    scale = np.array([3.0, 9.0])                                                      # maxRayDistance and its square
    dev = (np.abs(got - dist64) / scale)[live].max()
    print("distance blend: relative deviation", dev)
    assert dev <= 4 * MEASURED_DISTANCE_BLEND


@GRIDS
def test_query_statement_against_float64(grid):
    q = PC.query_case(grid)
    finite = np.isfinite(q["points"].view(np.float32).reshape(-1, 12)).all(-1)
    want = R.query64(q["vol"], q["irradiance"], q["distance"], q["points"][finite])
    dev = np.abs(q["reference"][finite, :3].astype(np.float64) - want).max() / (np.pi * 2.0)      # the atlases hold values in [0, 2)
    print("query: relative deviation", dev)
    assert dev <= 4 * MEASURED_QUERY


# ---------------------------------------------------------------- 5. threads, errors, sanitizers
def test_thread_count_invariance():
    c = PC.blend_case(PC.BLEND_CASES[0])
    one = host_blend(c, 1)
    q = PC.query_case((3, 2, 2))
    for n in (2, 3, 7, 0, -1, 1000):
        got = host_blend(c, n)
        assert np.array_equal(u32(got[0]), u32(one[0])) and np.array_equal(u32(got[1]), u32(one[1])), n
        same_bytes(native.probes_query_host(q["vol"], q["irradiance"], q["distance"], q["points"], n), q["reference"], f"query with {n} threads")


def test_argument_errors():
    lib = native.lib
    err = lambda: lib.hrpt_last_error(None).decode()          # noqa: E731
    c = PC.blend_case(PC.BLEND_CASES[0])
    good = c["vol"]
    RULE = (": counts >= 1 with at most 2^20 probes, raysPerProbe 1..1024, spacing and maxRayDistance finite and > 0, hysteresis in [0, 1), "
            "distanceExponent finite and >= 1, normalBias and viewBias finite and >= 0, pad 0")
    nan, inf = float("nan"), float("inf")
    bad = [("counts", (0, 1, 1)), ("counts", (1024, 1024, 2)), ("counts", (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)), ("counts", (1 << 20, 2, 1)), ("raysPerProbe", 0), ("raysPerProbe", 1025),
           ("spacing", (0.0, 1.0, 1.0)), ("spacing", (1.0, -1.0, 1.0)), ("spacing", (1.0, 1.0, nan)), ("spacing", (inf, 1.0, 1.0)), ("origin", (nan, 0.0, 0.0)), ("origin", (0.0, inf, 0.0)),
           ("maxRayDistance", 0.0), ("maxRayDistance", inf), ("maxRayDistance", nan), ("hysteresis", 1.0), ("hysteresis", -0.1), ("hysteresis", nan),
           ("distanceExponent", 0.5), ("distanceExponent", nan), ("distanceExponent", inf), ("normalBias", -1.0), ("normalBias", nan), ("viewBias", -1.0), ("viewBias", inf), ("pad", 1)]
    rays, dirs = np.zeros(1200, S.Ray), np.full((100, 4), 7.0, np.float32)
    rays.view(np.uint8)[:] = 7
    irr, dist = c["irradiance"].copy(), c["distance"].copy()
    pts, out = PC.points(good, 64)[:16].copy(), np.full((16, 4), 7.0, np.float32)
    for key, value in bad:
        v = good.copy(); v[key] = value
        assert lib.hrpt_probes_rays_host(v.ctypes.data, 1, rays.ctypes.data, dirs.ctypes.data) == -1 and err() == "hrpt_probes_rays_host" + RULE, (key, value)
        assert lib.hrpt_probes_blend_host(v.ctypes.data, c["dirs"].ctypes.data, c["radiance"].ctypes.data, c["hits"].ctypes.data, irr.ctypes.data, dist.ctypes.data, 1, 1) == -1
        assert err() == "hrpt_probes_blend_host" + RULE, (key, value)
        assert lib.hrpt_probes_query_host(v.ctypes.data, irr.ctypes.data, dist.ctypes.data, pts.ctypes.data, out.ctypes.data, 16, 1) == -1 and err() == "hrpt_probes_query_host" + RULE
    for v in (native.probe_volume((0, 0, 0), (1, 1, 1), (1 << 20, 1, 1), 1, hysteresis=0.0, distance_exponent=1.0),):        # the limits are inclusive
        assert lib.hrpt_probes_rays_host(v.ctypes.data, 1, None, np.zeros((1, 4), np.float32).ctypes.data) == 0
    assert lib.hrpt_probes_rays_host(None, 1, rays.ctypes.data, dirs.ctypes.data) == -1 and err() == "hrpt_probes_rays_host: null volume"
    ptrs = [c["dirs"].ctypes.data, c["radiance"].ctypes.data, c["hits"].ctypes.data, irr.ctypes.data, dist.ctypes.data]
    for k in range(5):
        p = list(ptrs); p[k] = None
        assert lib.hrpt_probes_blend_host(good.ctypes.data, *p, 1, 1) == -1 and err() == "hrpt_probes_blend_host: null array", k
    assert lib.hrpt_probes_blend_host(good.ctypes.data, *ptrs, 2, 1) == -1 and err() == "hrpt_probes_blend_host: hasHistory must be 0 or 1"
    qp = [irr.ctypes.data, dist.ctypes.data, pts.ctypes.data, out.ctypes.data]
    for k in range(4):
        p = list(qp); p[k] = None
        assert lib.hrpt_probes_query_host(good.ctypes.data, *p, 16, 1) == -1 and err() == "hrpt_probes_query_host: null array", k
    assert lib.hrpt_probes_query_host(good.ctypes.data, None, None, None, None, 0, 1) == 0                 # nothing to do
    # an error changes nothing
    assert (rays.view(np.uint8) == 7).all() and (dirs == 7.0).all() and (out == 7.0).all()
    assert np.array_equal(irr, c["irradiance"]) and np.array_equal(dist, c["distance"])
    # context and object calls on NULL
    assert lib.hrpt_probes_create(None, good.ctypes.data, None) == -1
    assert lib.hrpt_probes_update(None, None, 0, 0) == -1 and lib.hrpt_probes_query(None, None, None, 0, 0) == -1
    assert lib.hrpt_probes_shade_gbuffer(None, None, 1.0) == -1 and lib.hrpt_read_probe_irradiance(None, None, 0) == -1
    assert lib.hrpt_get_probe_irradiance_device(None, None) == -1 and lib.hrpt_probes_read(None, None, 0, None, 0) == -1
    assert lib.hrpt_probes_write(None, None, 0, None, 0) == -1 and lib.hrpt_probes_get_device(None, None, None) == -1
    assert lib.hrpt_probes_blend_device(None, good.ctypes.data, *ptrs, 1, None) == -1
    lib.hrpt_probes_destroy(None)


@pytest.mark.parametrize("seed", [5, 6])
def test_host_side_is_clean_under_the_sanitizers(seed):
    """pt_probes.h + the host executors + a driver with its own main, built with AddressSanitizer and UBSan (`make probes_asan`), over
    every grid shape and ray count with untraced rays, hostile radiance, distances, atlases and query points on exactly sized heap arrays.
    Nothing is loaded into Python."""
    subprocess.check_call(["make", "-C", CSRC, "probes_asan"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(CSRC, "build", "probes_asan"), str(seed)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "no report" in r.stdout
