"""Deferred lighting without a GPU: the host executors hrpt_deferred_rays_host / hrpt_deferred_shade_host against
the NumPy statement of tests/deferred_reference.py, bit for bit, with and without the visibility, sun-radiance, sky and indirect images;
thread-count invariance; the statement against its float64 formulation; the argument errors; the sanitizer build of the host side
(`make deferred_asan`, a stand-alone program); and the statement against the path tracer's own bounce-0 direct light, both on the CPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from hobbyrenderer_amd import native, scenes, structs as S
import deferred_cases as DC
import deferred_reference as R
from test_temporal_cpu import u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hobbyrenderer_amd", "csrc")
SYMBOLS = ("hrpt_deferred_lighting", "hrpt_deferred_lighting_device", "hrpt_deferred_rays_host", "hrpt_deferred_shade_host")
SIZES = pytest.mark.parametrize("size", DC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
COUNTS = pytest.mark.parametrize("count", DC.LIGHT_COUNTS)
# Largest deviation of the float32 statement from the float64 formulation over the cases of this file, relative to the largest channel in
# play (measured here, recorded in DESIGN.md section 27): the test holds the statement to four times it.
MEASURED_STATEMENT = 1.32e-5
# Largest relative difference between the statement and the path tracer's bounce-0 direct light on the Cornell case below (interpolated hit
# position against o + d t, and the order of the final adds), relative to the image's largest channel: the test holds four times it.
MEASURED_PATH_TRACER = 0.0


def same_bytes(got, want, what):
    a, b = u32(got), u32(want)
    if not np.array_equal(a, b):
        i = tuple(np.argwhere(a != b)[0])
        raise AssertionError(f"{what}: {int((a != b).sum())} of {a.size} words differ, first at {i}: {got[i]} != {want[i]}")


def test_symbols_are_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "hobbyrt_pt.h")).read()
    for name in SYMBOLS:
        assert name in native.EXPORTS and hasattr(native.lib, name) and f" {name}(" in header, name
    assert "#define HRPT_ABI_VERSION 3" in header and S.ABI_VERSION == 3
    assert (S.DEFERRED_SHADOWS, S.DEFERRED_SKY, S.DEFERRED_INDIRECT) == (1, 2, 4)
    # that the C header says the same as the mirrors: test_binding_contract.py
    assert C.sizeof(S.DeferredParams) == 16 and S.DeferredParams.indirectIntensity.offset == 4 and S.DeferredParams.reserved.offset == 8
    assert C.sizeof(S.DeferredImages) == 56 and (S.DeferredImages.depth.offset, S.DeferredImages.indirect.offset, S.DeferredImages.colorOut.offset) == (32, 40, 48)


# ---------------------------------------------------------------- 1. rays
@SIZES
def test_rays_host_equals_reference(size):
    c = DC.case(*size)
    depth, normal = c["planes"][4], c["planes"][1]
    got = native.deferred_rays_host(depth, normal, c["cb"], c["lights"])
    ref = R.rays(depth, normal, c["cb"], c["lights"])
    assert got.shape == (9, size[1], size[0])
    assert got.tobytes() == ref.tobytes()
    assert (got["tmin"] == 0).all() and (got["rng"] == 0).all() and (got["pad"] == 0).all()
    unlit = np.isnan(got["origin"]).all(-1)
    assert (u32(got["origin"][unlit]) == 0x7FC00000).all() and (got["direction"][unlit] == 0).all() and (got["tmax"][unlit] == 0).all()
    assert unlit[:, c["miss"]].all() and unlit[4].all() and unlit[5].all()              # misses, the unknown type, intensity 0
    # a sub-range is the same records
    for first, count in ((0, 4), (4, 4), (8, 1), (3, 0)):
        part = native.deferred_rays_host(depth, normal, c["cb"], c["lights"], first, count)
        assert part.tobytes() == ref[first:first + count].tobytes(), (first, count)


def test_the_cases_hold_what_they_are_there_for():
    c = DC.case(61, 37)
    rays = R.rays(c["planes"][4], c["planes"][1], c["cb"], c["lights"])
    lit = ~np.isnan(rays["origin"]).all(-1)
    sp = c["special"]
    assert set(sp) == set(DC.SPECIAL) and c["miss"].any() and not c["miss"].all()
    x, y = sp["on_light"]
    assert rays["tmax"][3, y, x] == 0 and np.isnan(rays["direction"][3, y, x]).all() and lit[3, y, x]       # dist == 0: L = 0 / 0, the pair stays lit
    x, y = sp["grazing"]
    _, L, _ = R.light_direction(c["lights"][7], c["planes"][1][..., :3], R.hit_positions(c["cb"], c["planes"][4])[2], None)
    assert R._dot(c["planes"][1][y, x, :3], L[y, x]) == 0 and not lit[7, y, x]                               # dot(N, L) == 0 exactly: skipped
    x, y = sp["cone_edge"]
    assert lit[6, y, x] and lit[6].sum() == 1 and np.array_equal(rays["direction"][6, y, x], np.float32([0, 1, 0]))   # cosTheta == cosOuter == 1
    x, y = sp["v_is_minus_l"]
    d = R.hit_positions(c["cb"], c["planes"][4])[1]
    assert lit[2, y, x] and np.array_equal(rays["direction"][2, y, x], d[y, x])                              # L == d == -V
    for i in (0, 1, 2, 3, 7, 8):
        assert 0 < lit[i].sum() < lit[i].size, i                                                             # every real light lights some pixels, not all
    X = R.hit_positions(c["cb"], c["planes"][4])[2]
    far = ((c["lights"][3]["m_Position"] - X) ** 2).sum(-1) > 2.5 ** 2 + 0.01
    assert (far & ~c["miss"]).any() and not lit[3][far].any()                                                # the finite range culls


# ---------------------------------------------------------------- 2. shade
def _host(c, count, flags=0, vis=False, sun=False, sky=False, indirect=False, nthreads=3, intensity=0.7):
    return native.deferred_shade_host(*c["planes"], DC.with_lights(c["cb"], count), c["lights"][:count], c["visibility"][:count] if vis else None,
                                      c["sun_radiance"] if sun else None, c["sky"] if sky else None, c["indirect"] if indirect else None,
                                      S.DeferredParams(flags, intensity), nthreads)


def _statement(c, count, flags=0, vis=False, sun=False, sky=False, indirect=False, intensity=0.7, **kw):
    return R.shade(*c["planes"], DC.with_lights(c["cb"], count), c["lights"][:count], flags, c["visibility"][:count] if vis else None,
                   c["sun_radiance"] if sun else None, c["sky"] if sky else None, c["indirect"] if indirect else None, intensity, **kw)


@SIZES
@COUNTS
def test_shade_host_equals_reference(size, count):
    c = DC.case(*size)
    for kw in (dict(), dict(vis=True), dict(sun=True), dict(sky=True), dict(flags=S.DEFERRED_INDIRECT, indirect=True),
               dict(flags=S.DEFERRED_INDIRECT, vis=True, sun=True, sky=True, indirect=True)):
        got, ref = _host(c, count, **kw), _statement(c, count, **kw)
        same_bytes(got, ref, f"{size} {count} {kw}")
        assert np.isfinite(got).all()
    got = _host(c, count, vis=True, sky=True)
    assert np.array_equal(got[c["miss"]], c["sky"][c["miss"]]) and np.array_equal(got[~c["miss"]][:, 3], c["planes"][0][~c["miss"]][:, 3])
    assert (_host(c, count)[c["miss"]] == 0).all()


def test_every_input_matters_and_indirect_without_the_flag_does_not():
    c = DC.case(61, 37)
    base = _host(c, 9)
    for kw in (dict(vis=True), dict(sun=True), dict(sky=True), dict(flags=S.DEFERRED_INDIRECT, indirect=True)):
        assert not np.array_equal(base, _host(c, 9, **kw)), kw
    same_bytes(_host(c, 9, indirect=True), base, "an indirect image without the flag")
    assert not np.array_equal(_host(c, 3), base) and not np.array_equal(_host(c, 0), _host(c, 1))
    # emissive only with no light; texels with indirect.w != 1 get no indirect term
    none = _host(c, 0)
    hit = ~c["miss"]
    same_bytes(none[hit][:, :3], c["planes"][3][hit][:, :3] + np.float32(0), "no light: emissive")
    ind = _host(c, 0, flags=S.DEFERRED_INDIRECT, indirect=True)
    off = hit & (c["indirect"][..., 3] != 1)
    assert off.any() and np.array_equal(ind[off], none[off]) and not np.array_equal(ind[hit & ~off], none[hit & ~off])


def test_thread_count_does_not_matter():
    c = DC.case(61, 37)
    kw = dict(flags=S.DEFERRED_INDIRECT, vis=True, sun=True, sky=True, indirect=True)
    one = _host(c, 9, nthreads=1, **kw)
    for n in (2, 5, 16, 64, 0):
        same_bytes(_host(c, 9, nthreads=n, **kw), one, f"{n} threads")


def test_statement_is_close_to_float64():
    worst = 0.0
    for size in DC.SIZES:
        c = DC.case(*size)
        for kw in (dict(), dict(vis=True, sun=True)):
            a, lit32 = _statement(c, 9, return_lit=True, **kw)
            b, lit64 = _statement(c, 9, F=np.float64, return_lit=True, **kw)
            # the special pixels sit exactly on a decision in binary32 (dist == 0, dot == 0, the cone edge, V + L == 0), which binary64's X does
            # not reproduce: they are left out; everywhere else the cull decisions agree
            hit = ~c["miss"]
            for x, y in c["special"].values():
                hit[y, x] = False
            assert np.array_equal(lit32[:, hit], lit64[:, hit])
            scale = np.abs(b[hit][:, :3]).max() if hit.any() else 0.0
            if scale > 0:
                worst = max(worst, float(np.abs(a[hit][:, :3].astype(np.float64) - b[hit][:, :3]).max() / scale))
    print(f"statement vs float64: largest deviation {worst:.3e} of the largest channel")
    assert worst <= 4 * MEASURED_STATEMENT


# ---------------------------------------------------------------- 3. errors
def test_argument_errors():
    lib = native.lib
    err = lambda: lib.hrpt_last_error(None).decode()
    c = DC.case(33, 9)
    W, H = 33, 9
    planes = [np.ascontiguousarray(p) for p in c["planes"]]
    out = np.full((H, W, 4), 7.0, np.float32)
    rays = np.zeros((9, H, W), S.Ray); rays.view(np.uint8)[:] = 7
    cb, lights = np.ascontiguousarray(c["cb"]), np.ascontiguousarray(c["lights"])
    ptrs = [p.ctypes.data for p in planes]
    im = S.DeferredImages(*ptrs, None, out.ctypes.data)
    ok = S.DeferredParams(0, 1.0)
    shade = lambda images=im, w=W, h=H, constants=cb.ctypes.data, l=lights.ctypes.data, n=9, vis=None, sun=None, sky=None, p=ok: \
        lib.hrpt_deferred_shade_host(C.byref(images) if images is not None else None, w, h, constants, l, n, vis, sun, sky, C.byref(p) if p is not None else None, 1)
    assert shade(images=None) == -1 and err() == "hrpt_deferred_shade_host: null images"
    assert shade(constants=None) == -1 and err() == "hrpt_deferred_shade_host: null argument"
    assert shade(p=None) == -1 and err() == "hrpt_deferred_shade_host: null argument"
    for w, h in ((0, 9), (33, 0), (65536, 9)):
        assert shade(w=w, h=h) == -1 and err() == "hrpt_deferred_shade_host: size must be 1..65535"
    for k in list(range(5)) + [6]:
        p = ptrs + [None, out.ctypes.data]; p[k] = None
        assert shade(images=S.DeferredImages(*p)) == -1 and err() == "hrpt_deferred_shade_host: null image", k
    for k in range(5):
        assert shade(images=S.DeferredImages(*ptrs, None, ptrs[k])) == -1 and err() == "hrpt_deferred_shade_host: colorOut must differ from every other image"
    assert shade(sky=out.ctypes.data) == -1 and err() == "hrpt_deferred_shade_host: colorOut must differ from every other image"
    assert shade(l=None) == -1 and err() == "hrpt_deferred_shade_host: null lights"
    assert shade(l=None, n=0) == 0 and (out[~c["miss"]][:, :3] == planes[3][~c["miss"]][:, :3]).all()
    out[:] = 7.0
    rule = ": unknown flag bits, non-zero reserved or an indirectIntensity that is not finite"
    bad = [S.DeferredParams(8, 1.0), S.DeferredParams(0x80000000, 1.0), S.DeferredParams(0, math.nan), S.DeferredParams(0, math.inf), S.DeferredParams(0, -math.inf)]
    for k in range(2):
        p = S.DeferredParams(0, 1.0); p.reserved[k] = 1
        bad.append(p)
    for p in bad:
        assert shade(p=p) == -1 and err() == "hrpt_deferred_shade_host" + rule
    assert shade(p=S.DeferredParams(S.DEFERRED_INDIRECT, 1.0)) == -1 and err() == "hrpt_deferred_shade_host: HRPT_DEFERRED_INDIRECT without an indirect image"
    ray = lambda images=im, w=W, h=H, constants=cb.ctypes.data, l=lights.ctypes.data, first=0, n=9, r=rays.ctypes.data: \
        lib.hrpt_deferred_rays_host(C.byref(images) if images is not None else None, w, h, constants, l, first, n, r)
    assert ray(images=None) == -1 and err() == "hrpt_deferred_rays_host: null argument"
    assert ray(constants=None) == -1 and err() == "hrpt_deferred_rays_host: null argument"
    assert ray(w=0) == -1 and err() == "hrpt_deferred_rays_host: size must be 1..65535"
    for k in (1, 4):
        p = ptrs + [None, None]; p[k] = None
        assert ray(images=S.DeferredImages(*p)) == -1 and err() == "hrpt_deferred_rays_host: the depth and normal images are required", k
    assert ray(l=None) == -1 and err() == "hrpt_deferred_rays_host: null array"
    assert ray(r=None) == -1 and err() == "hrpt_deferred_rays_host: null array"
    assert ray(first=0xFFFFFFFF, n=2) == -1 and err() == "hrpt_deferred_rays_host: light range out of range"
    assert ray(n=0, r=None, l=None) == 0                                # nothing to do
    # an error changes nothing
    assert (out == 7.0).all() and (rays.view(np.uint8) == 7).all()
    # the context calls on NULL
    assert lib.hrpt_deferred_lighting(None, cb.ctypes.data, C.byref(ok)) == -1
    assert lib.hrpt_deferred_lighting_device(None, C.byref(im), W, H, cb.ctypes.data, C.byref(ok), None) == -1


@pytest.mark.parametrize("seed", [5, 6])
def test_host_side_is_clean_under_the_sanitizers(seed):
    """pt_deferred.h + the host executors + a driver with its own main, built with AddressSanitizer and UBSan (`make deferred_asan`), over
    every image size and light count with misses, every optional image present and absent and hostile planes, lights and constants on
    exactly sized heap arrays. Nothing is loaded into Python."""
    subprocess.check_call(["make", "-C", CSRC, "deferred_asan"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(CSRC, "build", "deferred_asan"), str(seed)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "no report" in r.stdout


# ---------------------------------------------------------------- 4. against the path tracer's own direct light, on the CPU
def test_statement_equals_the_path_tracers_bounce_0_direct_light(luts):
    """Cornell with the point and spot light at radius 0 and every material at m_IOR 1.5, 61 x 37, m_MaxBounces = 1, one sample: the oracle's
    Accumulation is then emissive + deterministic direct light (the sun is blocked by the closed room, the two other lights are points).
    The statement is fed the oracle's visibilities and the G-buffer planes of gbuffer_reference. The two differ in X (interpolated position
    against o + d t) and in the order of the final adds; a pixel whose visibility flips at a shadow edge because of X is left out, at most
    0.5 % of the hit pixels."""
    import gbuffer_reference as G
    from oracle import binding
    W, H = 61, 37
    sc = scenes.cornell_scene(luts, extra_lights=True)
    sc.lights["m_Radius"] = 0.0
    assert (sc.materials["m_IOR"] == np.float32(1.5)).all()
    view, pos = scenes.planar_view(W, H, position=(0.0, 1.0, -3.4), fov_y=math.radians(40.0))
    cb = scenes.fill_constants(view, pos, sc, 0, 1)
    oracle = binding.Oracle(sc)
    try:
        acc, out = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
        oracle.render(cb, acc, out)
        planes = G.gbuffer(sc, oracle, cb, W, H)
        five = [planes[i] for i in (S.GB_ALBEDO, S.GB_NORMAL, S.GB_GEO_NORMAL, S.GB_EMISSIVE, S.GB_DEPTH)]
        assert not (five[4][..., 0] == R.MISS).any()                                   # a closed room
        records = R.rays(five[4], five[1], cb, sc.lights)
        vis = R.visibilities(oracle, records)
        sun_radiance, _ = R.atmosphere(oracle, cb, five[4], float(sc.lights[0]["m_Intensity"]))
    finally:
        oracle.close()
    ref = R.shade(*five, cb, sc.lights, 0, vis, sun_radiance)
    assert (acc[..., 3] == 1).all()
    direct = ref[..., :3] - five[3][..., :3]
    lit_pixels = (direct > 0).any(-1)
    print(f"direct light: {int(lit_pixels.sum())} of {lit_pixels.size} pixels, largest channel {float(direct.max()):.3f}")
    assert lit_pixels.mean() > 0.5 and direct.max() > 0.1                              # the comparison is of direct light, not of emissive alone
    scale = float(acc[..., :3].max())
    diff = np.abs(ref[..., :3].astype(np.float64) - acc[..., :3]).max(-1) / scale
    flipped = diff > 1e-3                                                              # a whole light's contribution, not rounding
    print(f"statement vs path tracer: {int(flipped.sum())} of {flipped.size} pixels flipped at a shadow edge, largest difference elsewhere {diff[~flipped].max():.3e} of {scale:.3f}")
    assert flipped.sum() <= 0.005 * flipped.size
    assert diff[~flipped].max() <= 4 * MEASURED_PATH_TRACER
    assert ((vis > 0) & (vis < 1)).sum() == 0 and (vis == 0).any() and (vis == 1).any()         # hard shadows, both outcomes
