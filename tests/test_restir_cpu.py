"""Resampled direct lighting without a GPU: the four host executors against the NumPy statement of
tests/restir_reference.py, bit for bit, per flag and with all of them, with 1 and 32 candidates, 0, 1 and 8 neighbours, with and without a
history; thread-count invariance; the argument errors; the sanitizer build of the host side (`make restir_asan`, a stand-alone program); the
draw that is exactly 1.0; the one-light case against deferred lighting; and the two statistical statements -- in expectation the stage
equals deferred lighting with shadows, and reuse lowers the variance -- over fixed seeds, so their verdicts are deterministic."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from hobbyrenderer_amd import native, structs as S
import deferred_reference as R
import restir_cases as RC
import restir_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hobbyrenderer_amd", "csrc")
SYMBOLS = ("hrpt_restir_lighting", "hrpt_restir_lighting_device", "hrpt_read_restir_reservoirs", "hrpt_get_restir_device", "hrpt_restir_initial_device",
           "hrpt_restir_temporal_device", "hrpt_restir_spatial_device", "hrpt_restir_shade_device", "hrpt_restir_initial_host", "hrpt_restir_temporal_host",
           "hrpt_restir_spatial_host", "hrpt_restir_shade_host")
SHADOWS, SKY, TEMPORAL, SPATIAL, INITIAL_VISIBILITY, RESET = RR.SHADOWS, RR.SKY, RR.TEMPORAL, RR.SPATIAL, RR.INITIAL_VISIBILITY, RR.RESET
ALL = SHADOWS | SKY | TEMPORAL | SPATIAL | INITIAL_VISIBILITY
SIZES = pytest.mark.parametrize("size", RC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
COUNTS = pytest.mark.parametrize("count", RC.LIGHT_COUNTS)
# Largest deviation of the one-light image (n == 1, no reuse) from the float64 formulation of deferred lighting over the cases of this file,
# relative to the largest channel in play (measured here, recorded in DESIGN.md section 30): the test holds four times it.
MEASURED_ONE_LIGHT = 2.29e-6
# The sequences of the two statistical tests. K was chosen on the CPU so that the statement alone meets the 5-standard-error bar (the largest
# |z| of the fifteen means at K = 128 is 2.9).
K = 128


def same_bytes(got, want, what):
    a, b = np.frombuffer(got.tobytes(), np.uint32), np.frombuffer(want.tobytes(), np.uint32)
    if not np.array_equal(a, b):
        i = int(np.flatnonzero(a != b)[0])
        raise AssertionError(f"{what}: {int((a != b).sum())} of {a.size} words differ, first at word {i}: {a[i]:#x} != {b[i]:#x}")


@functools.lru_cache(maxsize=None)
def _targets(size, count, sun):
    c = RC.case(*size, count)
    return RR.targets(c["planes"], c["cb"], c["lights"], c["sun_radiance"] if sun else None)


def test_symbols_are_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "hobbyrt_pt.h")).read()
    for name in SYMBOLS:
        assert name in native.EXPORTS and hasattr(native.lib, name) and f" {name}(" in header, name
    assert "#define HRPT_ABI_VERSION 3" in header and S.ABI_VERSION == 3
    assert (S.RESTIR_SHADOWS, S.RESTIR_SKY, S.RESTIR_TEMPORAL, S.RESTIR_SPATIAL, S.RESTIR_INITIAL_VISIBILITY, S.RESTIR_RESET) == (1, 2, 4, 8, 16, 32)
    # that the C header says the same as the mirrors: test_binding_contract.py compiles a C program against it
    assert C.sizeof(S.RestirParams) == 48 and S.RestirParams.spatialRadius.offset == 16 and S.RestirParams.reserved.offset == 32
    assert S.RestirReservoir.itemsize == 16 and C.sizeof(S.RestirImages) == 88 and S.RestirImages.colorOut.offset == 80
    d = S.RestirParams()
    assert (d.flags, d.candidates, d.spatialSamples, d.spatialRadius, d.maxHistory, d.normalThreshold) == (SHADOWS | SKY | TEMPORAL | SPATIAL, 8, 1, 32.0, 20.0, 0.5)
    assert d.depthThreshold == np.float32(0.1)


# ---------------------------------------------------------------- 1. the four host executors == the statement
def _chain(c, p, sun, history, nthreads=3):
    """The four host executors chained as the context call chains them, the visibilities from the case: (initial, rays, temporal, final, keys, rays, image)."""
    sr = c["sun_radiance"] if sun else None
    cur, rays0 = native.restir_initial_host(c["planes"], c["cb"], c["lights"], p, sr, nthreads)
    iv = c["visibility"][0] if p.flags & INITIAL_VISIBILITY else None
    tres = native.restir_temporal_host(c["planes"], c["cb"], c["lights"], cur, p, sr, c["motion"] if p.flags & TEMPORAL else None, c["history"] if history else None, iv, nthreads)
    fin, keys, rays1 = native.restir_spatial_host(c["planes"], c["cb"], c["lights"], tres, p, sr, nthreads)
    image = native.restir_shade_host(c["planes"], c["cb"], c["lights"], fin, p, sr, c["sky"] if sun else None, c["visibility"][1] if p.flags & SHADOWS else None, nthreads)
    return cur, rays0, tres, fin, keys, rays1, image


def _statement(c, T, p, sun, history):
    cur = RR.initial(T, p)
    rays0 = RR.ray_records(T, cur) if p.flags & INITIAL_VISIBILITY else None
    iv = c["visibility"][0] if p.flags & INITIAL_VISIBILITY else None
    tres = RR.temporal(T, c["planes"], p, cur, c["motion"], c["history"] if history else None, iv)
    fin, keys = RR.spatial(T, c["planes"], p, tres)
    image = RR.shade(T, c["planes"], fin, c["visibility"][1] if p.flags & SHADOWS else None, c["sky"] if sun else None)
    return cur, rays0, tres, fin, keys, RR.ray_records(T, fin), image


VARIANTS = [dict(flags=0), dict(flags=SHADOWS), dict(flags=SKY), dict(flags=TEMPORAL), dict(flags=SPATIAL), dict(flags=INITIAL_VISIBILITY), dict(flags=TEMPORAL | RESET),
            dict(flags=ALL), dict(flags=ALL, history=False), dict(flags=ALL, candidates=1), dict(flags=ALL, candidates=32), dict(flags=ALL, spatialSamples=0),
            dict(flags=ALL, spatialSamples=8, spatialRadius=5.0), dict(flags=ALL, spatialSamples=8, normalThreshold=-1.0, depthThreshold=10.0)]
NAMES = ("initial reservoirs", "initial rays", "temporal reservoirs", "final reservoirs", "keys", "final rays", "image")


@SIZES
@COUNTS
def test_host_executors_equal_the_statement(size, count):
    c = RC.case(*size, count)
    for v in VARIANTS:
        v = dict(v)
        history, flags = v.pop("history", True), v.pop("flags")
        p = RC.params(flags, 3 + count, spatialRadius=6.0)
        for k, x in v.items():
            setattr(p, k, x)
        sun = bool(flags & SKY)
        got, ref = _chain(c, p, sun, history), _statement(c, _targets(size, count, sun), p, sun, history)
        for name, a, b in zip(NAMES, got, ref):
            assert (a is None) == (b is None), name
            if a is not None:
                same_bytes(a, b, f"{size} {count} lights {flags:#x} {v}: {name}")
        assert np.isfinite(got[6]).all()


def test_the_cases_hold_what_they_are_there_for():
    size = (61, 37)
    c = RC.case(*size, 40)
    sp = c["special"]
    assert set(sp) == set(RC.SPECIAL) and c["miss"].any() and not c["miss"].all()
    T = _targets(size, 40, False)
    p = RC.params(ALL & ~SKY, 9, spatialSamples=8, spatialRadius=6.0)
    cur, _, tres, fin, keys, rays, image = _statement(c, T, p, False, True)
    hit = ~c["miss"]
    x, y = sp["all_culled"]
    assert not T.lit[:, y, x].any() and cur[y, x]["light"] == S.RESTIR_EMPTY and cur[y, x]["M"] == p.candidates and cur[y, x]["W"] == 0
    on = tuple(RC.DC.SPECIAL["on_light"])
    assert T.lit[3, on[1], on[0]] and T.p[3, on[1], on[0]] == 0 and np.isnan(T.L[3, on[1], on[0]]).all()        # dist == 0: lit, a NaN target counts as 0
    assert (cur["light"][c["miss"]] == S.RESTIR_EMPTY).all() and (cur["M"][c["miss"]] == 0).all()
    assert (cur["light"][hit] != S.RESTIR_EMPTY).mean() > 0.5 and len(np.unique(cur["light"][hit])) > 20              # candidates come from all over the list
    # the temporal pass takes history records at some pixels, and never at the four that must not
    plain = RR.temporal(T, c["planes"], p, cur, c["motion"], None, c["visibility"][0])
    changed = (tres["M"] != plain["M"])
    assert 0.1 < changed[hit].mean() < 0.9
    for name in ("off_screen", "motion_w0", "history_light_out_of_range", "history_empty"):
        x, y = sp[name]
        assert not changed[y, x], name
    # the spatial pass accepts neighbours at some pixels and rejects at others
    alone, _ = RR.spatial(T, c["planes"], RC.params(ALL & ~SKY & ~SPATIAL, 9), tres)
    merged = fin["M"] != alone["M"]
    assert 0.1 < merged[hit].mean() < 0.99
    assert np.array_equal(keys[..., :3], c["planes"][1][..., :3]) and np.array_equal(keys[..., 3], c["planes"][4][..., 1])
    assert (image[c["miss"]] == 0).all() and (image[hit][:, :3] > 0).any()
    # one and no light
    for n in (0, 1):
        c1 = RC.case(*size, n)
        cur1 = RR.initial(_targets(size, n, False), p)
        assert set(np.unique(cur1["light"])) <= {0, S.RESTIR_EMPTY} and ((cur1["light"] == 0).any() if n else (cur1["M"] == 0).all())


def test_thread_count_does_not_matter():
    c = RC.case(61, 37, 40)
    p = RC.params(ALL, 5, spatialSamples=3, spatialRadius=6.0)
    one = _chain(c, p, True, True, nthreads=1)
    for n in (2, 5, 16, 64, 0):
        for name, a, b in zip(NAMES, _chain(c, p, True, True, nthreads=n), one):
            same_bytes(a, b, f"{n} threads: {name}")


def test_a_draw_of_exactly_one_still_takes_the_first_candidate():
    """hrt_rng_next returns exactly 1.0f for a state of at least 0xFFFFFF80. With frameSeed 1365036 the selection draw of the first candidate
    at pixel g = 80 of the 33 x 9 one-light case is such a draw (found by search); `u * wSum <= w` takes the candidate, `<` would not."""
    size, seed, g = (33, 9), 1365036, 80
    c = RC.case(*size, 1)
    T = _targets(size, 1, False)
    s = RR.states(seed, size[1], size[0])[0]
    s, _ = RR._rng_next(s)
    s, u1 = RR._rng_next(s)
    y, x = divmod(g, size[0])
    assert u1[y, x] == 1.0 and T.p[0, y, x] > 0
    p = RC.params(0, seed, candidates=1)
    got, _ = native.restir_initial_host(c["planes"], c["cb"], c["lights"], p)
    same_bytes(got, RR.initial(T, p), "initial reservoirs")
    assert got[y, x]["light"] == 0 and got[y, x]["W"] == 1.0 and got[y, x]["M"] == 1 and got[y, x]["pHat"] == T.p[0, y, x]


# ---------------------------------------------------------------- 2. one light: deferred lighting up to the rounding of W
def test_one_light_without_reuse_is_deferred_lighting():
    worst, worst_w = 0.0, 0.0
    for size in RC.SIZES:
        for light in (0, 1, 3):                                       # a spot, a point light, the point light with a finite range
            c = RC.case(*size, 9)
            lights = c["lights"][light:light + 1]
            cb = RC.DC.with_lights(c["cb"], 1)
            vis = c["visibility"][1]
            for candidates in (1, 8, 32):
                p = RC.params(SHADOWS, 11, candidates=candidates)
                cur, _ = native.restir_initial_host(c["planes"], cb, lights, p)
                tres = native.restir_temporal_host(c["planes"], cb, lights, cur, p)
                fin, _, _ = native.restir_spatial_host(c["planes"], cb, lights, tres, p)
                got = native.restir_shade_host(c["planes"], cb, lights, fin, p, visibility=vis)
                deferred = native.deferred_shade_host(*c["planes"], cb, lights, vis[None])
                ref = R.shade(*c["planes"], cb, lights, 0, vis[None], F=np.float64)
                hit = ~c["miss"]
                for x, y in list(c["special"].values()) + [q for q in RC.DC.SPECIAL.values() if q[0] < size[0] and q[1] < size[1]]:
                    hit[y, x] = False                                 # pixels that sit exactly on a decision in binary32 (test_deferred_cpu.py)
                chosen = fin["light"][hit] == 0
                w = fin["W"][hit][chosen]
                if w.size:
                    worst_w = max(worst_w, float(np.abs(w.astype(np.float64) - 1).max()))
                scale = np.abs(ref[hit][:, :3]).max() if hit.any() else 0.0
                if scale > 0:
                    worst = max(worst, float(np.abs(got[hit][:, :3].astype(np.float64) - ref[hit][:, :3]).max() / scale))
                    # and against deferred lighting's own float32 image: W is 1 up to a few roundings
                    assert np.abs(got[hit].astype(np.float64) - deferred[hit]).max() <= 8 * 2.0 ** -23 * scale
    print(f"one light vs float64 deferred lighting: largest deviation {worst:.3e} of the largest channel; |W - 1| at most {worst_w:.3e}")
    assert worst_w <= 4 * 2.0 ** -23
    assert worst <= 4 * MEASURED_ONE_LIGHT


# ---------------------------------------------------------------- 3. errors
def test_argument_errors():
    lib = native.lib
    err = lambda: lib.hrpt_last_error(None).decode()
    W, H = 33, 9
    c = RC.case(W, H, 9)
    planes = [np.ascontiguousarray(p) for p in c["planes"]]
    motion, hres, hkey = (np.ascontiguousarray(a) for a in (c["motion"], c["history"][0], c["history"][1]))
    out = np.full((H, W, 4), 7.0, np.float32)
    res = np.zeros((H, W), S.RestirReservoir); res.view(np.uint8)[:] = 7
    keys = np.full((H, W, 4), 7.0, np.float32)
    given = np.zeros((H, W), S.RestirReservoir)
    cb, lights = np.ascontiguousarray(c["cb"]), np.ascontiguousarray(c["lights"])
    ptrs = [p.ctypes.data for p in planes]
    full = lambda: S.RestirImages(*ptrs, motion.ctypes.data, hres.ctypes.data, hkey.ctypes.data, res.ctypes.data, keys.ctypes.data, out.ctypes.data)
    ok = RC.params(TEMPORAL | SPATIAL)

    def call(name, images="full", w=W, h=H, constants=cb.ctypes.data, l=lights.ctypes.data, p=ok, extra=None):
        images = full() if images == "full" else images
        tail = {"initial": [None, None], "temporal": [None, given.ctypes.data, None], "spatial": [None, given.ctypes.data, None], "shade": [None, None, given.ctypes.data, None]}[name]
        if extra:
            for k, v in extra.items():
                tail[k] = v
        return getattr(lib, f"hrpt_restir_{name}_host")(C.byref(images) if images is not None else None, w, h, constants, l, C.byref(p) if p is not None else None, *tail, 1)

    rule = (": unknown flag bits, non-zero reserved, candidates outside 1..32, spatialSamples above 8, a spatialRadius outside (0, 65535], "
            "a maxHistory that is not finite and positive, or a threshold that is not finite")
    bad = [RC.params(64), RC.params(0x80000000), RC.params(0, candidates=0), RC.params(0, candidates=33), RC.params(0, spatialSamples=9)]
    bad += [RC.params(0, spatialRadius=v) for v in (0.0, -1.0, math.nan, math.inf, 65536.0)] + [RC.params(0, maxHistory=v) for v in (0.0, -2.0, math.nan, math.inf)]
    bad += [RC.params(0, depthThreshold=v) for v in (math.nan, math.inf)] + [RC.params(0, normalThreshold=v) for v in (math.nan, -math.inf)]
    for k in range(4):
        p = RC.params(0); p.reserved[k] = 1
        bad.append(p)
    for name in ("initial", "temporal", "spatial", "shade"):
        what = f"hrpt_restir_{name}_host"
        assert call(name, images=None) == -1 and err() == what + ": null images"
        assert call(name, constants=None) == -1 and err() == what + ": null argument"
        assert call(name, p=None) == -1 and err() == what + ": null argument"
        for w, h in ((0, 9), (33, 0), (65536, 9)):
            assert call(name, w=w, h=h) == -1 and err() == what + ": size must be 1..65535"
        for k in (0, 1, 2, 4):
            im = full(); setattr(im, ("albedo", "normal", "geoNormal", "emissive", "depth")[k], None)
            assert call(name, images=im) == -1 and err() == what + ": null image", (name, k)
        assert call(name, l=None) == -1 and err() == what + ": null lights"
        for p in bad:
            assert call(name, p=p) == -1 and err() == what + rule, name
        written = {"initial": ["reservoirOut"], "temporal": ["reservoirOut"], "spatial": ["reservoirOut", "keyOut"], "shade": ["colorOut"]}[name]
        for field in written:
            im = full(); setattr(im, field, None)
            assert call(name, images=im) == -1 and err() == what + ": null output", (name, field)
            im = full(); setattr(im, field, ptrs[4])
            assert call(name, images=im) == -1 and err() == what + ": an output must differ from every other image", (name, field)
    assert call("shade", images=S.RestirImages(*ptrs[:3], None, ptrs[4], None, None, None, None, None, out.ctypes.data)) == -1 and err() == "hrpt_restir_shade_host: null image"
    im = full(); im.motion = None
    assert call("temporal", images=im) == -1 and err() == "hrpt_restir_temporal_host: HRPT_RESTIR_TEMPORAL without a motion image"
    im = full(); im.keyIn = None
    assert call("temporal", images=im) == -1 and err() == "hrpt_restir_temporal_host: reservoirIn and keyIn go together"
    im = full(); im.reservoirIn = res.ctypes.data
    assert call("temporal", images=im) == -1 and err() == "hrpt_restir_temporal_host: an output must differ from every other image"
    assert call("initial", p=RC.params(INITIAL_VISIBILITY)) == -1 and err() == "hrpt_restir_initial_host: HRPT_RESTIR_INITIAL_VISIBILITY without raysOut"
    for name, k in (("temporal", 1), ("spatial", 1), ("shade", 2)):
        assert call(name, extra={k: None}) == -1 and err() == f"hrpt_restir_{name}_host: null reservoirs"
        assert call(name, extra={k: (out if name == "shade" else res).ctypes.data}) == -1 and err() == f"hrpt_restir_{name}_host: an output must differ from every other image"
    # an error changes nothing
    assert (out == 7.0).all() and (keys == 7.0).all() and (res.view(np.uint8) == 7).all()
    # the context calls on NULL
    assert lib.hrpt_restir_lighting(None, cb.ctypes.data, C.byref(ok)) == -1
    assert lib.hrpt_restir_lighting_device(None, C.byref(full()), W, H, cb.ctypes.data, C.byref(ok), None) == -1
    assert lib.hrpt_read_restir_reservoirs(None, res.ctypes.data, res.nbytes) == -1 and lib.hrpt_get_restir_device(None, None, None) == -1


@pytest.mark.parametrize("seed", [5, 6])
def test_host_side_is_clean_under_the_sanitizers(seed):
    """pt_restir.h + the host executors + a driver with its own main, built with AddressSanitizer and UBSan (`make restir_asan`), chained as
    the context call chains them over every image size, 0 to 70 lights, every flag and hostile planes, motion, histories, lights and constants
    on exactly sized heap arrays. Nothing is loaded into Python."""
    subprocess.check_call(["make", "-C", CSRC, "restir_asan"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(CSRC, "build", "restir_asan"), str(seed)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "no report" in r.stdout


# ---------------------------------------------------------------- 4. in expectation: deferred lighting with shadows; reuse lowers the variance
@pytest.fixture(scope="module")
def floor(luts):
    """The floor scene's planes, its 40 lights, every (light, pixel) visibility from the oracle and deferred lighting's exact image."""
    import gbuffer_reference as G
    from oracle import binding
    sc = RC.floor_scene(luts)
    cb = RC.floor_constants(sc)
    W, H = RC.FLOOR_SIZE
    oracle = binding.Oracle(sc)
    try:
        planes = G.gbuffer(sc, oracle, cb, W, H)
        five = tuple(planes[i] for i in (S.GB_ALBEDO, S.GB_NORMAL, S.GB_GEO_NORMAL, S.GB_EMISSIVE, S.GB_DEPTH))
        lights = sc.lights[:RC.FLOOR_LIGHTS]
        assert not (lights["m_Type"] == S.LIGHT_DIRECTIONAL).any()
        records = R.rays(five[4], five[1], cb, lights)
        vis = R.visibilities(oracle, records)
    finally:
        oracle.close()
    exact = R.shade(*five, cb, lights, 0, vis)
    hit = five[4][..., 0] != R.MISS
    assert 0.5 < hit.mean() < 1 and (vis[:, hit] == 0).mean() > 0.05 and (exact[hit][:, :3] > 0).all()
    return dict(planes=five, cb=cb, lights=lights, records=records, vis=vis, exact=exact)


def sequence(f, k, flags, frames=3):
    """The last image of `frames` calls with distinct seeds, RESET on the first, through the host executors; a chosen light's visibility is
    the oracle's for that (light, pixel) pair, whose ray record is deferred lighting's (asserted on the first frame of sequence 0)."""
    H, W = f["vis"].shape[1:]
    yy, xx = np.mgrid[0:H, 0:W]
    motion = np.zeros((H, W, 4), np.float32)
    motion[..., 3] = 1.0
    history = None
    for frame in range(frames):
        p = RC.params(flags | (RESET if frame == 0 else 0), 1000 * k + frame + 7)
        cur, _ = native.restir_initial_host(f["planes"], f["cb"], f["lights"], p)
        tres = native.restir_temporal_host(f["planes"], f["cb"], f["lights"], cur, p, None, motion, history)
        fin, keys, rays = native.restir_spatial_host(f["planes"], f["cb"], f["lights"], tres, p)
        light = np.minimum(fin["light"], RC.FLOOR_LIGHTS - 1)
        if k == 0 and frame == 0:
            traced = ~np.isnan(rays["origin"]).any(-1)
            assert traced.any() and rays[traced].tobytes() == f["records"][light, yy, xx][traced].tobytes()
        image = native.restir_shade_host(f["planes"], f["cb"], f["lights"], fin, p, visibility=f["vis"][light, yy, xx])
        history = (fin, keys)
    return image


@pytest.fixture(scope="module")
def sequences(floor):
    return {name: np.array([sequence(floor, k, flags) for k in range(K)], np.float64)[..., :3] for name, flags in (("reuse", TEMPORAL | SPATIAL | SHADOWS), ("candidates", SHADOWS))}


def unbiasedness_z(images, exact):
    """z = (mean over the sequences - exact) / standard error, for the image mean and the four quadrant means, per channel: [5, 3]."""
    n, H, W = images.shape[:3]
    regions = [(slice(0, H), slice(0, W))] + [(ys, xs) for ys in (slice(0, H // 2), slice(H // 2, H)) for xs in (slice(0, W // 2), slice(W // 2, W))]
    z = []
    for ys, xs in regions:
        m = images[:, ys, xs].reshape(n, -1, 3).mean(1)
        z.append((m.mean(0) - exact[ys, xs, :3].astype(np.float64).reshape(-1, 3).mean(0)) / (m.std(0, ddof=1) / math.sqrt(n)))
    return np.array(z)


def test_in_expectation_the_stage_equals_deferred_lighting_with_shadows(floor, sequences):
    z = unbiasedness_z(sequences["reuse"], floor["exact"])
    print(f"K = {K}: z of the image mean and the four quadrant means per channel\n{np.round(z, 2)}\nlargest |z| {np.abs(z).max():.2f}")
    assert np.abs(z).max() <= 5.0


def test_reuse_lowers_the_variance(sequences):
    reuse, alone = (float(sequences[k].var(0, ddof=1).sum()) for k in ("reuse", "candidates"))
    print(f"summed per-pixel variance over {K} sequences: {reuse:.1f} with temporal and spatial reuse, {alone:.1f} with the candidates alone, ratio {reuse / alone:.3f}")
    assert reuse / alone < 1
