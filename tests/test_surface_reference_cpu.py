"""Hit attributes, normal maps and sampled-alpha masks against a float64 reference written from the shader text (tests/surface_reference.py,
DESIGN.md section 31), settled on the CPU against the oracle, whose G-buffer and render the GPU reproduces bit for bit.

* The vertex decode, exhaustively: every code of every field against or_unpack_vertex.
* The first hit of cases F, G and H (tests/surface_cases.py): 48 x 27 primary rays per camera, the hit by path_reference's brute force
  over the reference's own world triangles, the attributes by surface_reference at the reference's (u, v), against the oracle's G-buffer
  (gbuffer_reference, the device's in bits): ids and flags exactly, the float planes to TAU_ATTR (TAU_ATTR_FAR on the island) in
  |got - ref|_inf / max(|ref|_inf, 1) per pixel and plane. A pixel whose decision margin is below path_reference.DELTA is left out.
* Whole paths of F, G and H under section 31's protocol with the new decisions in the margin, to TAU_SURFACE.
* The bars are module constants of surface_reference.py and path_reference.py, measured here and nowhere else.
* Conditions from the reference alone: at most 5 % left out, at least 32 included samples per branch (normal map on a front face, a back face and
  a mirrored instance, clipped z, each sampler, MASK commit and reject at the closest hit, shadow MASK blocks and passes, each of the
  alpha map's four gradient levels, dist < 0.1).
* Seventeen mutations of the reference, each of which the oracle must miss by more than the bar on at least 5 included samples.
* The exact probes: alpha == cutoff commits, the next binary32 cutoff above does not, with no margin at all."""
import numpy as np
import pytest

from hobbyrenderer_amd import scenes, structs as S
import gbuffer_reference as G
import path_cases as PC
import path_reference as R
import surface_cases as SC
import surface_reference as SR

PLANES = ["albedo", "normal", "geo_normal", "emissive", "depth"]
MINIMUM, CAUGHT_MINIMUM = 32, 5
_CACHE = {}


# ---------------------------------------------------------------- the decode
def _every_code():
    """65 536 records: every tangent code once, every half once in each uv slot, every normal code 64 times in each component (the three
    components run through the codes at different offsets), both sign bits, and bit 31 and the tangent's upper half set at random."""
    i = np.arange(65536, dtype=np.uint32)
    rng = np.random.default_rng(3)
    v = np.zeros(len(i), S.VertexQuantized)
    v["m_Pos"] = rng.normal(size=(len(i), 3)).astype(np.float32)
    v["m_Normal"] = (i % 1024) | (((i + 341) % 1024) << 10) | (((i * 7 + 682) % 1024) << 20) | (((i >> 10) & 1) << 30) | (((i >> 11) & 1) << 31)
    v["m_Tangent"] = i | (rng.integers(0, 65536, len(i)).astype(np.uint32) << 16)
    v["m_Uv"] = i | ((np.uint32(65535) - i) << 16)
    return v


def test_decode_of_every_code_against_the_oracle():
    """UnpackVertex / DecodeOct of every code. Integers (the sign of the tangent, the halfs, the positions) must agree exactly.

    Normal: fl(fl(c / 511) - 1). The division rounds once, by at most half an ulp of a number below 4, 2^-23; the subtraction is exact
    for c / 511 in [0.5, 2] (Sterbenz) and rounds by at most 2^-25 otherwise. Bound 2^-22.

    Tangent: e = fl(fl(c / 127) - 1) carries at most 2^-23 (as above, |c / 127| < 2.01) + 2^-24; z = 1 - |ex| - |ey| two more roundings
    of numbers below 2 and the errors of ex and ey, together below 5 * 2^-24 + 2 * 2^-24; the fold adds one rounding and t's error to x
    and y: every component of v is known to 11 * 2^-24. |v|_1 = 1 before the fold and >= 1 after it, so |v|_2 >= 1 / sqrt(3) and the
    normalised components move by at most 2 * sqrt(3) * 11 * 2^-24 < 39 * 2^-24; normalize itself (three products, two sums, sqrt,
    reciprocal, product: 8 roundings of relative 2^-24) adds 8 * 2^-24. Bound 47 * 2^-24 < 2^-18."""
    from oracle.binding import lib
    raw = _every_code()
    out = np.zeros((len(raw), 12), np.float32)
    fn, pv, po = lib().or_unpack_vertex, raw.ctypes.data, out.ctypes.data
    for k in range(len(raw)):
        fn(pv + 24 * k, po + 48 * k)
    ref = SR.decode_vertices(raw)
    codes = ref["codes"]
    assert all(len(np.unique(codes[:, k])) == 1024 for k in range(3)) and set(np.unique(codes[:, 3])) == {0, 1}
    assert len(np.unique(codes[:, 4] | (codes[:, 5] << 8))) == 65536 and len(np.unique(codes[:, 6])) == 65536 and len(np.unique(codes[:, 7])) == 65536
    assert np.array_equal(out[:, 0:3], raw["m_Pos"])
    assert np.array_equal(out[:, 11].astype(np.float64), ref["tangent"][:, 3])                                   # bit 30, not bit 31
    with np.errstate(invalid="ignore"):                                    # widening a signalling NaN
        assert np.array_equal(out[:, 6:8].astype(np.float64), ref["uv"], equal_nan=True)                          # exact, NaN and infinity included
    assert np.isnan(ref["uv"]).sum() == 2 * 2046 and np.isinf(ref["uv"]).sum() == 4
    e_n = np.abs(out[:, 3:6] - ref["normal"]).max()
    e_t = np.abs(out[:, 8:11] - ref["tangent"][:, :3]).max()
    print(f"decode: normal off by at most {e_n:.3e} (bound {2.0 ** -22:.3e}), tangent by {e_t:.3e} (bound {2.0 ** -18:.3e})")
    assert e_n <= 2.0 ** -22 and e_t <= 2.0 ** -18
    assert np.abs(np.sqrt((ref["tangent"][:, :3] ** 2).sum(1)) - 1.0).max() < 1e-15


def test_quantised_unit_vectors_decode_to_themselves():
    """scenes.quantize_vertex round trips of random unit vectors: the normal within half a step of the 10-bit code per component, the
    tangent within the 8-bit octahedral code's step (a half step of 1 / 254 in each of e.x and e.y, before normalisation at most
    3 / 254 per component, after it at most sqrt(3) times that), the sign and the half-precision uv exactly."""
    rng = np.random.default_rng(8)
    unit = lambda a: a / np.sqrt((a * a).sum(1, keepdims=True))      # noqa: E731
    n, t = unit(rng.normal(size=(300, 3))), unit(rng.normal(size=(300, 3)))
    uv = np.round(rng.uniform(-2, 2, (300, 2)) * 256) / 256
    w = np.where(rng.random(300) < 0.5, -1.0, 1.0)
    raw = np.array([scenes.quantize_vertex((0, 0, 0), n[k], uv[k], t[k], w[k]) for k in range(300)], S.VertexQuantized)
    assert np.array_equal(raw, scenes.quantize_vertices(np.zeros((300, 3)), n, uv, t, w))
    ref = SR.decode_vertices(raw)
    assert np.abs(ref["normal"] - n).max() <= 0.5 / 511 + 1e-7
    assert np.abs(ref["tangent"][:, :3] - t).max() <= np.sqrt(3.0) * 3.0 / 254
    assert np.array_equal(ref["tangent"][:, 3], w) and np.array_equal(ref["uv"], uv)
    assert (t[:, 2] < 0).sum() > 100 and (ref["tangent"][:, 2] < 0).sum() > 100


# ---------------------------------------------------------------- the first hit
def _first_hit(luts, name):
    """(case, reference views, the oracle's planes per view), once per session."""
    key = ("first hit", name)
    if key not in _CACHE:
        from oracle.binding import Oracle
        case = SC.case(name, luts)
        o = Oracle(case.scene)
        try:
            got = [G.gbuffer(case.scene, o, cb, w, h) for _, cb, w, h in case.first_hit_views()]
        finally:
            o.close()
        _CACHE[key] = (case, SC.first_hit_reference(case), got)
    return _CACHE[key]


def _first_hit_errors(case, ref, got):
    """Per view: (included, ids agree, {plane: error}, bar)."""
    out = []
    for k, ((label, cb, w, h, planes, margin, info), g) in enumerate(zip(ref, got)):
        same = (g[S.GB_IDS].reshape(-1, 4).astype(np.int64) == planes[S.GB_IDS]).all(1)
        err = {PLANES[p]: SR.plane_error(g[p], planes[p]) for p in range(5)}
        out.append((margin >= R.DELTA, same, err, SR.TAU_ATTR_FAR if k in case.far_views else SR.TAU_ATTR))
    return out


@pytest.mark.parametrize("name", SC.NAMES)
def test_oracle_first_hit_equals_the_reference(luts, name):
    case, ref, got = _first_hit(luts, name)
    for (label, *_), (inc, same, err, bar) in zip(ref, _first_hit_errors(case, ref, got)):
        worst = {p: float(np.where(inc, e, 0.0).max()) for p, e in err.items()}
        print(f"case {name}, {label}: {len(inc)} pixels, {int((~inc).sum())} left out, ids differ on {int((~same).sum())}, worst included error "
              + ", ".join(f"{p} {w:.3e}" for p, w in worst.items()) + f", bar {bar:.3e}")
        assert (same | ~inc).all(), f"{label}: ids, hit or front-face flags differ at pixel {int(np.argmax(~same & inc))}"
        for p, e in err.items():
            assert worst[p] <= bar, f"{label}, {p}: pixel {int(np.argmax(np.where(inc, e, 0.0)))}"


def test_domain_of_the_tangent_frame(luts):
    """|cross(n_w, t_w)| > 1e-2 and |interpolated local normal| > 1e-2 on every hit of every view: the Gram-Schmidt step is not a finite
    number otherwise, and that corner stays with the bit comparison against the oracle."""
    for name in SC.NAMES:
        for label, *_, info in _first_hit(luts, name)[1]:
            assert info["pbr"]["sine"].min() > 1e-2 and info["attr"]["local_normal_length"].min() > 1e-2, (name, label)


# ---------------------------------------------------------------- paths
def _paths(luts, name):
    """dict(case, ps, views, rays, oracle [n, 4], paths) of a case under section 31's protocol, once per session."""
    key = ("paths", name)
    if key not in _CACHE:
        from oracle.binding import Oracle
        case = SC.case(name, luts)
        ps = R.PathScene(case.scene)
        views = case.views()
        o = Oracle(case.scene)
        try:
            got, rays = [], []
            for _, cb, w, h in views:
                acc, out = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
                o.render(cb, acc, out)
                got.append(acc.reshape(-1, 4)); rays.append(PC.rays_of(cb, w, h))
        finally:
            o.close()
        paths = R.concatenate([R.trace_paths(ps, cb, r) for (_, cb, _, _), r in zip(views, rays)])
        _CACHE[key] = dict(case=case, ps=ps, views=views, rays=rays, oracle=np.concatenate(got), paths=paths)
    return _CACHE[key]


@pytest.mark.parametrize("name", SC.NAMES)
def test_oracle_render_equals_the_replay(luts, name):
    m = _paths(luts, name)
    assert (m["oracle"][:, 3] == 1.0).all() and np.isfinite(m["paths"].radiance).all()
    err = R.path_error(m["oracle"], m["paths"])
    inc = m["paths"].included()
    worst = int(np.argmax(np.where(inc, err, -1.0)))
    print(f"case {name}: {len(err)} paths, {int((~inc).sum())} left out, worst included error {err[worst]:.3e} (path {worst}), tau {R.TAU_SURFACE:.3e}")
    assert err[worst] <= R.TAU_SURFACE, f"path {worst}: oracle {m['oracle'][worst, :3]} against {m['paths'].radiance[worst]}, margin {m['paths'].margin[worst]:.3e}"
    assert not ((err > 1e-2) & inc).any()


def test_the_bars_are_what_the_oracle_measures(luts):
    """TAU_ATTR / TAU_ATTR_FAR = 4 x the worst included first-hit error, rounded up to a power of two; DELTA stays section 31's because no
    path of F - H deviates by more than 1e-2; TAU_SURFACE = 4 x the worst included path error, which does not fit TAU / 4."""
    import math
    near, far = 0.0, 0.0
    print()
    for name in SC.NAMES:
        case, ref, got = _first_hit(luts, name)
        left, total = 0, 0
        for k, (inc, same, err, bar) in enumerate(_first_hit_errors(case, ref, got)):
            w = max(float(np.where(inc, e, 0.0).max()) for e in err.values())
            near, far = (near, max(far, w)) if k in case.far_views else (max(near, w), far)
            left, total = left + int((~inc).sum()), total + len(inc)
        print(f"  case {name}, first hit: {total} pixels, {100 * left / total:.2f} % left out")
    print(f"  worst included first-hit error {near:.4e}, on the island {far:.4e}")
    for worst, recorded, bar in ((near, SR.TAU_ATTR_WORST_INCLUDED_ERROR, SR.TAU_ATTR), (far, SR.TAU_ATTR_FAR_WORST_INCLUDED_ERROR, SR.TAU_ATTR_FAR)):
        assert 2.0 ** math.ceil(math.log2(4.0 * worst)) == bar and abs(worst - recorded) <= 1e-3 * recorded, (worst, recorded)
    worst = 0.0
    for name in SC.NAMES:
        m = _paths(luts, name)
        err, inc = R.path_error(m["oracle"], m["paths"]), m["paths"].included()
        print(f"  case {name}, paths: worst included error {err[inc].max():.3e}, left out {100 * (1 - inc.mean()):.2f} % of {len(inc)}, "
              f"deviating by more than 1e-2: {int((err > 1e-2).sum())}")
        assert (err > 1e-2).sum() == 0, "a flip: DELTA has to be derived again"
        recorded = R.SURFACE_CASE_TABLE[name]
        assert f"{err[inc].max():.3e}" == f"{recorded[0]:.3e}" and f"{1 - inc.mean():.4f}" == f"{recorded[1]:.4f}", (name, err[inc].max(), 1 - inc.mean())
        worst = max(worst, float(err[inc].max()))
    assert worst > R.TAU / 4.0, "the paths fit section 31's bar with its headroom: TAU_SURFACE is not needed"
    assert R.TAU_SURFACE == 4.0 * R.TAU_SURFACE_WORST_INCLUDED_ERROR and abs(worst - R.TAU_SURFACE_WORST_INCLUDED_ERROR) <= 1e-3 * worst


# ---------------------------------------------------------------- conditions, from the reference alone
@pytest.mark.parametrize("name", SC.NAMES)
def test_at_most_five_percent_are_left_out(luts, name):
    case = SC.case(name, luts)
    for label, *_, margin, _ in SC.first_hit_reference(case):
        assert (margin < R.DELTA).mean() <= R.MAX_EXCLUDED_SHARE, label
    assert 1.0 - _paths(luts, name)["paths"].included().mean() <= R.MAX_EXCLUDED_SHARE


def _branch_counts(luts):
    count = {}
    add = lambda b, n: count.__setitem__(b, count.get(b, 0) + int(n))      # noqa: E731
    for name in SC.NAMES:
        case = SC.case(name, luts)
        for label, cb, w, h, planes, margin, info in SC.first_hit_reference(case):
            inc = (margin >= R.DELTA)[info["rows"]]
            p = info["pbr"]
            mapped = (p["sampler"] >= 0) & inc
            det = np.array([np.linalg.det(np.asarray(r["m_World"], np.float64)[:3, :3]) for r in case.scene.instances])
            mirrored = det[planes[S.GB_IDS][info["rows"], 0]] < 0
            add("normal map on a front face", (mapped & info["front"]).sum())
            add("normal map on a back face", (mapped & ~info["front"]).sum())
            add("normal map on a mirrored instance", (mapped & mirrored).sum())
            add("saturate-clipped z", (mapped & p["clipped"]).sum())
            for s, what in ((5, "linear-wrap"), (2, "point-clamp"), (1, "anisotropic")):
                add(f"normal map through the {what} sampler", (mapped & (p["sampler"] == s)).sum())
        paths = _paths(luts, name)["paths"]
        for b in R.SURFACE_BRANCHES:
            add(b, (paths.took[b] & paths.included()).sum())
    return count


def test_every_branch_is_reached_by_enough_included_samples(luts):
    count = _branch_counts(luts)
    print(count)
    short = {b: c for b, c in count.items() if c < MINIMUM}               # every one of the alpha map's four levels among them
    assert not short, short


# ---------------------------------------------------------------- mutations
FIRST_HIT_MUTATIONS = ("tangent_through_world", "normal_through_world", "mirror_without_flip", "tangent_sign_from_vertex_0",
                       "bitangent_sign_ignored", "normal_map_y_negated", "no_gram_schmidt", "vertex_normals_normalised", "normal_div_512",
                       "tangent_div_128", "sign_bit_31", "uv_swapped")
FIRST_HIT_MUTATIONS_G = ("closest_alpha_at_shadow_level",)
PATH_MUTATIONS = ("shadow_alpha_at_level_0", "gradient_without_max_dist", "gradient_without_half_area")


def test_every_mutation_has_its_test():
    assert set(FIRST_HIT_MUTATIONS + FIRST_HIT_MUTATIONS_G + PATH_MUTATIONS + ("alpha_greater_than",)) == set(SR.MUTATIONS) and len(SR.MUTATIONS) == 17


@pytest.mark.parametrize("mutation,name", [(m, "F") for m in FIRST_HIT_MUTATIONS] + [(m, "G") for m in FIRST_HIT_MUTATIONS_G])
def test_a_mutated_first_hit_is_caught(luts, mutation, name):
    """The bars would see such an error in the product: the mutated reference misses the oracle's ids or planes on included pixels."""
    case, ref, got = _first_hit(luts, name)
    mutated = SC.first_hit_reference(case, mutation)
    caught = 0
    for base, (inc, same, err, bar) in zip(ref, _first_hit_errors(case, mutated, got)):
        inc = base[5] >= R.DELTA                                           # the unmutated reference says which pixels count
        bad = ~same
        for e in err.values():
            bad |= e > bar
        caught += int((bad & inc).sum())
    print(f"{mutation} on the first hit of case {name}: caught on {caught} included pixels")
    assert caught >= CAUGHT_MINIMUM


@pytest.mark.parametrize("mutation", PATH_MUTATIONS)
def test_a_mutated_shadow_alpha_test_is_caught(luts, mutation):
    m = _paths(luts, "G")
    ps = R.PathScene(m["case"].scene, mutation)
    mutated = R.concatenate([R.trace_paths(ps, cb, r) for (_, cb, _, _), r in zip(m["views"], m["rays"])])
    err = R.path_error(m["oracle"], mutated)
    inc = m["paths"].included()
    caught = int((inc & (err > R.TAU_SURFACE)).sum())
    print(f"{mutation} on the paths of case G: {caught} of {int(inc.sum())} included paths beyond tau")
    assert caught >= CAUGHT_MINIMUM


# ---------------------------------------------------------------- exact probes
def _probe_replay(scene, mutation=None):
    """(closest-hit commits, shadow visibilities, margins) of the exact probes by the reference."""
    ps = R.PathScene(scene, mutation)
    rays, _ = SC.probe_rays()
    n = len(rays)
    took = {b: np.zeros(n, bool) for b in R.BRANCHES + R.SURFACE_BRANCHES}
    margin = np.full(n, np.inf)
    o, d = np.asarray(rays["origin"], np.float64), np.asarray(rays["direction"], np.float64)
    hit, tri, *_ = ps.trace_standard(o, d, np.zeros(n), R.Rng(rays["rng"]), np.ones(n, bool), margin, took)
    on_quad = hit & (ps.mode[ps.mat_of[tri]] == S.ALPHA_MODE_MASK)
    srays, _ = SC.probe_shadow_rays()
    m2 = np.full(n, np.inf)
    vis = ps.shadow(np.asarray(srays["origin"], np.float64), np.asarray(srays["direction"], np.float64), np.asarray(srays["tmax"], np.float64),
                    np.ones(n, bool), m2, took)
    return on_quad, vis, np.minimum(margin, m2)


def test_exact_probes(luts):
    """alpha == cutoff commits (>=), cutoff = nextafter(0.5, 1) does not: the reference, the oracle's closest-hit query and its shadow
    query all answer what the texels say, with no margin to hide behind; the reference with > in place of >= does not."""
    from oracle.binding import Oracle
    scene = SC.probe_scene(luts)
    rays, commits = SC.probe_rays()
    srays, _ = SC.probe_shadow_rays()
    assert len(rays) == 28 and 4 < commits.sum() < 20
    texels = SC.alpha_map_5x3().data.view(np.float32).reshape(3, 5, 4)[..., 3]
    assert all(texels[y, x] == 0.5 for x, y in SC.HALF_TEXELS)
    on_quad, vis, margin = _probe_replay(scene)
    assert np.array_equal(on_quad, commits) and np.array_equal(vis, np.where(commits, 0.0, 1.0))
    assert (margin == 0.0).sum() == len(SC.HALF_TEXELS)                  # the half texels of the first quad sit ON the threshold
    mask_instances = np.nonzero(scene.materials["m_AlphaMode"][scene.instances["m_MaterialIndex"]] == S.ALPHA_MODE_MASK)[0]
    o = Oracle(scene)
    try:
        for k in range(len(rays)):
            ok, inst, *_ = o.trace_standard(rays["origin"][k], rays["direction"][k], 0.0, 1e10, int(rays["rng"][k]))
            assert ok and (inst in mask_instances) == commits[k], k
            assert o.shadow_query(srays["origin"][k], srays["direction"][k], float(srays["tmax"][k])) == (0.0 if commits[k] else 1.0), k
    finally:
        o.close()
    wrong, wrong_vis, _ = _probe_replay(scene, "alpha_greater_than")
    flipped = int((wrong != commits).sum())
    print(f"alpha_greater_than on the exact probes: {flipped} closest-hit and {int((wrong_vis != vis).sum())} shadow verdicts flip")
    assert flipped == len(SC.HALF_TEXELS) and (wrong_vis != vis).sum() == len(SC.HALF_TEXELS)
