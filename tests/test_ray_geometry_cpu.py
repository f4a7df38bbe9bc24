"""The hit definition against geometry, without a GPU: tests/ray_reference.py (float64 triple products + a derived forward error bound of the
fp32 watertight test) is checked against exact rational arithmetic and against deliberately wrong answers, then the oracle's BVH walk, its
brute-force loop and its visibility query are judged by it on every scene family of tests/ray_cases.py, and the inputs of the GPU tests are
shown not to pass vacuously. DESIGN.md "Hit definition: independent check"."""
from fractions import Fraction

import numpy as np
import pytest

from hobbyrenderer_amd import structs as S

import ray_cases as RC
import ray_reference as RR

f32 = np.float32
FRAMES = list(RC.SOUP_FRAMES)


# ------------------------------------------------------------------------------------------------ the reference against exact arithmetic
def _exact_pair(tri, o, d):
    """U3, V3, W3, t, u, v (None when d . n == 0) and the normal, as Fractions, for float64 arrays holding fp32 values."""
    F = lambda v: [Fraction(float(x)) for x in v]
    sub = lambda a, b: [a[k] - b[k] for k in range(3)]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    p0, p1, p2, o, d = F(tri[0]), F(tri[1]), F(tri[2]), F(o), F(d)
    A, B, C = sub(p0, o), sub(p1, o), sub(p2, o)
    U3, V3, W3 = dot(d, cross(C, B)), dot(d, cross(A, C)), dot(d, cross(B, A))
    n = cross(sub(p1, p0), sub(p2, p0))
    den = dot(d, n)
    if den == 0:
        return U3, V3, W3, None, None, None, n
    return U3, V3, W3, dot(A, n) / den, V3 / (U3 + V3 + W3), W3 / (U3 + V3 + W3), n


def _self_check_pairs():
    """(tris [m, 3, 3], o [m, 3], d [m, 3], tmin [m], tmax [m], kind [m]) as fp32: random pairs at every scale and offset of the soups, rays
    aimed at fp32 vertices and edge points, exactly coplanar pairs in oblique dyadic planes, zero-area triangles (collinear, repeated vertex)."""
    rng = np.random.default_rng(7)
    T, O, D, LO, HI, K = [], [], [], [], [], []

    def add(tri, o, d, lo, hi, kind):
        T.append(tri); O.append(o); D.append(d); LO.append(lo); HI.append(hi); K.append(kind)
    for i in range(160):
        scale, offset = list(RC.SOUP_FRAMES.values())[i % 5]
        tri = (rng.uniform(-1, 1, (3, 3)) * scale + offset).astype(f32)
        o = (rng.uniform(-2.5, 2.5, 3) * scale + offset).astype(f32)
        target = (tri.astype(np.float64) * rng.dirichlet((1, 1, 1))[:, None]).sum(0) if i % 2 else rng.uniform(-1.5, 1.5, 3) * scale + offset
        d = (target - o) * [1.0, 1e-3, 1e3][i % 3]
        t_ref = 1.0 / [1.0, 1e-3, 1e3][i % 3]
        add(tri, o, d.astype(f32), 0.0 if i % 4 else 0.5 * t_ref, 1e10 if i % 3 else t_ref * rng.uniform(0.5, 1.5), "random")
    for i in range(120):
        scale, offset = list(RC.SOUP_FRAMES.values())[i % 5]
        tri = (rng.uniform(-1, 1, (3, 3)) * scale + offset).astype(f32)
        s = [0.0, 0.5, rng.uniform()][i % 3]
        point = (tri[i % 3].astype(np.float64) * (1 - s) + tri[(i + 1) % 3].astype(np.float64) * s).astype(f32)
        o = (rng.uniform(-2.5, 2.5, 3) * scale + offset).astype(f32)
        add(tri, o, (point.astype(np.float64) - o).astype(f32), 0.0, 1e10, "edge")
    for i in range(60):                                     # oblique dyadic plane through p0 spanned by e1, e2: everything below is exact in fp32
        p0 = rng.integers(-8, 9, 3) / 4.0
        e1, e2 = rng.integers(-6, 7, 3) / 2.0, rng.integers(-6, 7, 3) / 2.0
        if not np.cross(e1, e2).any():
            e2 = e2 + [1.0, 0.0, 0.5]
        tri = np.array([p0, p0 + e1, p0 + e2])
        a, b = rng.integers(-8, 9, 2) / 4.0, rng.integers(-8, 9, 2) / 4.0
        o = p0 + a[0] * e1 + a[1] * e2
        d = b[0] * e1 + b[1] * e2
        if not d.any():
            d = e1
        add(tri.astype(f32), o.astype(f32), d.astype(f32), 0.0, 1e10, "coplanar")
    for i in range(60):
        p0, e = rng.integers(-8, 9, 3) / 4.0, rng.integers(-6, 7, 3) / 2.0
        if i % 3 == 0:
            tri = np.array([p0, p0 + e, p0 + 3 * e])       # collinear
        elif i % 3 == 1:
            tri = np.array([p0, p0 + e, p0 + e])           # repeated vertex
        else:
            tri = np.array([p0, p0, p0])                   # a point
        o = rng.uniform(-3, 3, 3)
        target = p0 + e * rng.uniform() if i % 2 else rng.uniform(-2, 2, 3)
        add(tri.astype(f32), o.astype(f32), (target - o).astype(f32), 0.0, 1e10, "zero_area")
    return (np.array(T, f32), np.array(O, f32), np.array(D, f32), np.array(LO, f32), np.array(HI, f32), np.array(K))


def test_reference_never_contradicts_exact_arithmetic():
    tris, o, d, lo, hi, kind = _self_check_pairs()
    t64, o64, d64 = tris.astype(np.float64), o.astype(np.float64), d.astype(np.float64)
    pv = RR.pair_values(t64, o64, d64)
    sign = RR.sign_class(pv)
    cls = RR.interval_class(sign, pv["t"], pv["Et"], lo.astype(np.float64), hi.astype(np.float64))
    decided = {k: 0 for k in set(kind)}
    worst = 0.0
    for i in range(len(tris)):
        U3, V3, W3, t, u, v, n = _exact_pair(t64[i], o64[i], d64[i])
        zero_area = all(c == 0 for c in n)
        coplanar = t is None and not zero_area
        assert bool(pv["zero_area"][i]) == zero_area and bool(pv["coplanar"][i]) == coplanar, (i, kind[i])
        for name, exact in (("U", U3), ("V", V3), ("W", W3)):                        # a decided sign is the exact sign
            val, err = pv[name + "s"][i], pv["E" + name][i]
            if abs(val) > err:
                assert (val > 0) == (exact > 0) and exact != 0, (i, kind[i], name)
        same_sign = (U3 > 0 and V3 > 0 and W3 > 0) or (U3 < 0 and V3 < 0 and W3 < 0)
        mixed = (U3 > 0 or V3 > 0 or W3 > 0) and (U3 < 0 or V3 < 0 or W3 < 0)
        inside = t is not None and Fraction(float(lo[i])) < t < Fraction(float(hi[i]))
        if cls[i] == RR.HIT:
            assert same_sign and inside, (i, kind[i])
            for got, exact in ((pv["t"][i], t), (pv["u"][i], u), (pv["v"][i], v)):
                rel = abs(Fraction(float(got)) - exact) / abs(exact)
                worst = max(worst, float(rel))
                assert rel <= Fraction(1, 2 ** 40), (i, kind[i], float(rel))
        elif cls[i] == RR.MISS:
            assert mixed or not inside or coplanar or zero_area, (i, kind[i])
        if np.isfinite(pv["Et"][i]) and t is not None:                                # a finite bound on t contains the exact t with room to spare
            assert abs(Fraction(float(pv["t"][i])) - t) <= Fraction(float(pv["Et"][i])) / 1024, (i, kind[i])
        decided[kind[i]] += int(cls[i] != RR.AMBIGUOUS)
    print(f"decided pairs by kind: {decided}; worst float64 relative error of t, u, v on decided hits {worst:.2e}")
    n_kind = {k: int((kind == k).sum()) for k in decided}
    assert decided["random"] >= 0.95 * n_kind["random"]                               # the bound decides what is not near an edge
    assert decided["coplanar"] == n_kind["coplanar"] and decided["zero_area"] == n_kind["zero_area"]
    assert (cls[kind == "coplanar"] == RR.MISS).all() and (cls[kind == "zero_area"] == RR.MISS).all()


def test_prefilter_only_drops_decided_misses():
    """surely_missed is a shortcut of RayTable: whatever it drops, the full evaluation calls a decided miss as well."""
    rng = np.random.default_rng(3)
    for scale, offset in RC.SOUP_FRAMES.values():
        tris = RC.soup_triangles(200, scale, offset, seed=4).astype(np.float64)
        o = (offset + scale * rng.uniform(-2.5, 2.5, (64, 3))).astype(f32).astype(np.float64)
        d = (rng.normal(size=(64, 3)) * [1.0, 1e-3, 1e3][int(rng.integers(3))]).astype(f32).astype(np.float64)
        dropped = RR.surely_missed(tris, o, d)
        cls, _ = RR.classify(tris, o, d, np.zeros(64), np.full(64, 1e10))
        assert dropped.mean() > 0.8
        assert (cls[dropped] == RR.MISS).all()


# ------------------------------------------------------------------------------------------------ the reference against wrong answers
@pytest.fixture(scope="module")
def answered(luts):
    """The unit soup with the reference's own answer for every ray (nearest decided hit), as a RayHit array, and a visibility array."""
    case = RC.soup_case(luts, "lds", "unit")
    tb = case.table
    best = tb.nearest_decided()
    hits = np.zeros(tb.n, S.RayHit)
    p = best["pos"][best["hit"]]
    hits["hit"][best["hit"]] = 1
    for f, col in (("t", tb.c_t), ("u", tb.c_u), ("v", tb.c_v)):
        hits[f][best["hit"]] = col[p].astype(f32)
    hits["instance"][best["hit"]] = tb.owner[tb.c_tri[p]]
    hits["primitive"][best["hit"]] = tb.prim[tb.c_tri[p]]
    sv = tb.shadow_view(case.rays["tmax"])
    vis = np.where(sv["n_hit"] > 0, 0.0, 1.0).astype(f32)
    return case, best, hits, vis


def test_judge_accepts_the_references_own_answer(answered):
    case, best, hits, vis = answered
    rep = case.table.judge_closest(hits)
    assert not rep, str(rep)
    assert best["hit"].sum() > 1000 and (best["runner_up"] >= 0).sum() > 300
    srep = case.table.judge_shadow(vis, case.rays["tmax"])
    assert not srep, str(srep)


def _second_nearest(case, best, hits):
    tb = case.table
    rows = np.flatnonzero(best["runner_up"] >= 0)
    p1, p2 = best["pos"][rows], best["runner_up"][rows]
    rows, p2 = rows[tb.c_t[p2] - tb.c_Et[p2] > tb.c_t[p1] + tb.c_Et[p1]], p2[tb.c_t[p2] - tb.c_Et[p2] > tb.c_t[p1] + tb.c_Et[p1]]
    r, p = rows[:5], p2[:5]
    hits["instance"][r], hits["primitive"][r] = tb.owner[tb.c_tri[p]], tb.prim[tb.c_tri[p]]
    hits["t"][r], hits["u"][r], hits["v"][r] = tb.c_t[p], tb.c_u[p], tb.c_v[p]
    return "nearer_decided_hit", r


def _hit_dropped(case, best, hits):
    r = np.flatnonzero(best["hit"])[:3]
    hits["hit"][r] = 0
    return "missed_decided_hit", r


def _miss_turned_into_hit(case, best, hits):
    tb = case.table
    vw = tb.view(tb.tmin, tb.tmax)
    r = np.flatnonzero((vw["n_hit"] == 0) & (vw["n_amb"] == 0))[:3]              # every pair a decided miss: whichever triangle is named is one
    hits["hit"][r] = 1
    hits["instance"][r], hits["primitive"][r], hits["t"][r], hits["u"][r], hits["v"][r] = 0, 7, 1.0, 0.3, 0.3
    return "hit_on_decided_miss", r


def _uv_swapped(case, best, hits):
    r = np.flatnonzero(best["hit"] & (np.abs(hits["u"] - hits["v"]) > 1e-2))[:4]
    hits["u"][r], hits["v"][r] = hits["v"][r].copy(), hits["u"][r].copy()
    return "u_beyond_bound", r


def _u_is_third_barycentric(case, best, hits):
    w = f32(1) - hits["u"] - hits["v"]
    r = np.flatnonzero(best["hit"] & (np.abs(hits["u"] - w) > 1e-2))[:4]
    hits["u"][r] = w[r]
    return "u_beyond_bound", r


def _t_moved(case, best, hits):
    tb = case.table
    r = np.flatnonzero(best["hit"])[:4]
    hits["t"][r] = (tb.c_t[best["pos"][r]] + 4 * tb.c_Et[best["pos"][r]]).astype(f32)
    return "t_beyond_bound", r


def _primitive_off_by_one(case, best, hits):
    tb = case.table
    rows = np.flatnonzero(best["hit"])
    nxt = tb.c_tri[best["pos"][rows]] + 1
    ok = (nxt < tb.T) & (tb.lookup(rows, np.minimum(nxt, tb.T - 1)) < 0)          # the next primitive exists and is a decided miss for the ray
    r = rows[ok][:4]
    hits["primitive"][r] += 1
    return "hit_on_decided_miss", r


def _primitive_out_of_range(case, best, hits):
    r = np.flatnonzero(best["hit"])[:2]
    hits["primitive"][r] = case.table.T + 5
    return "unknown_primitive", r


CLOSEST_CORRUPTIONS = [_second_nearest, _hit_dropped, _miss_turned_into_hit, _uv_swapped, _u_is_third_barycentric, _t_moved, _primitive_off_by_one,
                       _primitive_out_of_range]


@pytest.mark.parametrize("corrupt", CLOSEST_CORRUPTIONS, ids=lambda f: f.__name__.strip("_"))
def test_judge_reports_each_corruption_by_name(answered, corrupt):
    case, best, hits, _ = answered
    hits = hits.copy()
    want, rows = corrupt(case, best, hits)
    assert len(rows) > 0, "the case offers no ray to corrupt this way"
    rep = case.table.judge_closest(hits)
    assert want in rep.names(), f"{corrupt.__name__}: expected {want}, got: {rep}"
    assert rep.violations[want][0] == len(rows) and f"first ray {rows.min()}" in rep.violations[want][1], str(rep)


@pytest.mark.parametrize("to", [1.0, 0.0, 0.5], ids=["shadowed-to-lit", "lit-to-shadowed", "partial"])
def test_judge_reports_flipped_visibility(answered, to):
    case, _, _, vis = answered
    vis = vis.copy()
    r = np.flatnonzero(vis == 1.0 - to)[:3] if to != 0.5 else np.array([np.flatnonzero(vis == 0)[0], np.flatnonzero(vis == 1)[0]])
    vis[r] = to
    rep = case.table.judge_shadow(vis, case.rays["tmax"])
    want = {1.0: {"lit_through_decided_hit"}, 0.0: {"dark_without_hit"}, 0.5: {"lit_through_decided_hit", "dark_without_hit"}}[to]
    assert rep.names() == want, str(rep)


def test_judge_applies_key_order_to_exact_ties(luts):
    """Two coincident dyadic triangles: equal float64 t, so (instance, primitive) decides; and either passes once their t differ."""
    import bvh_scenes
    tri = np.array([[-1, -1, 2], [3, -1, 2], [-1, 3, 2]], f32)
    sc = bvh_scenes.triangle_scene(luts, np.array([tri, tri, tri + f32(0.5)]))
    rays = np.zeros(1, S.Ray); rays["direction"] = (0, 0, 1); rays["tmax"] = 1e10
    tb = RC.Case("tie", sc, rays, "tie").table
    hits = np.zeros(1, S.RayHit); hits["hit"] = 1; hits["t"] = 2.0; hits["u"] = 0.25; hits["v"] = 0.25
    assert not tb.judge_closest(hits)
    hits["primitive"] = 1
    assert tb.judge_closest(hits).names() == {"tie_order"}
    hits["primitive"] = 2; hits["t"] = 2.5
    assert tb.judge_closest(hits).names() == {"nearer_decided_hit", "u_beyond_bound", "v_beyond_bound"}


# ------------------------------------------------------------------------------------------------ the oracle against the reference
def _oracle_hits(o, rays, brute_force):
    hits = np.zeros(len(rays), S.RayHit)
    for i, r in enumerate(rays):
        h = o.trace_closest(r["origin"], r["direction"], float(r["tmin"]), float(r["tmax"]), brute_force=brute_force)
        if h is not None:
            hits[i]["hit"] = 1
            hits[i]["instance"], hits[i]["primitive"], hits[i]["u"], hits[i]["v"], hits[i]["t"] = h
    return hits


def _judge_oracle(case, watertight=False):
    from oracle.binding import Oracle
    o = Oracle(case.scene)
    try:
        walk, brute = _oracle_hits(o, case.rays, False), _oracle_hits(o, case.rays, True)
        vis = np.array([o.shadow_query(r["origin"], r["direction"], float(r["tmax"])) for r in case.rays], f32)
    finally:
        o.close()
    assert np.array_equal(walk.view(np.uint8), brute.view(np.uint8)), case.name
    rep = case.table.judge_closest(walk)
    srep = case.table.judge_shadow(vis, case.rays["tmax"])
    print(f"{case.name}: {rep.stats} vacuous {rep.vacuous_share:.4f} bounded {rep.bounded_share:.4f} headroom {rep.headroom}; "
          f"shadow {srep.stats} unjudged {srep.unjudged_share:.4f}")
    assert not rep, f"{case.name}: {rep}"
    assert not srep, f"{case.name}: {srep}"
    if watertight:
        assert walk["hit"].all(), f"{case.name}: {int((walk['hit'] == 0).sum())} rays leave the closed mesh, first {int(np.argmin(walk['hit']))}"
        assert (vis == 0).all(), f"{case.name}: {int((vis != 0).sum())} shadow rays leave the closed mesh, first {int(np.argmax(vis != 0))}"
    return rep, srep


@pytest.mark.parametrize("frame", FRAMES)
def test_oracle_on_soups(luts, frame):
    _judge_oracle(RC.soup_case(luts, "lds", frame))


@pytest.mark.parametrize("frame", FRAMES)
def test_oracle_on_edges_and_vertices(luts, frame):
    _judge_oracle(RC.edge_case(luts, "lds", frame))


@pytest.mark.parametrize("offset,moved", [(0.0, False), (1e3, False), (0.0, True)], ids=["origin", "offset1e3", "moved"])
def test_oracle_closed_mesh_is_watertight(luts, offset, moved):
    _judge_oracle(RC.closed_case(luts, offset, moved), watertight=True)


def test_oracle_primary_rays_inside_closed_mesh(luts):
    _judge_oracle(RC.gbuffer_case(luts)[2], watertight=True)


def test_oracle_axis_parallel_and_denormal_directions(luts):
    _judge_oracle(RC.axis_case(luts))


@pytest.mark.parametrize("which", ["planar", "zero_area"])
def test_oracle_degenerate_sets(luts, which):
    case = RC.degenerate_case(luts, which)
    rep, _ = _judge_oracle(case)
    if which == "planar":
        in_plane = (case.rays["direction"][:, 1] == 0) & (case.rays["origin"][:, 1] == f32(0.25))
        assert in_plane.sum() == 300 and rep.stats["hits"] == 0           # every pair is a decided miss here: a hit would be in the report, too
    else:
        assert rep.stats["hits"] > 100


def test_interval_ends_are_exact(luts):
    """The rational check of the construction (t == 2 exactly, the edge functions sum to +-16), then the oracle on the interval ends."""
    from oracle.binding import Oracle
    import bvh_reference
    sc = RC.interval_scene(luts)
    rays, want, label = RC.interval_rays()
    tris = bvh_reference.expected_triangles(sc)["pos"].astype(np.float64)
    for i in range(0, len(rays), 8):
        hit_some = 0
        for tri in tris:
            U3, V3, W3, t, u, v, n = _exact_pair(tri, rays["origin"][i].astype(np.float64), rays["direction"][i].astype(np.float64))
            if t is not None and ((U3 > 0 and V3 > 0 and W3 > 0) or (U3 < 0 and V3 < 0 and W3 < 0)):
                assert t == 2 and abs(U3 + V3 + W3) == 16, label[i]
                hit_some += 1
        assert hit_some == 2, label[i]                                  # the triangle and its reversed copy
    o = Oracle(sc)
    try:
        for brute in (False, True):
            got = _oracle_hits(o, rays, brute)
            bad = np.flatnonzero((got["hit"] != 0) != want)
            assert len(bad) == 0, [label[i] for i in bad]
            assert (got["t"][want] == 2.0).all() and (got["primitive"][want] % 2 == 0).all()
    finally:
        o.close()


def test_oracle_non_finite_and_zero_rays(luts):
    from oracle.binding import Oracle
    sc = RC.soup_scene(luts, "lds", "unit")
    rays = RC.nonfinite_rays()
    case = RC.Case("non-finite", sc, rays, "nonfinite")
    assert case.table.degenerate.all()
    o = Oracle(sc)
    try:
        for brute in (False, True):
            assert (_oracle_hits(o, rays, brute)["hit"] == 0).all()
        assert all(o.shadow_query(r["origin"], r["direction"], 1e10) == 1.0 for r in rays)
    finally:
        o.close()


# ------------------------------------------------------------------------------------------------ the inputs cannot pass by being vacuous
@pytest.mark.parametrize("size", list(RC.SOUP_SIZES))
@pytest.mark.parametrize("frame", FRAMES)
def test_gpu_inputs_are_not_vacuous(luts, size, frame):
    """The caps of the GPU tests, from the reference and the inputs alone: at most 1 % vacuous rays and 2 % unjudged shadow queries for the
    interior-aimed / random rays; a decided bound for at least 95 % of the edge and vertex rays."""
    case = RC.soup_case(luts, size, frame)
    _, vacuous, bounded = case.table.closest_vacuity()
    unjudged = case.table.shadow_unjudged_share(case.rays["tmax"])
    sv = case.table.shadow_view(case.rays["tmax"])
    print(f"{case.name}: vacuous {vacuous:.4f} decided-hit rays {bounded:.3f} shadow unjudged {unjudged:.4f} shadowed {(sv['n_hit'] > 0).mean():.3f}")
    assert vacuous <= 0.01 and unjudged <= 0.02
    assert 0.3 < bounded < 0.95 and 0.1 < (sv["n_hit"] > 0).mean() < 0.9          # hits and misses, shadowed and lit, both well represented
    assert case.table.slivers == 0
    edges = RC.edge_case(luts, size, frame)
    _, e_vacuous, e_bounded = edges.table.closest_vacuity()
    print(f"{edges.name}: ambiguous-front rays {e_vacuous:.4f} decided bound {e_bounded:.4f}")
    assert e_bounded >= 0.95
    assert e_vacuous >= 0.05                                                       # the family does reach the edges
