"""Geometric reference for ray / triangle hits, numpy float64 -- TEST INFRASTRUCTURE.

It shares no code and no arithmetic with the product or with oracle/pt_oracle.c: inputs are the fp32 world-space triangles of
bvh_reference.expected_triangles(scene) and fp32 rays, both converted EXACTLY to float64; everything below is float64 (and, for two exact
yes/no questions on a sliver of pairs, Python integers through fractions.Fraction). No float32 operation is performed here.

What is computed for a pair (ray o, d, tmin, tmax; triangle p0, p1, p2), with A = p0 - o, B = p1 - o, C = p2 - o:

    U3 = d . (C x B)      V3 = d . (A x C)      W3 = d . (B x A)          the signed edge functions (scalar triple products)
    n = (p1 - p0) x (p2 - p0),   t = (A . n) / (d . n)                    the plane equation
    u = V3 / (U3 + V3 + W3),     v = W3 / (U3 + V3 + W3)                  the barycentrics of p1 and p2 (DXR convention)

The fp32 test under judgement (tri_test / make_shear in csrc/pt_traverse.h, restated in the oracle) picks kz = the axis of the largest
|d| component, kx, ky the other two, and works on sheared coordinates: with S = (d_kx / d_kz, d_ky / d_kz, 1 / d_kz) and a = A permuted,

    Ax = a_x - Sx a_z,  Ay = a_y - Sy a_z,  Az = Sz a_z      (B, C alike)
    U = Cx By - Cy Bx,  V = Ax Cy - Ay Cx,  W = Bx Ay - By Ax,  det = (U + V) + W,  T = (U Az + V Bz) + W Cz
    rcp = 1 / det,  t = T rcp,  u = V rcp,  v = W rcp;   rejected when U, V, W have mixed strict signs, det == 0 or !(tmin < t < tmax).

In exact arithmetic U = U3 / |d_kz| (the kx / ky swap for d_kz < 0 makes the sign that of the triple product for either direction of d_kz),
and likewise V, W, so the comparison is made in those "sheared units": Us = U3 / |d_kz|.

FORWARD ERROR BOUND of the fp32 evaluation (derived, not measured). Standard model: every fp32 operation returns x (1 + delta) + eps with
|delta| <= u = 2^-24 and |eps| <= eta = 2^-149 (gradual underflow: both builds keep denormals; eps = 0 for sums and differences).
First order in u; magnitudes are the float64 values of the same quantities. Written for A, alike for B and C:

    a_x = fl(p0_x - o_x):                          error <= u |a_x|
    Sx = fl(d_kx / d_kz):                          error <= u |Sx| + eta
    fl(Sx a_z):   three relative errors (Sx, a_z, the product) and the underflows:   <= 3u |Sx a_z| + eta (|a_z| + 1)
    Ax = fl(a_x - fl(Sx a_z)):                     the two above + u |Ax| <= u (|a_x| + |Sx a_z|)
        E(Ax) = u (2 |a_x| + 4 |Sx a_z|) + eta (|a_z| + 1)                                  (E(Ay) with Sy and a_y)
    Az = fl(Sz a_z) with Sz = fl(1 / d_kz):        E(Az) = 3u |Az| + eta (|a_z| + 1)
    U = fl(fl(Cx By) - fl(Cy Bx)):  each product carries the errors of its factors, u of itself and eta; the difference u |U| <= u (sum):
        E(U) = |By| E(Cx) + |Cx| E(By) + |Bx| E(Cy) + |Cy| E(Bx) + 2u (|Cx||By| + |Cy||Bx|) + 2 eta      (V, W by rotating A, B, C)
    det = fl(fl(U + V) + W):        E(det) = E(U) + E(V) + E(W) + 2u (|U| + |V| + |W|)
    T = fl(fl(fl(U Az) + fl(V Bz)) + fl(W Cz)):  three products (u each), two sums (u of at most the magnitude sum each):
        E(T) = sum over (U, Az), (V, Bz), (W, Cz) of [E(U) |Az| + |U| E(Az)] + 3u (|U Az| + |V Bz| + |W Cz|) + 3 eta
    t = fl(T fl(1 / det)):  T'/det' - T/det = (dT - t ddet) / det' with |det'| >= |det| - E(det) (not linearised: the bound is infinite, and
        the pair's t undecided, when det is not decided to be non-zero), then two roundings and one underflow:
        E(t) = (E(T) + |t| E(det)) / (|det| - E(det)) + 2u |t| + eta
        E(u) = (E(V) + |u| E(det)) / (|det| - E(det)) + 2u |u| + eta          E(v) with W

Every E above is then MULTIPLIED BY 2 for the neglected higher-order terms (the denominator |det| - E(det) uses the doubled E(det)).
To each bound the rounding of this module's own float64 evaluation is added: 2^-50 times the magnitude sum of the float64 expression (six
products per triple product, three per dot product), about 2^-26 of the fp32 terms. The bound is a function of the inputs only; it
contains no constant fitted to any implementation. It holds for whichever order a compiler evaluates the commutative products in, and does
not assume that the differences p - o are exact (they often are, by Sterbenz' lemma; the bound does not use it).

CLASSIFICATION of a pair
    decided hit:   Us, Vs, Ws all beyond their bounds with one sign, and tmin < t - E(t), t + E(t) < tmax.
    decided miss:  two of Us, Vs, Ws beyond their bounds with opposite signs; or t + E(t) < tmin or t - E(t) > tmax (E(t) finite); or the ray
                   exactly parallel to the triangle's plane (d . n == 0: in the plane or beside it), or the triangle of exactly zero area (n == 0). The last two are exact
                   questions: float64 answers "no" whenever |x| exceeds its own rounding bound, and on the sliver where it does not they are
                   settled in integer arithmetic (Fraction); beyond `exact_budget` such pairs in one call the rest stay ambiguous.
                   A ray with a non-finite component, or with direction (0, 0, 0), makes S or a non-finite: every pair is a decided miss
                   (fp32: NaN compares false, and an infinite d_kz gives Sz = 0, t = 0, never above tmin >= 0).
    ambiguous:     everything else.

VERDICTS (judge_closest / judge_shadow) are spelled out at those functions; they return a bvh_reference.Report of named violations.
"""
from fractions import Fraction

import numpy as np

from bvh_reference import Report

U = 2.0 ** -24
ETA = 2.0 ** -149
EPS64 = 2.0 ** -50
HIT, MISS, AMBIGUOUS = 1, 0, 2
SHADOW_BIAS = float(np.float32(0.01))          # kShadowBias, an fp32 constant of the query (CommonLighting.hlsli:380-496)


def _f64(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, "the reference takes the fp32 inputs of the kernels and widens them exactly"
    return a.astype(np.float64)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _abs_cross(a, b):
    """Magnitude sum of the six products of a cross product, per component."""
    a, b = np.abs(a), np.abs(b)
    return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1)


def shear_axes(d):
    """(kx, ky, kz) of make_shear for float64 directions [n, 3]: comparisons of exact values only. The kx / ky swap for a negative d_kz only
    exchanges names in the bound (it is symmetric in x and y) and the signs come from the triple products, so it is not restated."""
    ad = np.abs(d)
    kz = np.zeros(len(d), np.int64)
    kz = np.where(ad[:, 1] > ad[np.arange(len(d)), kz], 1, kz)
    kz = np.where(ad[:, 2] > ad[np.arange(len(d)), kz], 2, kz)
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    return kx, ky, kz


def _frac3(v):
    return [Fraction(float(x)) for x in v]


def _exact_normal(tri):
    p0, p1, p2 = (_frac3(tri[k]) for k in range(3))
    e1 = [p1[k] - p0[k] for k in range(3)]
    e2 = [p2[k] - p0[k] for k in range(3)]
    return [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]


def pair_values(tris, o, d, exact_budget=200000):
    """One row per PAIR: tris float64 [m, 3, 3]; o, d float64 [m, 3] (finite, d != 0). Returns a dict of [m] arrays: Us, Vs, Ws, EU, EV, EW
    (sheared units), det, Edet, t, Et, u, Eu, v, Ev, and the exact flags `coplanar`, `zero_area`, `sliver` (an exact question left open: over
    the budget)."""
    m = len(o)
    P = tris - o[:, None, :]                                            # [m, vertex, xyz]
    A, B, C = P[:, 0], P[:, 1], P[:, 2]
    kx, ky, kz = shear_axes(d)
    rows = np.arange(m)
    dz = d[rows, kz]
    adz = np.abs(dz)
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    with np.errstate(all="ignore"):
        U3 = (d * _cross(C, B)).sum(-1); V3 = (d * _cross(A, C)).sum(-1); W3 = (d * _cross(B, A)).sum(-1)
        m3 = lambda p, q: (np.abs(d) * _abs_cross(p, q)).sum(-1)
        Us, Vs, Ws = U3 / adz, V3 / adz, W3 / adz
        e64U, e64V, e64W = EPS64 * m3(C, B) / adz, EPS64 * m3(A, C) / adz, EPS64 * m3(B, A) / adz
        # sheared magnitudes
        Sx, Sy, Sz = (d[rows, kx] / dz)[:, None], (d[rows, ky] / dz)[:, None], (1.0 / dz)[:, None]
        perm = np.stack([kx, ky, kz], 1)
        Pk = np.take_along_axis(P, np.broadcast_to(perm[:, None, :], P.shape), axis=2)
        ax, ay, az = Pk[..., 0], Pk[..., 1], Pk[..., 2]                  # [m, vertex]
        X, Y, Z = ax - Sx * az, ay - Sy * az, Sz * az
        under = ETA * (np.abs(az) + 1.0)
        EX = U * (2 * np.abs(ax) + 4 * np.abs(Sx * az)) + under
        EY = U * (2 * np.abs(ay) + 4 * np.abs(Sy * az)) + under
        EZ = 3 * U * np.abs(Z) + under
        aX, aY, aZ = np.abs(X), np.abs(Y), np.abs(Z)

        def edge(i, j):         # fl(X_i Y_j - Y_i X_j)
            return (aY[..., j] * EX[..., i] + aX[..., i] * EY[..., j] + aX[..., j] * EY[..., i] + aY[..., i] * EX[..., j]
                    + 2 * U * (aX[..., i] * aY[..., j] + aY[..., i] * aX[..., j]) + 2 * ETA)
        EU1, EV1, EW1 = edge(2, 1), edge(0, 2), edge(1, 0)
        aU, aV, aW = np.abs(Us), np.abs(Vs), np.abs(Ws)
        det = (Us + Vs) + Ws
        Edet1 = EU1 + EV1 + EW1 + 2 * U * (aU + aV + aW)
        ET1 = (EU1 * aZ[..., 0] + EV1 * aZ[..., 1] + EW1 * aZ[..., 2] + aU * EZ[..., 0] + aV * EZ[..., 1] + aW * EZ[..., 2]
               + 3 * U * (aU * aZ[..., 0] + aV * aZ[..., 1] + aW * aZ[..., 2]) + 3 * ETA)
        EU, EV, EW = 2 * EU1 + e64U, 2 * EV1 + e64V, 2 * EW1 + e64W
        Edet = 2 * Edet1 + (e64U + e64V + e64W)
        # plane equation
        nrm = _cross(e1, e2)
        mag_n = _abs_cross(e1, e2)
        num = (A * nrm).sum(-1); den = (d * nrm).sum(-1)
        mnum = (np.abs(A) * mag_n).sum(-1); mden = (np.abs(d) * mag_n).sum(-1)
        t = num / den
        u, v = V3 / (U3 + V3 + W3), W3 / (U3 + V3 + W3)
        room = np.abs(det) - Edet
        room = np.where(room > 0, room, np.nan)
        e64t = 4 * EPS64 * (mnum + np.abs(t) * mden) / np.abs(den)
        Et = 2 * ((ET1 + np.abs(t) * Edet1) / room + 2 * U * np.abs(t) + ETA) + e64t
        Eu = 2 * ((EV1 + np.abs(u) * Edet1) / room + 2 * U * np.abs(u) + ETA) + 4 * EPS64 * np.abs(u)
        Ev = 2 * ((EW1 + np.abs(v) * Edet1) / room + 2 * U * np.abs(v) + ETA) + 4 * EPS64 * np.abs(v)
        Et, Eu, Ev = (np.where(np.isfinite(x), x, np.inf) for x in (Et, Eu, Ev))
        t = np.where(np.isfinite(t), t, 0.0); u = np.where(np.isfinite(u), u, 0.0); v = np.where(np.isfinite(v), v, 0.0)
    # the two exact questions, asked only where float64 cannot answer "no"
    zero_area = np.zeros(m, bool); coplanar = np.zeros(m, bool); sliver = np.zeros(m, bool)
    maybe_flat = (np.abs(nrm) <= 4 * EPS64 * mag_n).all(1)
    maybe = np.flatnonzero(maybe_flat | (np.abs(den) <= 8 * EPS64 * mden))
    sliver[maybe[exact_budget:]] = True
    for i in maybe[:exact_budget]:
        n_exact = _exact_normal(tris[i])
        if all(c == 0 for c in n_exact):
            zero_area[i] = True
        else:
            fd = _frac3(d[i])
            coplanar[i] = (fd[0] * n_exact[0] + fd[1] * n_exact[1] + fd[2] * n_exact[2]) == 0
    return dict(Us=Us, Vs=Vs, Ws=Ws, EU=EU, EV=EV, EW=EW, det=det, Edet=Edet, t=t, Et=Et, u=u, Eu=Eu, v=v, Ev=Ev,
                coplanar=coplanar, zero_area=zero_area, sliver=sliver)


def surely_missed(tris, o, d):
    """Dense prefilter [n, T] (bool): pairs that are decided misses by two edge functions of opposite sign under a COARSER bound than
    pair_values', so that only the few others need the full evaluation. With c a point of the scene, p' = p - c, o' = o - c:
        U3 = d . ((pc - o) x (pb - o)) = d . (pc' x pb') + (d x o') . (pc' - pb')          two matrix products per edge function,
    its float64 rounding is below 2^-48 times the same expression over magnitudes, and since |Sx|, |Sy| <= 1 (kz is the largest axis)
    |X|, |Y| <= 2 M and E(X), E(Y) <= 6u M + eta (M + 1) for M = |p - o|_inf <= |p'|_inf + |o'|_inf, the doubled E(U) of the module docstring
    is at most 128u Mb Mc + eta (16 Mb Mc + 8 Mb + 8 Mc + 4)."""
    c = tris.reshape(-1, 3).mean(0).astype(np.float32).astype(np.float64) if len(tris) else np.zeros(3)
    tp, op = tris - c, o - c
    _, _, kz = shear_axes(d)
    adz = np.abs(d[np.arange(len(d)), kz])[:, None]
    dxo, adxo, ad = _cross(d, op), _abs_cross(d, op), np.abs(d)
    r, far = np.abs(tp).max(2), np.abs(op).max(1)                    # [T, vertex], [n]
    pos = np.zeros((len(o), len(tris)), np.int8); neg = np.zeros_like(pos)
    for i, j in ((2, 1), (0, 2), (1, 0)):
        g, ag, e = _cross(tp[:, i], tp[:, j]), _abs_cross(tp[:, i], tp[:, j]), tp[:, i] - tp[:, j]
        val = d @ g.T + dxo @ e.T
        mag = ad @ ag.T + adxo @ np.abs(e).T
        Mi, Mj = far[:, None] + r[None, :, i], far[:, None] + r[None, :, j]
        bound = (128 * U * Mi * Mj + ETA * (16 * Mi * Mj + 8 * Mi + 8 * Mj + 4)) * adz + 4 * EPS64 * mag
        pos += val > bound
        neg += val < -bound
    return (pos >= 1) & (neg >= 1)


def sign_class(pv):
    """Per pair from the edge functions and the exact flags alone (no interval yet): HIT = one decided sign, MISS, AMBIGUOUS."""
    pos = (pv["Us"] > pv["EU"]).astype(np.int8) + (pv["Vs"] > pv["EV"]) + (pv["Ws"] > pv["EW"])
    neg = (pv["Us"] < -pv["EU"]).astype(np.int8) + (pv["Vs"] < -pv["EV"]) + (pv["Ws"] < -pv["EW"])
    cls = np.full(pos.shape, AMBIGUOUS, np.int8)
    cls[(pos == 3) | (neg == 3)] = HIT
    cls[(pos >= 1) & (neg >= 1)] = MISS
    cls[(pv["coplanar"] | pv["zero_area"]) & (cls != HIT)] = MISS
    return cls


def interval_class(sign, t, Et, tmin, tmax, tmax_err=0.0):
    """Adds the interval: a sign-HIT becomes HIT only with t decidedly inside; anything with t decidedly outside becomes MISS."""
    with np.errstate(invalid="ignore"):
        inside = (t - Et > tmin) & (t + Et < tmax - tmax_err)
        outside = np.isfinite(Et) & ((t + Et < tmin) | (t - Et > tmax + tmax_err))
        empty = np.broadcast_to(~(np.asarray(tmax) + tmax_err > tmin), np.shape(t))       # tmin >= tmax: no t passes (also NaN ends)
    cls = np.where(sign == MISS, MISS, np.where(outside | empty, MISS, np.where((sign == HIT) & inside, HIT, AMBIGUOUS)))
    return cls.astype(np.int8)


def classify(tris, o, d, tmin, tmax):
    """Dense classification [n, T] of a few pairs (the self-checks): returns (cls, pair values as [n, T] arrays)."""
    n, T = len(o), len(tris)
    i, k = np.repeat(np.arange(n), T), np.tile(np.arange(T), n)
    pv = {name: a.reshape(n, T) for name, a in pair_values(tris[k], o[i], d[i]).items()}
    cls = interval_class(sign_class(pv), pv["t"], pv["Et"], np.asarray(tmin, np.float64)[:, None], np.asarray(tmax, np.float64)[:, None])
    return cls, pv


class RayTable:
    """The reference of one case: for rays [n] against all triangles of a scene, every pair that is not a decided miss by its edge functions
    (the candidates: a few per ray), with t, u, v and their bounds. Interval-independent, so closest-hit and shadow verdicts of every kernel
    variant are read off one table. O(n T) float64 work, chunked."""

    def __init__(self, scene_tris, rays, chunk_pairs=2000000):
        self.owner = np.asarray(scene_tris["owner"], np.int64)
        self.prim = np.asarray(scene_tris["prim"], np.int64)
        self.key = self.owner << 32 | self.prim                              # expected_triangles lists them in (owner, primitive) order
        assert (np.diff(self.key) > 0).all()
        tris = _f64(scene_tris["pos"])
        self.T = T = len(tris)
        self.n = n = len(rays)
        o, d = _f64(rays["origin"]), _f64(rays["direction"])
        self.tmin, self.tmax = _f64(rays["tmin"]), _f64(rays["tmax"])
        self.degenerate = ~(np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1))
        cols = {k: [] for k in ("ray", "tri", "decided", "t", "Et", "u", "Eu", "v", "Ev")}
        self.slivers = 0
        good = np.flatnonzero(~self.degenerate)
        step = max(1, chunk_pairs // max(T, 1))
        for s in range(0, len(good), step):
            sel = good[s:s + step]
            i, k = np.nonzero(~surely_missed(tris, o[sel], d[sel]))
            pv = pair_values(tris[k], o[sel[i]], d[sel[i]])
            sc = sign_class(pv)
            self.slivers += int(pv["sliver"].sum())
            keep = sc != MISS
            cols["ray"].append(sel[i][keep]); cols["tri"].append(k[keep]); cols["decided"].append(sc[keep] == HIT)
            for name in ("t", "Et", "u", "Eu", "v", "Ev"):
                cols[name].append(pv[name][keep])
        for name, parts in cols.items():
            setattr(self, "c_" + name, np.concatenate(parts) if parts else np.zeros(0))
        self.c_ray = self.c_ray.astype(np.int64); self.c_tri = self.c_tri.astype(np.int64); self.c_decided = self.c_decided.astype(bool)
        self.c_key = self.c_ray * T + self.c_tri                              # ascending: chunks are in ray order, nonzero() is row-major
        assert (np.diff(self.c_key) > 0).all()

    # -------------------------------------------------------------------------------------------------------------------- views
    def view(self, tmin, tmax, tmax_err=0.0):
        """Per candidate HIT / MISS / AMBIGUOUS for the interval (tmin, tmax) per ray, and per ray the summaries the verdicts need."""
        r = self.c_ray
        tmin = np.broadcast_to(np.asarray(tmin, np.float64), (self.n,)); tmax = np.broadcast_to(np.asarray(tmax, np.float64), (self.n,))
        terr = np.broadcast_to(np.asarray(tmax_err, np.float64), (self.n,))
        cls = interval_class(np.where(self.c_decided, HIT, AMBIGUOUS), self.c_t, self.c_Et, tmin[r], tmax[r], terr[r])
        hi = np.where(cls == HIT, self.c_t + self.c_Et, np.inf)
        with np.errstate(invalid="ignore"):
            lo_amb = np.where(cls == AMBIGUOUS, np.where(np.isfinite(self.c_Et), self.c_t - self.c_Et, -np.inf), np.inf)
        n = self.n
        best_hi = np.full(n, np.inf); np.minimum.at(best_hi, r, hi)
        # the runner-up (another triangle): mask the first minimum of each ray and reduce again
        first = np.full(n, -1, np.int64)
        is_best = (hi == best_hi[r]) & np.isfinite(hi)
        pos = np.flatnonzero(is_best)
        first[r[pos[::-1]]] = pos[::-1]                                        # lowest position wins
        hi2 = hi.copy(); hi2[first[first >= 0]] = np.inf
        second_hi = np.full(n, np.inf); np.minimum.at(second_hi, r, hi2)
        best_tri = np.where(first >= 0, self.c_tri[np.maximum(first, 0)], -1) if len(self.c_tri) else first
        amb_lo = np.full(n, np.inf); np.minimum.at(amb_lo, r, lo_amb)
        n_hit = np.bincount(r[cls == HIT], minlength=n)
        n_amb = np.bincount(r[cls == AMBIGUOUS], minlength=n)
        return dict(cls=cls, best_hi=best_hi, second_hi=second_hi, best_tri=best_tri, amb_lo=amb_lo, n_hit=n_hit, n_amb=n_amb)

    def lookup(self, ray, tri):
        """Position of the candidates (ray, tri), -1 where the pair is a decided miss."""
        key = np.asarray(ray, np.int64) * self.T + np.asarray(tri, np.int64)
        p = np.searchsorted(self.c_key, key)
        p = np.minimum(p, max(len(self.c_key) - 1, 0))
        found = (self.c_key[p] == key) if len(self.c_key) else np.zeros(len(key), bool)
        return np.where(found, p, -1)

    def triangle_of(self, instance, primitive):
        """Index of the triangle (instance, primitive) owns, -1 when there is none."""
        key = np.asarray(instance, np.int64) << 32 | np.asarray(primitive, np.int64)
        p = np.minimum(np.searchsorted(self.key, key), self.T - 1)
        return np.where(self.key[p] == key, p, -1)

    def nearest_decided(self, view=None):
        """The reference's own answer where it has one: per ray the decided hit of smallest float64 t (ties by (instance, primitive)), as a
        dict of hit (bool), tri, t, u, v -- and `runner_up`, the decided hit after it (-1 without). Feeds the corruption tests."""
        view = view or self.view(self.tmin, self.tmax)
        sel = np.flatnonzero(view["cls"] == HIT)
        order = sel[np.lexsort((self.c_tri[sel], self.c_t[sel], self.c_ray[sel]))]
        r = self.c_ray[order]
        start = np.flatnonzero(np.concatenate([[True], r[1:] != r[:-1]])) if len(r) else np.zeros(0, np.int64)
        out = dict(hit=np.zeros(self.n, bool), pos=np.full(self.n, -1, np.int64), runner_up=np.full(self.n, -1, np.int64))
        out["hit"][r[start]] = True
        out["pos"][r[start]] = order[start]
        nxt = start + 1
        ok = (nxt < len(r)) & (r[np.minimum(nxt, len(r) - 1)] == r[start]) if len(r) else np.zeros(0, bool)
        out["runner_up"][r[start][ok]] = order[nxt[ok]]
        return out

    # -------------------------------------------------------------------------------------------------------------------- verdicts
    def judge_closest(self, hits, tmin=None, tmax=None):
        """Verdict on closest-hit records (S.RayHit fields hit, instance, primitive, t, u, v) over opaque geometry.

        missed_decided_hit     a miss is reported and some pair of the ray is a decided hit
        unknown_primitive      (instance, primitive) names no triangle of the scene
        hit_on_decided_miss    the reported triangle is a decided miss for the ray
        t_beyond_bound, u_beyond_bound, v_beyond_bound     reported value further than E(.) from the pair's float64 value (finite bounds only)
        nearer_decided_hit     another triangle is a decided hit with t + E(t) < reported t
        tie_order              the reported triangle and another decided hit have EQUAL float64 t and the other has the smaller (instance, primitive)
        hit_on_degenerate_ray  a hit is reported for a ray with a non-finite component or a zero direction
        Two decided hits with overlapping t intervals and different float64 t: either passes.

        The returned Report carries .vacuous (bool per ray: an ambiguous pair is, or may be, at or in front of the nearest decided hit -- or no
        pair is decided -- so the verdict could not have failed on the winner), .vacuous_share, .bounded_share (rays with a decided hit: an upper
        bound on what may be reported) and .headroom (largest |reported - float64| / bound for t, u, v over the reported decided hits)."""
        rep = Report()
        tmin = self.tmin if tmin is None else tmin
        tmax = self.tmax if tmax is None else tmax
        vw = self.view(tmin, tmax)
        n = self.n
        assert len(hits) == n
        hit = hits["hit"] != 0
        where = lambda i: f"ray {i}"
        rep.flag("hit_on_degenerate_ray", hit & self.degenerate, "rays", where)
        rep.flag("missed_decided_hit", ~hit & (vw["n_hit"] > 0), "rays", where)
        rows = np.flatnonzero(hit & ~self.degenerate)
        k = self.triangle_of(hits["instance"][rows], hits["primitive"][rows])
        bad = np.zeros(n, bool); bad[rows[k < 0]] = True
        rep.flag("unknown_primitive", bad, "rays", where)
        rows, k = rows[k >= 0], k[k >= 0]
        p = self.lookup(rows, k)
        status = np.where(p >= 0, vw["cls"][np.maximum(p, 0)], MISS) if len(vw["cls"]) else np.full(len(rows), MISS)
        bad = np.zeros(n, bool); bad[rows[status == MISS]] = True
        rep.flag("hit_on_decided_miss", bad, "rays", where)
        keep = status != MISS
        rows, k, p, status = rows[keep], k[keep], p[keep], status[keep]
        rt, ru, rv = (hits[f][rows].astype(np.float64) for f in ("t", "u", "v"))
        headroom = {}
        for name, got, ref, err in (("t", rt, self.c_t[p], self.c_Et[p]), ("u", ru, self.c_u[p], self.c_Eu[p]), ("v", rv, self.c_v[p], self.c_Ev[p])):
            fin = np.isfinite(err)
            with np.errstate(invalid="ignore"):
                off = np.abs(got - ref)
                bad = np.zeros(n, bool); bad[rows[fin & ~(off <= err)]] = True
            rep.flag(name + "_beyond_bound", bad, "rays", where)
            dec = fin & (status == HIT) & (err > 0)
            headroom[name] = float((off[dec] / err[dec]).max()) if dec.any() else 0.0
        other_hi = np.where(vw["best_tri"][rows] == k, vw["second_hi"][rows], vw["best_hi"][rows])
        bad = np.zeros(n, bool); bad[rows[other_hi < rt]] = True
        rep.flag("nearer_decided_hit", bad, "rays", where)
        # exact ties among decided hits: sorted by (ray, t, triangle), an entry whose predecessor has the same ray and t loses the tie
        sel = np.flatnonzero(vw["cls"] == HIT)
        order = sel[np.lexsort((self.c_tri[sel], self.c_t[sel], self.c_ray[sel]))]
        loses = np.zeros(len(self.c_key), bool)
        if len(order) > 1:
            same = (self.c_ray[order][1:] == self.c_ray[order][:-1]) & (self.c_t[order][1:] == self.c_t[order][:-1])
            loses[order[1:][same]] = True
        bad = np.zeros(n, bool); bad[rows[(status == HIT) & loses[p]]] = True
        rep.flag("tie_order", bad, "rays", where)
        rep.vacuous, rep.vacuous_share, rep.bounded_share = self.closest_vacuity(vw)
        rep.headroom = headroom
        rep.stats.update(rays=n, hits=int(hit.sum()), decided_rays=int((vw["n_hit"] > 0).sum()))
        return rep

    def closest_vacuity(self, vw=None):
        """(vacuous per ray, its share, share of rays with a decided hit) for the rays' own intervals: from the inputs alone."""
        vw = vw or self.view(self.tmin, self.tmax)
        vac = ~self.degenerate & (vw["n_amb"] > 0) & (vw["amb_lo"] <= vw["best_hi"])
        return vac, float(vac.mean()) if self.n else 0.0, float((vw["n_hit"] > 0).mean()) if self.n else 0.0

    def shadow_unjudged_share(self, max_dist):
        vw = self.shadow_view(max_dist)
        return float(((vw["n_hit"] == 0) & (vw["n_amb"] > 0) & ~self.degenerate).mean()) if self.n else 0.0

    def shadow_view(self, max_dist):
        """The interval of the visibility query, (0.01, max(0.01, maxDist - 0.02)) with fp32 ends: the upper end is rounded once by the query, which
        the comparison allows for (u |maxDist|)."""
        md = np.broadcast_to(_f64(np.asarray(max_dist, np.float32)), (self.n,))
        hi = np.maximum(SHADOW_BIAS, md - 2.0 * SHADOW_BIAS)
        with np.errstate(invalid="ignore"):
            return self.view(SHADOW_BIAS, hi, np.where(np.isfinite(md), U * np.abs(md), 0.0))

    def judge_shadow(self, visibility, max_dist):
        """Verdict on visibility values over opaque geometry: exactly 0 where some pair is a decided hit in the query's interval
        ("lit_through_decided_hit"), exactly 1 where every pair is a decided miss there ("dark_without_hit"; also for degenerate rays), not judged
        otherwise. .unjudged_share is the share of rays not judged."""
        rep = Report()
        vw = self.shadow_view(max_dist)
        vis = np.asarray(visibility)
        where = lambda i: f"ray {i}"
        must0 = (vw["n_hit"] > 0) & ~self.degenerate
        must1 = ((vw["n_hit"] == 0) & (vw["n_amb"] == 0)) | self.degenerate
        rep.flag("lit_through_decided_hit", must0 & (vis != 0.0), "rays", where)
        rep.flag("dark_without_hit", must1 & (vis != 1.0), "rays", where)
        rep.unjudged_share = float((~must0 & ~must1).mean()) if self.n else 0.0
        rep.stats.update(rays=self.n, shadowed=int(must0.sum()), lit=int(must1.sum()))
        return rep
