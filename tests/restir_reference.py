"""NumPy restatement of resampled direct lighting (hrpt_restir_lighting) -- TEST INFRASTRUCTURE.

Shares no code with hobbyrenderer_amd/csrc/pt_restir.h: written from the definition, on deferred_reference's light_direction / light_radiance
/ direct_light and gbuffer_reference.primary_rays. Every step is binary32 with one rounding per operation in the order the definition fixes;
sin and cos come from the CPU oracle (or_sin, or_cos); the PCG hash is integer arithmetic.

The passes gather the target from a table: targets(...) evaluates pHat(S, i) -- with the diffuse and specular terms, the direction and the
distance that go with it -- for every light i at every pixel once, so pHat(S, light) and pHat(S_q, light) are both reads of it. With
F=np.float64 the same table is the float64 formulation of the target (for the accuracy statement of the one-light case)."""
import numpy as np

from hobbyrenderer_amd import structs as S
import deferred_reference as R
from probes_reference import pcg, _rng_next
from temporal_reference import _fmap, _min

f32 = np.float32
u32 = np.uint32
EMPTY = u32(S.RESTIR_EMPTY)
TWO_PI = f32(6.2831853)
SHADOWS, SKY, TEMPORAL, SPATIAL, INITIAL_VISIBILITY, RESET = (S.RESTIR_SHADOWS, S.RESTIR_SKY, S.RESTIR_TEMPORAL, S.RESTIR_SPATIAL, S.RESTIR_INITIAL_VISIBILITY,
                                                             S.RESTIR_RESET)


def luminance(c, F=f32):
    return (c[..., 0] * F(f32(0.2126)) + c[..., 1] * F(f32(0.7152))) + c[..., 2] * F(f32(0.0722))


class Targets:
    """p [n, H, W], dif / spec / L [n, H, W, 3], max_dist [n, H, W], lit [n, H, W] of lights[:n] at every pixel; hit [H, W]; X [H, W, 3]."""


def targets(planes, cb, lights, sun_radiance=None, F=f32):
    A, N4, G, _, Dp = (np.asarray(a, f32) for a in planes)
    n = int(cb["m_LightCount"])
    H, W = Dp.shape[:2]
    o, d, X = R.hit_positions(cb, Dp)
    if F is np.float64:
        X = np.stack([o.astype(F)[k] + d.astype(F)[..., k] * Dp[..., 0].astype(F) for k in range(3)], -1)
    T = Targets()
    T.n, T.hit, T.X = n, ~(Dp[..., 0] == R.MISS), X
    N, V = N4[..., :3].astype(F), (-d).astype(F)
    base, rough, metal = A[..., :3].astype(F), N4[..., 3].astype(F), G[..., 3].astype(F)
    sun = np.asarray(cb["m_SunDirection"], f32).astype(F)
    T.p, T.max_dist, T.lit = np.zeros((n, H, W), F), np.zeros((n, H, W), F), np.zeros((n, H, W), bool)
    T.dif, T.spec, T.L = np.zeros((n, H, W, 3), F), np.zeros((n, H, W, 3), F), np.zeros((n, H, W, 3), F)
    with np.errstate(all="ignore"):
        for i in range(n):
            l = lights[i]
            lit, L, max_dist = R.light_direction(l, N, X, sun, F)
            if int(l["m_Type"]) == S.LIGHT_DIRECTIONAL:
                radiance = (np.asarray(sun_radiance, f32)[..., :3].astype(F) if sun_radiance is not None
                            else np.broadcast_to(np.asarray(l["m_Color"], F) * F(l["m_Intensity"]), (H, W, 3)))
            else:
                radiance = R.light_radiance(l, X, F)
            dif, spec = R.direct_light(N, V, base, rough, metal, L, radiance, F)
            p = luminance(dif + spec, F)
            T.p[i] = np.where(lit & (p > 0), p, F(0))
            T.dif[i], T.spec[i] = np.where(lit[..., None], dif, F(0)), np.where(lit[..., None], spec, F(0))
            T.L[i], T.max_dist[i], T.lit[i] = L, max_dist, lit
    return T


def _grid(H, W):
    return np.mgrid[0:H, 0:W]


def states(frame_seed, H, W):
    """(sA, sB, sC) uint32 [H, W]: each derived from the initial value."""
    g = np.arange(H * W, dtype=u32).reshape(H, W)
    with np.errstate(over="ignore"):
        sA = pcg((g + pcg(u32(frame_seed))).astype(u32))
    sB = pcg(sA)
    return sA, sB, pcg(sB)


def _empty(H, W):
    r = np.zeros((H, W), S.RestirReservoir)
    r["light"] = EMPTY
    return r


class _Running:
    """The reservoir being built at every pixel: add() under a mask of the pixels that take part."""

    def __init__(self, H, W):
        self.light, self.w_sum, self.M, self.p_hat = np.full((H, W), EMPTY, u32), np.zeros((H, W), f32), np.zeros((H, W), f32), np.zeros((H, W), f32)

    def add(self, mask, light, w, m, p_hat, u):
        with np.errstate(all="ignore"):
            w, m = np.broadcast_to(np.asarray(w, f32), mask.shape), np.broadcast_to(np.asarray(m, f32), mask.shape)
            self.w_sum = np.where(mask, self.w_sum + w, self.w_sum).astype(f32)
            self.M = np.where(mask, self.M + m, self.M).astype(f32)
            take = mask & (w > 0) & ((u * self.w_sum).astype(f32) <= w)
            self.light = np.where(take, light, self.light).astype(u32)
            self.p_hat = np.where(take, p_hat, self.p_hat).astype(f32)

    def finish(self, norm, valid):
        out = _empty(*valid.shape)
        with np.errstate(all="ignore"):
            Wt = np.where(self.p_hat > 0, ((self.w_sum / norm).astype(f32) / self.p_hat).astype(f32), f32(0))
        out["light"], out["W"], out["M"], out["pHat"] = self.light, Wt, self.M, self.p_hat
        out[~valid] = _empty(1, 1)[0, 0]
        return out


def _gather(table, light, n, yy, xx):
    """table[light, yy, xx] where light < n, else 0."""
    ok = light < n
    li = np.where(ok, light, 0).astype(np.int64)
    v = table[li, yy, xx] if n else np.zeros(light.shape + table.shape[3:], table.dtype)
    return np.where(ok.reshape(ok.shape + (1,) * (v.ndim - ok.ndim)), v, table.dtype.type(0))


def ray_records(T, res):
    """The shadow-ray record of each reservoir's light: S.Ray [H, W]; an empty reservoir or a miss gives the NaN-origin record."""
    H, W = T.hit.shape
    yy, xx = _grid(H, W)
    light = res["light"]
    lit = T.hit & (light < T.n) & (_gather(T.lit, light, T.n, yy, xx) if T.n else False)
    out = np.zeros((H, W), S.Ray)
    nan = np.array(0x7FC00000, u32).view(f32)
    out["origin"] = np.where(lit[..., None], T.X, nan)
    out["direction"] = np.where(lit[..., None], _gather(T.L, light, T.n, yy, xx), f32(0))
    out["tmax"] = np.where(lit, _gather(T.max_dist, light, T.n, yy, xx), f32(0))
    return out


def initial(T, params):
    """Pass A: reservoirs S.RestirReservoir [H, W]."""
    H, W = T.hit.shape
    n = T.n
    yy, xx = _grid(H, W)
    r = _Running(H, W)
    valid = T.hit & (n > 0)
    s = states(params.frameSeed, H, W)[0]
    for _ in range(params.candidates if n else 0):
        s, u0 = _rng_next(s)
        s, u1 = _rng_next(s)
        i = np.minimum((u0 * f32(n)).astype(f32).astype(u32), u32(n - 1))
        p = T.p[i.astype(np.int64), yy, xx]
        r.add(valid, i, (p * f32(n)).astype(f32), f32(1), p, u1)
    return r.finish(r.M, valid)


def temporal(T, planes, params, cur, motion=None, history=None, initial_visibility=None):
    """Pass B. history: (reservoirs, keys) or None; taken only with TEMPORAL and without RESET."""
    H, W = T.hit.shape
    n = T.n
    yy, xx = _grid(H, W)
    N, depth = np.asarray(planes[1], f32)[..., :3], np.asarray(planes[4], f32)
    cur = cur.copy()
    if initial_visibility is not None:
        cur["W"] = np.where(np.asarray(initial_visibility, f32) == 0, f32(0), cur["W"])
    s = states(params.frameSeed, H, W)[1]
    s, u0 = _rng_next(s)
    s, u1 = _rng_next(s)
    t = _Running(H, W)
    with np.errstate(all="ignore"):
        t.add(T.hit, cur["light"], ((cur["pHat"] * cur["W"]).astype(f32) * cur["M"]).astype(f32), cur["M"], cur["pHat"], u0)
        if history is not None and (params.flags & TEMPORAL) and not (params.flags & RESET):
            hres, hkey = history
            m = np.asarray(motion, f32)
            qx = np.floor(((xx.astype(f32) + f32(0.5)).astype(f32) + m[..., 0]).astype(f32))
            qy = np.floor(((yy.astype(f32) + f32(0.5)).astype(f32) + m[..., 1]).astype(f32))
            inside = (m[..., 3] == 1) & (qx >= 0) & (qy >= 0) & (qx < f32(W)) & (qy < f32(H))
            qxi, qyi = np.where(inside, qx, 0).astype(np.int64), np.where(inside, qy, 0).astype(np.int64)
            prev, key = hres[qyi, qxi], np.asarray(hkey, f32)[qyi, qxi]
            e = (depth[..., 1] + m[..., 2]).astype(f32)
            acc = (T.hit & inside & (prev["light"] < n) & (R._dot(N, key[..., :3]) >= f32(params.normalThreshold))
                   & (np.abs(key[..., 3] - e) <= (f32(params.depthThreshold) * e).astype(f32)))
            Mp = _min(prev["M"], (f32(params.maxHistory) * cur["M"]).astype(f32))
            pp = _gather(T.p, prev["light"], n, yy, xx)
            t.add(acc, prev["light"], ((pp * prev["W"]).astype(f32) * Mp).astype(f32), Mp, pp, u1)
    return t.finish(t.M, T.hit)


def spatial(T, planes, params, tres):
    """Pass C: (final reservoirs [H, W], keys [H, W, 4])."""
    H, W = T.hit.shape
    n = T.n
    yy, xx = _grid(H, W)
    N4, depth = np.asarray(planes[1], f32), np.asarray(planes[4], f32)
    N, vd = N4[..., :3], depth[..., 1]
    c = tres
    s = _Running(H, W)
    Sc, accepted = np.zeros((H, W), f32), np.zeros((H, W), np.int64)
    rng = states(params.frameSeed, H, W)[2]
    cos, sin = _fmap("or_cos"), _fmap("or_sin")
    with np.errstate(all="ignore"):
        for _ in range(params.spatialSamples if params.flags & SPATIAL else 0):
            rng, ua = _rng_next(rng)
            rng, ub = _rng_next(rng)
            rng, us = _rng_next(rng)
            r = (f32(params.spatialRadius) * np.sqrt(ua)).astype(f32)
            th = (TWO_PI * ub).astype(f32)
            qx = xx + np.floor(((r * cos(th)).astype(f32) + f32(0.5)).astype(f32)).astype(np.int64)
            qy = yy + np.floor(((r * sin(th)).astype(f32) + f32(0.5)).astype(f32)).astype(np.int64)
            ok = T.hit & (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H) & ~((qx == xx) & (qy == yy))
            qx, qy = np.where(ok, qx, 0), np.where(ok, qy, 0)
            ok &= T.hit[qy, qx]
            ok &= ~(R._dot(N, N[qy, qx]) < f32(params.normalThreshold))
            ok &= ~(np.abs(vd[qy, qx] - vd) > (f32(params.depthThreshold) * vd).astype(f32))
            nb = c[qy, qx]
            ta = _gather(T.p, nb["light"], n, yy, xx)
            tb = _gather(T.p, c["light"], n, qy, qx)
            ni, nc = (nb["M"] * nb["pHat"]).astype(f32), (c["M"] * c["pHat"]).astype(f32)
            mi = np.where(ni == 0, f32(0), ni / (ni + (c["M"] * ta).astype(f32)).astype(f32)).astype(f32)
            mc = np.where(nc == 0, f32(0), nc / (nc + (nb["M"] * tb).astype(f32)).astype(f32)).astype(f32)
            s.add(ok, nb["light"], ((ta * nb["W"]).astype(f32) * mi).astype(f32), nb["M"], ta, us)
            Sc = np.where(ok, Sc + mc, Sc).astype(f32)
            accepted = accepted + ok
        rng, uo = _rng_next(rng)
        Sc = np.where(accepted == 0, f32(1), Sc)
        accepted = np.maximum(accepted, 1)
        s.add(T.hit, c["light"], ((c["pHat"] * c["W"]).astype(f32) * Sc).astype(f32), c["M"], c["pHat"], uo)
    keys = np.concatenate([N, vd[..., None]], -1).astype(f32)
    return s.finish(accepted.astype(f32), T.hit), keys


def shade(T, planes, final, visibility=None, sky=None, F=f32):
    """Pass D: the lit image [H, W, 4]."""
    A, _, _, E, _ = (np.asarray(a, f32) for a in planes)
    H, W = T.hit.shape
    yy, xx = _grid(H, W)
    light = final["light"]
    with np.errstate(all="ignore"):
        k = final["W"].astype(F) * (F(1) if visibility is None else np.asarray(visibility, f32).astype(F))
        total_d = _gather(T.dif, light, T.n, yy, xx) * k[..., None]
        total_s = _gather(T.spec, light, T.n, yy, xx) * k[..., None]
        rgb = (total_d + total_s) + E[..., :3].astype(F)
    out = np.zeros((H, W, 4), F)
    out[..., :3], out[..., 3] = rgb, A[..., 3]
    miss = np.zeros((H, W, 4), F) if sky is None else np.asarray(sky, f32).astype(F)
    return np.where(T.hit[..., None], out, miss).astype(F)


def frame(T, planes, params, motion=None, history=None, visibility_of=None, sky=None):
    """One call of the stage: (image, final reservoirs, keys). visibility_of(ray records [H, W]) -> float32 [H, W], or None for 1."""
    cur = initial(T, params)
    iv = visibility_of(ray_records(T, cur)) if (params.flags & INITIAL_VISIBILITY) and visibility_of else None
    tres = temporal(T, planes, params, cur, motion, history, iv)
    fin, keys = spatial(T, planes, params, tres)
    vis = visibility_of(ray_records(T, fin)) if (params.flags & SHADOWS) and visibility_of else None
    return shade(T, planes, fin, vis, sky), fin, keys
