"""NumPy restatement of deferred lighting (hrpt_deferred_lighting) -- TEST INFRASTRUCTURE.

Shares no code with hobbyrenderer_amd/csrc/pt_deferred.h: written from the definition. The primary rays are gbuffer_reference.primary_rays;
every step after them is binary32 with one rounding per operation in the order the definition fixes (sums and dot products left to right,
normalize = v * (1 / sqrt(dot)), select-form min / max / saturate, no contraction); cos comes from the CPU oracle (or_cos). The atmosphere
terms and the visibilities are inputs here (images, as for hrpt_deferred_shade_host); `atmosphere` and `visibilities` below get them from
the oracle binding (sun_radiance, sky_radiance, shadow_query) for tests that own a scene.

shade(..., F=np.float64) is the same formulation in binary64 (math.cos), for the accuracy statement: steps 3-5 with the visibilities given."""
import math

import numpy as np

from hobbyrenderer_amd import structs as S
from gbuffer_reference import primary_rays

f32 = np.float32
MISS = f32(1e10)
SHADOWS, SKY, INDIRECT = S.DEFERRED_SHADOWS, S.DEFERRED_SKY, S.DEFERRED_INDIRECT


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _unit(a, F):
    inv = F(1.0) / np.sqrt(_dot(a, a))
    return a * inv[..., None] if np.ndim(inv) else a * inv


def _saturate(x, F):
    return np.where(x > 0, np.where(x < 1, x, F(1)), F(0)).astype(F)


def _max(a, b, F):           # hrt_max: (a >= b || b != b) ? a : b
    a, b = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F))
    return np.where((a >= b) | (b != b), a, b).astype(F)


def _cos(x, F):
    if F is np.float64:
        return F(math.cos(float(x)))
    from oracle.binding import lib
    return f32(lib().or_cos(float(f32(x))))


def _pow5(x):
    x2 = x * x
    return (x2 * x2) * x


def _mix(a, b, t):
    return a + t * (b - a)


def hit_positions(cb, depth):
    """(o [3], d [H, W, 3], X [H, W, 3]) float32: X = o + d * t per component; at a miss X is whatever 1e10 gives."""
    H, W = depth.shape[:2]
    o, d, _ = primary_rays(cb, W, H)
    t = np.asarray(depth, f32)[..., 0]
    X = np.stack([o[k] + d[..., k] * t for k in range(3)], -1).astype(f32)
    return o, d, X


def light_direction(l, N, X, sun, F=f32):
    """The cull and direction of one light at every pixel: (lit bool [H, W], L [H, W, 3], maxDist [H, W]). A comparison with a NaN is
    false, so `not (x <= 0)` is what the definition's 'skip if x <= 0' leaves lit."""
    shape = N.shape[:-1]
    t = int(l["m_Type"])
    with np.errstate(all="ignore"):
        if t == S.LIGHT_DIRECTIONAL:
            lit = ~(_dot(N, sun) <= 0)
            return lit, np.broadcast_to(sun, shape + (3,)).astype(F), np.full(shape, F(1e10), F)
        if t not in (S.LIGHT_POINT, S.LIGHT_SPOT):
            return np.zeros(shape, bool), np.zeros(shape + (3,), F), np.zeros(shape, F)
        lit = np.full(shape, not (F(l["m_Intensity"]) <= 0))
        to_light = np.asarray(l["m_Position"], F) - X
        dist_sq = _dot(to_light, to_light)
        rng = F(l["m_Range"])
        if rng > 0:
            lit &= ~(dist_sq > rng * rng)
        dist = np.sqrt(dist_sq)
        Lc = to_light / dist[..., None]
        ndl = _dot(N, Lc)
        if t == S.LIGHT_SPOT:
            lit &= ~(ndl <= 0)
            light_dir = _unit(np.asarray(l["m_Direction"], F), F)
            cos_theta = _dot(-Lc, light_dir)
            lit &= ~(cos_theta < _cos(l["m_SpotOuterConeAngle"], F))
        lit &= ~(ndl <= 0)
        return lit, Lc.astype(F), dist.astype(F)


def light_radiance(l, X, F=f32):
    """Radiance of a point or spot light at every X, [H, W, 3]."""
    with np.errstate(all="ignore"):
        to_light = np.asarray(l["m_Position"], F) - X
        dist_sq = _dot(to_light, to_light)
        dist = np.sqrt(dist_sq)
        att = F(1) / (dist_sq + F(1))
        rng = F(l["m_Range"])
        if rng > 0:
            q = dist / rng
            q2 = q * q
            q4 = q2 * q2
            sa = _saturate(F(1) - q4, F)
            att = att * (sa * sa)
        base = np.asarray(l["m_Color"], F) * F(l["m_Intensity"])
        if int(l["m_Type"]) == S.LIGHT_SPOT:
            Lc = to_light / dist[..., None]
            light_dir = _unit(np.asarray(l["m_Direction"], F), F)
            cos_theta = _dot(-Lc, light_dir)
            cos_outer, cos_inner = _cos(l["m_SpotOuterConeAngle"], F), _cos(l["m_SpotInnerConeAngle"], F)
            spot = _saturate((cos_theta - cos_outer) / (cos_inner - cos_outer), F)
            return ((base * spot[..., None]) * att[..., None]).astype(F)
        return (base * att[..., None]).astype(F)


def direct_light(N, V, base_color, rough, metal, L, radiance, F=f32):
    """prepare_byproducts + EvaluateDirectLight before the shadow factor, ior 1.5: (diffuse, specular), [H, W, 3] each."""
    PI = F(f32(3.14159265359))
    with np.errstate(all="ignore"):
        n_v = _saturate(_dot(N, V), F)
        n_l = _saturate(_dot(N, L), F)
        vpl = V + L
        ln = _dot(vpl, vpl)
        Hv = np.where((ln > F(f32(1e-8)))[..., None], vpl * (F(1) / np.sqrt(ln))[..., None], N)
        n_h = _saturate(_dot(N, Hv), F)
        v_h = _saturate(_dot(V, Hv), F)
        l_h = _saturate(_dot(L, Hv), F)
        q = (F(f32(1.5)) - F(1)) / (F(f32(1.5)) + F(1))
        d0 = q * q
        F0 = _mix(d0, base_color, metal[..., None])
        k_d = F(1) - metal
        fc = _pow5(F(1) - v_h)
        fs = _saturate(F(50) * F0[..., 1], F) * fc
        fk = F(1) - fc
        Fr = fs[..., None] + fk[..., None] * F0
        rough2 = rough * rough
        fl, fv = _pow5(F(1) - n_l), _pow5(F(1) - n_v)
        fd90 = F(0.5) + F(2) * rough2 * l_h * l_h
        fd = _mix(F(1), fd90, fl) * _mix(F(1), fd90, fv)
        dt = np.where((n_l <= 0) | (n_v <= 0), F(0), fd * n_l / PI)
        dif = (k_d * dt)[..., None] * base_color
        alpha = rough * rough
        alpha2 = alpha * alpha
        denom = n_h * n_h * (alpha2 - F(1)) + F(1)
        D = alpha2 / (PI * denom * denom)
        g1 = n_v * np.sqrt(alpha2 + (F(1) - alpha2) * n_l * n_l)
        g2 = n_l * np.sqrt(alpha2 + (F(1) - alpha2) * n_v * n_v)
        G2 = F(0.5) / _max(g1 + g2, F(f32(1e-6)), F)
        k = D * G2
        spec = Fr * k[..., None]
        return (dif * radiance).astype(F), ((spec * n_l[..., None]) * radiance).astype(F)


def rays(depth, normal, cb, lights, first=0, count=None):
    """The shadow-ray records of lights[first : first + count]: S.Ray [count, H, W]."""
    depth, normal = np.asarray(depth, f32), np.asarray(normal, f32)
    count = len(lights) - first if count is None else count
    H, W = depth.shape[:2]
    out = np.zeros((count, H, W), S.Ray)
    _, _, X = hit_positions(cb, depth)
    sun = np.asarray(cb["m_SunDirection"], f32)
    hit = ~(depth[..., 0] == MISS)
    nan = np.array(0x7FC00000, np.uint32).view(f32)
    for j in range(count):
        lit, L, max_dist = light_direction(lights[first + j], normal[..., :3], X, sun)
        lit &= hit
        out[j]["origin"] = np.where(lit[..., None], X, nan)
        out[j]["direction"] = np.where(lit[..., None], L, f32(0))
        out[j]["tmax"] = np.where(lit, max_dist, f32(0))
    return out


def shade(albedo, normal, geo_normal, emissive, depth, cb, lights, flags=0, visibility=None, sun_radiance=None, sky=None, indirect=None,
          indirect_intensity=1.0, F=f32, return_lit=False):
    """The lit image [H, W, 4] of the definition. visibility [len(lights), H, W] (None = 1), sun_radiance [H, W, 4] (None = colour x intensity),
    sky [H, W, 4] stored at misses (None = zeros), indirect [H, W, 4] read with INDIRECT in flags."""
    A, N4, G, E, Dp = (np.asarray(a, f32) for a in (albedo, normal, geo_normal, emissive, depth))
    H, W = Dp.shape[:2]
    o, d, X = hit_positions(cb, Dp)
    if F is np.float64:
        o64, d64 = o.astype(F), d.astype(F)
        X = np.stack([o64[k] + d64[..., k] * Dp[..., 0].astype(F) for k in range(3)], -1)
    hit = ~(Dp[..., 0] == MISS)
    N, V = N4[..., :3].astype(F), (-d).astype(F)
    base, rough, metal = A[..., :3].astype(F), N4[..., 3].astype(F), G[..., 3].astype(F)
    sun = np.asarray(cb["m_SunDirection"], f32).astype(F)
    total_d, total_s = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F)
    lits = []
    with np.errstate(all="ignore"):
        for i, l in enumerate(lights):
            lit, L, _ = light_direction(l, N, X, sun, F)
            lits.append(lit & hit)
            if int(l["m_Type"]) == S.LIGHT_DIRECTIONAL:
                radiance = np.asarray(sun_radiance, f32)[..., :3].astype(F) if sun_radiance is not None else np.broadcast_to(np.asarray(l["m_Color"], F) * F(l["m_Intensity"]), (H, W, 3))
            else:
                radiance = light_radiance(l, X, F)
            dif, spec = direct_light(N, V, base, rough, metal, L, radiance, F)
            vis = np.ones((H, W), F) if visibility is None else np.asarray(visibility, f32)[i].astype(F)
            total_d = np.where(lit[..., None], total_d + dif * vis[..., None], total_d)
            total_s = np.where(lit[..., None], total_s + spec * vis[..., None], total_s)
        rgb = (total_d + total_s) + E[..., :3].astype(F)
        if flags & INDIRECT:
            irr = np.asarray(indirect, f32)
            ind = (((irr[..., :3].astype(F) * base) * (F(1) - metal)[..., None]) * F(f32(0.31830988618))) * F(f32(indirect_intensity))
            rgb = np.where((irr[..., 3] == 1)[..., None], rgb + ind, rgb)
    out = np.zeros((H, W, 4), F)
    out[..., :3], out[..., 3] = rgb, A[..., 3]
    miss = np.zeros((H, W, 4), F) if sky is None else np.asarray(sky, f32).astype(F)
    out = np.where(hit[..., None], out, miss).astype(F)
    return (out, np.array(lits).reshape(len(lights), H, W)) if return_lit else out


def atmosphere(oracle, cb, depth, sun_intensity):
    """(sun_radiance, sky) images [H, W, 4] float32 from the oracle: sun_radiance(X) at hits, (sky_radiance(o, d, sun disk), 1) at misses."""
    depth = np.asarray(depth, f32)
    H, W = depth.shape[:2]
    o, d, X = hit_positions(cb, depth)
    sun = np.asarray(cb["m_SunDirection"], f32)
    sr, sky = np.zeros((H, W, 4), f32), np.zeros((H, W, 4), f32)
    for y in range(H):
        for x in range(W):
            if depth[y, x, 0] == MISS:
                sky[y, x, :3] = oracle.sky_radiance(o, d[y, x], sun, float(sun_intensity), True); sky[y, x, 3] = 1.0
            else:
                sr[y, x, :3] = oracle.sun_radiance(X[y, x], sun, float(sun_intensity))
    return sr, sky


def visibilities(oracle, ray_records):
    """float32 [n, H, W]: the oracle's CalculateRTShadow<true> for every lit record of `ray_records` (rays(...)), 1 elsewhere."""
    vis = np.ones(ray_records.shape, f32)
    for idx in np.ndindex(ray_records.shape):
        r = ray_records[idx]
        if np.isfinite(r["origin"]).all() and np.isfinite(r["direction"]).all():
            vis[idx] = oracle.shadow_query(r["origin"], r["direction"], float(r["tmax"]))
    return vis
