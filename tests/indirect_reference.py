"""NumPy restatement of traced indirect lighting (hrpt_indirect_lighting) -- TEST INFRASTRUCTURE.

Shares no code with hobbyrenderer_amd/csrc/pt_indirect.h or pt_lighting.h: written from the definition. The primary rays are
gbuffer_reference.primary_rays; every step after them is binary32 with one rounding per operation in the order the definition fixes (sums and
dot products left to right, normalize = v * (1 / sqrt(dot)), select-form min / max / saturate, no contraction); sin and cos come from the CPU
oracle (or_sin, or_cos), as deferred_reference.py takes its cosine. The traced radiance is an input here (an array, as for
hrpt_indirect_resolve_host).

lobes(..., F=np.float64) is the same formulation in binary64 (np.sin / np.cos) over the same binary32 draws, for the accuracy statement."""
import numpy as np

from hobbyrenderer_amd import structs as S
from gbuffer_reference import primary_rays

f32 = np.float32
u32 = np.uint32
MISS = f32(1e10)
DIFFUSE, SPECULAR = S.INDIRECT_DIFFUSE, S.INDIRECT_SPECULAR
NAN_BITS = 0x7FC00000


def pcg_hash(seed):
    seed = np.asarray(seed, u32)
    with np.errstate(over="ignore"):
        state = seed * u32(747796405) + u32(2891336453)
        word = ((state >> ((state >> u32(28)) + u32(4))) ^ state) * u32(277803737)
        return ((word >> u32(22)) ^ word).astype(u32)


def rng_next(state):
    """(new state, float32 draw = float(state) * 2^-32; may be exactly 1)."""
    state = pcg_hash(state)
    return state, state.astype(f32) * f32(1.0 / 4294967296.0)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _vec(x, y, z):
    return np.stack(np.broadcast_arrays(x, y, z), -1)


def _cross(a, b):
    return _vec(a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0])


def _unit(a, F):
    inv = F(1.0) / np.sqrt(_dot(a, a))
    return a * inv[..., None]


def _saturate(x, F):
    return np.where(x > 0, np.where(x < 1, x, F(1)), F(0)).astype(F)


def _max(a, b, F):           # hrt_max: (a >= b || b != b) ? a : b
    a, b = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F))
    return np.where((a >= b) | (b != b), a, b).astype(F)


def _sincos(x, F):
    if F is np.float64:
        return np.sin(x), np.cos(x)
    from oracle.binding import lib
    L = lib()
    flat = np.asarray(x, f32).ravel()
    s = np.array([L.or_sin(float(v)) for v in flat], f32).reshape(np.shape(x))
    c = np.array([L.or_cos(float(v)) for v in flat], f32).reshape(np.shape(x))
    return s, c


def _pow5(x):
    x2 = x * x
    return (x2 * x2) * x


def _frame(N, F):
    """tangent_frame: up = z unless |N.z| >= 0.999, then x."""
    z = np.abs(N[..., 2]) < F(f32(0.999))
    up = np.where(z[..., None], np.asarray([0, 0, 1], F), np.asarray([1, 0, 0], F))
    T = _unit(_cross(up, N), F)
    return T, _cross(N, T)


def _combine(T, N, B, l):
    return (T * l[..., 0:1] + N * l[..., 1:2]) + B * l[..., 2:3]


def hemisphere_cosine(ux, uy, N, F=f32):
    two_pi = F(f32(2.0) * f32(3.14159265359))
    sp, cp = _sincos(two_pi * ux, F)
    T, B = _frame(N, F)
    cos_t = np.sqrt(uy)
    sin_t = np.sqrt(_max(F(0), F(1) - cos_t * cos_t, F))
    return _combine(T, N, B, _vec(sin_t * cp, cos_t, sin_t * sp))


def ggx_vndf(ux, uy, N, V, rough, F=f32):
    two_pi = F(f32(2.0) * f32(3.14159265359))
    sp, cp = _sincos(two_pi * uy, F)
    T, B = _frame(N, F)
    r = np.sqrt(ux)
    alpha = rough * rough
    Vl = _vec(_dot(V, T), _dot(V, N), _dot(V, B))
    Vh = _unit(_vec(alpha * Vl[..., 0], Vl[..., 1], alpha * Vl[..., 2]), F)
    lensq = Vh[..., 0] * Vh[..., 0] + Vh[..., 2] * Vh[..., 2]
    root = np.sqrt(lensq)
    T1 = np.where((lensq > 0)[..., None], _vec(-Vh[..., 2] / root, F(0) / root, Vh[..., 0] / root), np.asarray([1, 0, 0], F))
    T2 = _cross(Vh, T1)
    t1, t2 = r * cp, r * sp
    s = F(0.5) * (F(1) + Vh[..., 1])
    a = np.sqrt(_max(F(0), F(1) - t1 * t1, F))
    t2 = a + s * (t2 - a)
    nz = np.sqrt(_max(F(0), (F(1) - t1 * t1) - t2 * t2, F))
    Nh = (T1 * t1[..., None] + T2 * t2[..., None]) + Vh * nz[..., None]
    Ne = _unit(_vec(alpha * Nh[..., 0], _max(F(0), Nh[..., 1], F), alpha * Nh[..., 2]), F)
    return _combine(T, N, B, Ne)


def vndf_weight(F0, N, V, L, Hv, rough, F=f32):
    alpha = rough * rough
    alpha2 = alpha * alpha
    n_v, n_l, v_h = _saturate(_dot(N, V), F), _saturate(_dot(N, L), F), _saturate(_dot(V, Hv), F)
    fc = _pow5(F(1) - v_h)
    fs = _saturate(F(50) * F0[..., 1], F) * fc
    fk = F(1) - fc
    Fr = fs[..., None] + fk[..., None] * F0
    g1 = F(2) * n_l / (n_l + np.sqrt(alpha2 + (F(1) - alpha2) * n_l * n_l))
    return np.where(((n_v <= 0) | (n_l <= 0))[..., None], F(0), Fr * g1[..., None]).astype(F)


def lobes(albedo, normal, geo_normal, depth, cb, frame_seed, F=f32):
    """Steps 1-5 at every pixel: dict of hit [H, W], X, s (the state behind the four draws), u [4, H, W] float32, traced_d, dir_d, traced_s,
    dir_s, w_s, and the culling quantities ndd = dot(N, dirD), nds = dot(N, dirS), wmax = maxcomp(wS)."""
    A, N4, G, Dp = (np.asarray(a, f32) for a in (albedo, normal, geo_normal, depth))
    H, W = Dp.shape[:2]
    o, d, _ = primary_rays(cb, W, H)
    t = Dp[..., 0]
    hit = ~(t == MISS)
    oF, dF = o.astype(F), d.astype(F)
    with np.errstate(all="ignore"):
        X = np.stack([oF[k] + dF[..., k] * t.astype(F) for k in range(3)], -1)
        V = -dF
        g = (np.arange(H, dtype=u32)[:, None] * u32(W) + np.arange(W, dtype=u32)[None, :]).astype(u32)
        s = pcg_hash(g + pcg_hash(u32(frame_seed)))
        u = []
        for _ in range(4):
            s, draw = rng_next(s)
            u.append(draw)
        N, base, rough, metal = N4[..., :3].astype(F), A[..., :3].astype(F), N4[..., 3].astype(F), G[..., 3].astype(F)
        dir_d = hemisphere_cosine(u[0].astype(F), u[1].astype(F), N, F)
        ndd = _dot(N, dir_d)
        traced_d = hit & (F(1) - metal > 0) & (ndd > 0)
        Hv = ggx_vndf(u[2].astype(F), u[3].astype(F), N, V, rough, F)
        i = -V
        k2 = F(2) * _dot(i, Hv)
        dir_s = i - Hv * k2[..., None]
        nds = _dot(N, dir_s)
        q = (F(f32(1.5)) - F(1)) / (F(f32(1.5)) + F(1))
        d0 = q * q
        F0 = d0 + metal[..., None] * (base - d0)
        w_s = vndf_weight(F0, N, V, dir_s, Hv, rough, F)
        w_s = np.where((nds > 0)[..., None], w_s, F(0))
        wmax = _max(w_s[..., 0], _max(w_s[..., 1], w_s[..., 2], F), F)
        traced_s = hit & (nds > 0) & (wmax > 0)
    return dict(hit=hit, X=X, s=s, u=np.array(u), traced_d=traced_d, dir_d=dir_d, traced_s=traced_s, dir_s=dir_s, w_s=w_s, ndd=ndd, nds=nds, wmax=wmax,
                metal=metal)


def _records(traced, X, direction, rng):
    out = np.zeros(traced.shape, S.Ray)
    nan = np.array(NAN_BITS, u32).view(f32)
    out["origin"] = np.where(traced[..., None], X, nan)
    out["tmin"] = np.where(traced, f32(1e-4), f32(0))
    out["direction"] = np.where(traced[..., None], direction, f32(0))
    out["tmax"] = np.where(traced, f32(1e10), f32(0))
    out["rng"] = np.where(traced, rng, u32(0))
    return out


def rays(albedo, normal, geo_normal, depth, cb, flags=DIFFUSE | SPECULAR, frame_seed=0):
    """The ray records of the flagged lobes: S.Ray [lobes, H, W], diffuse first."""
    L = lobes(albedo, normal, geo_normal, depth, cb, frame_seed)
    out = []
    if flags & DIFFUSE:
        out.append(_records(L["traced_d"], L["X"], L["dir_d"], L["s"]))
    if flags & SPECULAR:
        out.append(_records(L["traced_s"], L["X"], L["dir_s"], pcg_hash(L["s"])))
    return np.array(out)


def resolve(albedo, normal, geo_normal, depth, cb, radiance, flags=DIFFUSE | SPECULAR, frame_seed=0):
    """(diffuse, specular) [H, W, 4] float32 from radiance [lobes, H, W, 4]; zeros for a lobe that is not flagged and at misses."""
    L = lobes(albedo, normal, geo_normal, depth, cb, frame_seed)
    rad = np.asarray(radiance, f32)
    shape = L["hit"].shape + (4,)
    dif, spec = np.zeros(shape, f32), np.zeros(shape, f32)
    k = 0
    if flags & DIFFUSE:
        on = (rad[k, ..., 3] == 1) & L["hit"]
        dif[..., :3] = np.where(on[..., None], rad[k, ..., :3], f32(0))
        dif[..., 3] = np.where(on, f32(1), f32(0))
        k += 1
    if flags & SPECULAR:
        on = (rad[k, ..., 3] == 1) & L["hit"]
        with np.errstate(all="ignore"):
            spec[..., :3] = np.where(on[..., None], rad[k, ..., :3] * L["w_s"], f32(0))
        spec[..., 3] = np.where(on, f32(1), f32(0))
    return dif, spec


def compose(color, albedo, geo_normal, depth, diffuse, specular, intensity):
    C, A, G, Dp, Df, Sp = (np.asarray(a, f32) for a in (color, albedo, geo_normal, depth, diffuse, specular))
    hit = ~(Dp[..., 0] == MISS)
    with np.errstate(all="ignore"):
        rgb = C[..., :3] + ((((Df[..., :3] * A[..., :3]) * (f32(1) - G[..., 3])[..., None]) + Sp[..., :3]) * f32(intensity))
    out = C.copy()
    out[..., :3] = np.where(hit[..., None], rgb, C[..., :3])
    return out
