"""NumPy float32 statement of the irradiance probe volume (hrpt_probes_*): ray generation, blend, border rule and
query, written from the prose of section 26, independent of hobbyrenderer_amd/csrc/pt_probes.h. It is the yardstick of
tests/test_probes_cpu.py and tests/test_probes_gpu.py: the library must produce the same BITS.

Every operation is an IEEE binary32 + - * / sqrt floor or a comparison in the order section 26 writes it (sums and dot products left to
right), which NumPy rounds exactly like the C++ / HIP build (no FMA contraction there). min / max / clamp / saturate are the select forms of
hobbyrt/detmath.h; pow, sin and cos come from the CPU oracle (oracle.binding: or_pow, or_sin, or_cos); the PCG hash is integer arithmetic.

blend64 / query64 are float64 formulations of the same two stages (sums as matrix products, libm pow) that take the float32 directions and
atlases as exact inputs: the yardstick of the statement's own rounding.
"""
import numpy as np

from temporal_reference import F, _clamp, _fmap, _max, _min, _saturate

PI = F(3.14159265359)
TWO_PI = F(F(2) * PI)
GOLDEN = F(0.61803398875)
U32 = np.uint32
IRR_I, IRR_T, DIST_I, DIST_T = 6, 8, 14, 16
RAY_TMAX = F(1e10)
FLT_MAX = F(3.402823466e38)


# ---- integer RNG (hobbyrt/detmath.h hrt_pcg_hash, hrt_rng_next) ------------------------------------------------------------------------
def pcg(x):
    with np.errstate(over="ignore"):
        x = np.asarray(x, U32)
        state = (x * U32(747796405) + U32(2891336453)).astype(U32)
        word = (((state >> ((state >> U32(28)) + U32(4))) ^ state) * U32(277803737)).astype(U32)
        return ((word >> U32(22)) ^ word).astype(U32)


def _rng_next(state):
    state = pcg(state)
    return state, (state.astype(np.float32) * F(1.0 / 4294967296.0)).astype(np.float32)


# ---- the volume --------------------------------------------------------------------------------------------------------------------------
def probe_count(vol):
    return int(np.prod(np.asarray(vol["counts"], np.uint64)))


def probe_positions(vol):
    """[P, 3]: probe p = x + cx * (y + cy * z) at origin + (x, y, z) * spacing."""
    cx, cy, cz = [int(c) for c in vol["counts"]]
    p = np.arange(cx * cy * cz)
    xyz = [p % cx, (p // cx) % cy, p // (cx * cy)]
    o, s = np.asarray(vol["origin"], np.float32), np.asarray(vol["spacing"], np.float32)
    return np.stack([(o[k] + xyz[k].astype(np.float32) * s[k]).astype(np.float32) for k in range(3)], -1)


# ---- rays ----------------------------------------------------------------------------------------------------------------------------------
def rotation(frame_seed):
    """The rotation matrix of an update, float32 [3, 3]."""
    s = pcg(U32(frame_seed) ^ U32(0x9E3779B9))
    s, u1 = _rng_next(s)
    s, u2 = _rng_next(s)
    s, u3 = _rng_next(s)
    a, b = np.sqrt(F(1) - u1).astype(np.float32), np.sqrt(u1).astype(np.float32)
    sin, cos = _fmap("or_sin"), _fmap("or_cos")
    p2, p3 = TWO_PI * u2, TWO_PI * u3
    x, y, z, w = a * sin(p2), a * cos(p2), b * sin(p3), b * cos(p3)
    two, one = F(2), F(1)
    R = [[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
         [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
         [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]]
    return np.array(R, np.float32).reshape(3, 3)


def directions(frame_seed, n):
    """The n shared unit directions of an update, float32 [n, 3]."""
    R = rotation(frame_seed)
    k = np.arange(n, dtype=np.uint32)
    z = (F(1) - (U32(2) * k + U32(1)).astype(np.float32) / F(n)).astype(np.float32)
    r = np.sqrt(_max(F(0), F(1) - z * z)).astype(np.float32)
    t = (k.astype(np.float32) * GOLDEN).astype(np.float32)
    phi = (TWO_PI * (t - np.floor(t))).astype(np.float32)
    f = [r * _fmap("or_cos")(phi), r * _fmap("or_sin")(phi), z]
    v = [((R[i, 0] * f[0] + R[i, 1] * f[1]) + R[i, 2] * f[2]).astype(np.float32) for i in range(3)]
    length = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]).astype(np.float32)
    return np.stack([(c / length).astype(np.float32) for c in v], -1)


def rays(vol, frame_seed, ray_dtype):
    """(records [P * N] of `ray_dtype` (hobbyrenderer_amd.structs.Ray), directions4 [N, 4])."""
    n, P = int(vol["raysPerProbe"]), probe_count(vol)
    d = directions(frame_seed, n)
    out = np.zeros(P * n, ray_dtype)
    out["origin"] = np.repeat(probe_positions(vol), n, axis=0)
    out["direction"] = np.tile(d, (P, 1))
    out["tmax"] = RAY_TMAX
    out["rng"] = pcg(np.arange(P * n, dtype=np.uint32) + pcg(U32(frame_seed)))
    return out, np.concatenate([d, np.zeros((n, 1), np.float32)], -1)


# ---- octahedral mapping ------------------------------------------------------------------------------------------------------------------
def _sign1(x):
    return np.where(x >= 0, F(1), F(-1)).astype(np.float32)


def oct_decode(ox, oy):
    ax, ay = np.abs(ox), np.abs(oy)
    z = ((F(1) - ax) - ay).astype(np.float32)
    x = np.where(z < 0, (F(1) - ay) * _sign1(ox), ox).astype(np.float32)
    y = np.where(z < 0, (F(1) - ax) * _sign1(oy), oy).astype(np.float32)
    length = np.sqrt((x * x + y * y) + z * z).astype(np.float32)
    return np.stack([x / length, y / length, z / length], -1).astype(np.float32)


def oct_encode(d):
    s = ((np.abs(d[..., 0]) + np.abs(d[..., 1])) + np.abs(d[..., 2])).astype(np.float32)
    px, py = (d[..., 0] / s).astype(np.float32), (d[..., 1] / s).astype(np.float32)
    back = d[..., 2] < 0
    return (np.where(back, (F(1) - np.abs(py)) * _sign1(px), px).astype(np.float32), np.where(back, (F(1) - np.abs(px)) * _sign1(py), py).astype(np.float32))


def texel_directions(interior):
    """[interior * interior, 3], texel (i, j) at index j * interior + i."""
    c = (((np.arange(interior, dtype=np.float32) + F(0.5)) / F(interior)) * F(2) - F(1)).astype(np.float32)
    ox, oy = np.meshgrid(c, c)          # ox varies along i (the fast axis)
    return oct_decode(ox.ravel(), oy.ravel())


def border_source(x, y, T):
    ex, ey = x in (0, T - 1), y in (0, T - 1)
    if ex and ey:
        return (T - 2 if x == 0 else 1), (T - 2 if y == 0 else 1)
    if ey:
        return T - 1 - x, (1 if y == 0 else T - 2)
    if ex:
        return (1 if x == 0 else T - 2), T - 1 - y
    return x, y


def fill_border(tiles):
    """tiles [P, T, T, C] with the interior set; the border texels copied in place."""
    T = tiles.shape[1]
    for y in range(T):
        for x in range(T):
            sx, sy = border_source(x, y, T)
            if (sx, sy) != (x, y):
                tiles[:, y, x] = tiles[:, sy, sx]
    return tiles


def clamp_border(tiles):
    """The rule the stage does NOT use (every border texel = the nearest interior texel); kept for the test that guards the rule."""
    T = tiles.shape[1]
    for y in range(T):
        for x in range(T):
            tiles[:, y, x] = tiles[:, min(max(y, 1), T - 2), min(max(x, 1), T - 2)]
    return tiles


def lookup(tiles, probe, d, interior):
    """Bilinear lookup of tiles[probe] ([P, T, T, C]) at the unit directions d [n, 3]; probe: [n] indices. Returns [n, C]."""
    u, v = oct_encode(d)
    cx = ((u * F(0.5) + F(0.5)) * F(interior) + F(0.5)).astype(np.float32)
    cy = ((v * F(0.5) + F(0.5)) * F(interior) + F(0.5)).astype(np.float32)
    bx, by = np.floor(cx), np.floor(cy)
    x0, y0 = _clamp(bx, 0, interior).astype(np.int64), _clamp(by, 0, interior).astype(np.int64)
    fx, fy = (cx - bx).astype(np.float32)[:, None], (cy - by).astype(np.float32)[:, None]
    wx, wy = F(1) - fx, F(1) - fy
    a, b, c, e = tiles[probe, y0, x0], tiles[probe, y0, x0 + 1], tiles[probe, y0 + 1, x0], tiles[probe, y0 + 1, x0 + 1]
    return ((a * wx + b * fx) * wy + (c * wx + e * fx) * fy).astype(np.float32)


# ---- blend ---------------------------------------------------------------------------------------------------------------------------------
def ray_distances(vol, hits):
    return np.where(hits["hit"] != 0, _min(hits["t"], F(vol["maxRayDistance"])), F(vol["maxRayDistance"])).astype(np.float32)


def _history(new, old, sum_w, vol, has_history):
    h = F(vol["hysteresis"])
    blended = (new + h * (old - new)).astype(np.float32) if has_history else new
    return np.where(sum_w == 0, old, blended).astype(np.float32)


def blend(vol, directions4, radiance, hits, irradiance, distance, has_history):
    """The atlases after one update: irradiance [P, 8, 8, 4], distance [P, 16, 16, 2] (new arrays)."""
    with np.errstate(all="ignore"):
        n, P = int(vol["raysPerProbe"]), probe_count(vol)
        d = np.asarray(directions4, np.float32)[:, :3]
        L = np.asarray(radiance, np.float32).reshape(P, n, 4)
        traced = L[..., 3] != 0
        dist = ray_distances(vol, hits).reshape(P, n)
        irr_out, dist_out = np.array(irradiance, np.float32), np.array(distance, np.float32)

        def weights(interior):
            t = texel_directions(interior)
            return _max(F(0), ((t[:, None, 0] * d[None, :, 0] + t[:, None, 1] * d[None, :, 1]) + t[:, None, 2] * d[None, :, 2]).astype(np.float32))

        w_irr = weights(IRR_I)                                                                        # [36, n]
        w_dist = _fmap("or_pow")(weights(DIST_I), np.float32(vol["distanceExponent"]))            # [196, n]
        s, sw = np.zeros((P, IRR_I * IRR_I, 3), np.float32), np.zeros((P, IRR_I * IRR_I), np.float32)
        for k in range(n):
            w = np.broadcast_to(w_irr[None, :, k], sw.shape)
            use = traced[:, k, None] & (w > 0)
            s = np.where(use[..., None], s + w[..., None] * L[:, None, k, :3], s).astype(np.float32)
            sw = np.where(use, sw + w, sw).astype(np.float32)
        old = irr_out[:, 1:-1, 1:-1].reshape(P, IRR_I * IRR_I, 4)
        new = np.concatenate([s / sw[..., None], np.ones((P, IRR_I * IRR_I, 1), np.float32)], -1).astype(np.float32)
        texels = _history(new, old, sw[..., None], vol, has_history)
        texels[..., 3] = np.where(sw == 0, old[..., 3], F(1))
        irr_out[:, 1:-1, 1:-1] = texels.reshape(P, IRR_I, IRR_I, 4)

        s = np.zeros((P, DIST_I * DIST_I, 3), np.float32)
        for k in range(n):
            w = w_dist[None, :, k]
            use = (traced[:, k, None] & (w > 0))[..., None]
            dk = dist[:, k, None]
            term = np.stack([w * dk, w * (dk * dk), w + np.zeros_like(dk)], -1)
            s = np.where(use, s + term, s).astype(np.float32)
        old = dist_out[:, 1:-1, 1:-1].reshape(P, DIST_I * DIST_I, 2)
        new = (s[..., :2] / s[..., 2:3]).astype(np.float32)
        dist_out[:, 1:-1, 1:-1] = _history(new, old, s[..., 2:3], vol, has_history).reshape(P, DIST_I, DIST_I, 2)
        return fill_border(irr_out), fill_border(dist_out)


def blend64(vol, directions4, radiance, hits, irradiance, distance, has_history):
    """Float64 formulation of the blend's interior texels (no border): (irradiance rgb [P, 36, 3], distance [P, 196, 2]); NaN where no ray
    has weight (the statement keeps the old texel there)."""
    with np.errstate(all="ignore"):
        n, P = int(vol["raysPerProbe"]), probe_count(vol)
        d = np.asarray(directions4, np.float32)[:, :3].astype(np.float64)
        L = np.asarray(radiance, np.float32).reshape(P, n, 4).astype(np.float64)
        traced = (L[..., 3] != 0).astype(np.float64)
        dist = ray_distances(vol, hits).reshape(P, n).astype(np.float64)
        h = float(F(vol["hysteresis"]))
        out = []
        for interior, exponent, values, old in ((IRR_I, 1.0, L[..., :3], irradiance), (DIST_I, float(F(vol["distanceExponent"])), np.stack([dist, dist * dist], -1), distance)):
            t = texel_directions(interior).astype(np.float64)
            w = np.maximum(t @ d.T, 0.0) ** exponent                     # [T, n]
            w = np.where(w < 2.0 ** -126, 0.0, w)                        # hrt_pow flushes results below 2^-126 to zero: part of the definition
            w = w[None] * traced[:, None, :]                             # [P, T, n]
            new = np.einsum("ptk,pkc->ptc", w, values) / w.sum(-1)[..., None]
            o = np.asarray(old, np.float64)[:, 1:-1, 1:-1, :values.shape[-1]].reshape(P, interior * interior, -1)
            out.append(new + h * (o - new) if has_history else new)
        return out


# ---- query ---------------------------------------------------------------------------------------------------------------------------------
def _unit0(v):
    length = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]).astype(np.float32)
    safe = np.where(length > 0, length, F(1))
    return np.where((length > 0)[..., None], v / safe[..., None], v).astype(np.float32), length


def _dot(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(np.float32)


def query(vol, irradiance, distance, points, visibility=True):
    """float32 [n, 4] = (pi * sum / sumW, inside) at the records `points` (position, normal, view). visibility=False leaves the Chebyshev
    term out (for the test that shows it inactive)."""
    with np.errstate(all="ignore"):
        X, N, V = [np.asarray(points[k], np.float32) for k in ("position", "normal", "view")]
        finite = np.all(np.abs(np.concatenate([X, N, V], -1)) <= FLT_MAX, -1)
        X, N, V = [np.where(finite[:, None], a, F(0)).astype(np.float32) for a in (X, N, V)]      # a non-finite point answers 0 below
        irr, dist = np.asarray(irradiance, np.float32), np.asarray(distance, np.float32)
        counts = [int(c) for c in vol["counts"]]
        o, sp = np.asarray(vol["origin"], np.float32), np.asarray(vol["spacing"], np.float32)
        nb, vb = F(vol["normalBias"]), F(vol["viewBias"])
        Xb = ((X + N * nb) + V * vb).astype(np.float32)
        rel = ((Xb - o) / sp).astype(np.float32)
        top = np.array([max(c - 2, 0) for c in counts], np.float32)
        base = _min(_max(np.floor(rel), F(0)), top)
        alpha = _saturate((rel - base).astype(np.float32))
        inside = np.all((rel >= 0) & (rel <= np.array([c - 1 for c in counts], np.float32)), -1)
        base_i = base.astype(np.int64)
        n = len(X)
        s, sw = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
        for k in range(8):
            off = np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1])
            c = np.minimum(base_i + off, np.array(counts) - 1)
            tri_axis = np.where(off == 1, alpha, F(1) - alpha).astype(np.float32)
            tri = ((tri_axis[:, 0] * tri_axis[:, 1]) * tri_axis[:, 2]).astype(np.float32)
            pos = (o + c.astype(np.float32) * sp).astype(np.float32)
            p = c[:, 0] + counts[0] * (c[:, 1] + counts[1] * c[:, 2])
            to_probe, _ = _unit0((pos - X).astype(np.float32))
            wrap = ((_dot(to_probe, N) + F(1)) * F(0.5)).astype(np.float32)
            w = (wrap * wrap + F(0.2)).astype(np.float32)
            if visibility:
                bv = (Xb - pos).astype(np.float32)
                direction, dl = _unit0(bv)
                m = lookup(dist, p, direction, DIST_I)
                var = np.abs(m[:, 0] * m[:, 0] - m[:, 1]).astype(np.float32)
                diff = (dl - m[:, 0]).astype(np.float32)
                ch = (var / (var + diff * diff)).astype(np.float32)
                w = np.where((dl > 0) & (dl > m[:, 0]), w * _max((ch * ch) * ch, F(0.05)), w).astype(np.float32)
            w = _max(F(1e-6), w)
            w = np.where(w < F(0.2), w * ((w * w) / F(0.04)), w).astype(np.float32)
            w = (w * tri).astype(np.float32)
            e = lookup(irr, p, N, IRR_I)[:, :3]
            s = (s + w[:, None] * e).astype(np.float32)
            sw = (sw + w).astype(np.float32)
        out = np.concatenate([PI * (s / sw[:, None]), inside[:, None].astype(np.float32)], -1).astype(np.float32)
        out[~finite | (sw == 0)] = 0
        return out


def query64(vol, irradiance, distance, points):
    """Float64 formulation of the query's rgb [n, 3] for finite points (the float32 atlases and points taken as exact inputs)."""
    with np.errstate(all="ignore"):
        X, N, V = [np.asarray(points[k], np.float64) for k in ("position", "normal", "view")]
        irr, dist = np.asarray(irradiance, np.float64), np.asarray(distance, np.float64)
        counts = np.array([int(c) for c in vol["counts"]])
        o, sp = np.asarray(vol["origin"], np.float64), np.asarray(vol["spacing"], np.float64)
        Xb = X + N * float(F(vol["normalBias"])) + V * float(F(vol["viewBias"]))
        rel = (Xb - o) / sp
        base = np.clip(np.floor(rel), 0, np.maximum(counts - 2, 0))
        alpha = np.clip(rel - base, 0, 1)

        def unit0(v):
            length = np.linalg.norm(v, axis=-1)
            return np.where((length > 0)[:, None], v / np.where(length > 0, length, 1)[:, None], v), length

        def look(tiles, p, d, interior):
            s = np.abs(d).sum(-1)
            u, v = d[:, 0] / s, d[:, 1] / s
            back = d[:, 2] < 0
            sg = lambda x: np.where(x >= 0, 1.0, -1.0)
            u, v = np.where(back, (1 - np.abs(v)) * sg(u), u), np.where(back, (1 - np.abs(u)) * sg(v), v)
            cx, cy = (u * 0.5 + 0.5) * interior + 0.5, (v * 0.5 + 0.5) * interior + 0.5
            x0, y0 = np.clip(np.floor(cx), 0, interior).astype(int), np.clip(np.floor(cy), 0, interior).astype(int)
            fx, fy = (cx - x0)[:, None], (cy - y0)[:, None]
            return (tiles[p, y0, x0] * (1 - fx) + tiles[p, y0, x0 + 1] * fx) * (1 - fy) + (tiles[p, y0 + 1, x0] * (1 - fx) + tiles[p, y0 + 1, x0 + 1] * fx) * fy

        s, sw = np.zeros((len(X), 3)), np.zeros(len(X))
        for k in range(8):
            off = np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1])
            c = np.minimum(base.astype(int) + off, counts - 1)
            tri = np.prod(np.where(off == 1, alpha, 1 - alpha), -1)
            pos = o + c * sp
            p = c[:, 0] + counts[0] * (c[:, 1] + counts[1] * c[:, 2])
            w = (((unit0(pos - X)[0] * N).sum(-1) + 1) * 0.5) ** 2 + 0.2
            direction, dl = unit0(Xb - pos)
            m = look(dist, p, direction, DIST_I)
            var = np.abs(m[:, 0] ** 2 - m[:, 1])
            ch = var / (var + (dl - m[:, 0]) ** 2)
            w = np.where((dl > 0) & (dl > m[:, 0]), w * np.maximum(ch ** 3, 0.05), w)
            w = np.maximum(1e-6, w)
            w = np.where(w < 0.2, w * w * w / 0.04, w) * tri
            s += w[:, None] * look(irr, p, N, IRR_I)[:, :3]
            sw += w
        return np.pi * s / sw[:, None]


# ---- the query at the first hits of a G-buffer -------------------------------------------------------------------------------------------
def shade_gbuffer(vol, irradiance, distance, normal, depth, view, intensity):
    """float32 [H, W, 4]: (E * intensity, 1) at a hit, (0, 0, 0, 0) at a miss (depth.x == 1e10). World position: ReconstructWorldPos of the
    view depth; view vector: normalize(camera position - world position), as tests/modulation_reference.py forms them."""
    from temporal_reference import MISS, recon
    with np.errstate(all="ignore"):
        normal, depth = np.ascontiguousarray(normal, np.float32), np.ascontiguousarray(depth, np.float32)
        H, W = depth.shape[:2]
        u = np.broadcast_to(((np.arange(W, dtype=np.float32) + F(0.5)) / F(W))[None, :], (H, W))
        v = np.broadcast_to(((np.arange(H, dtype=np.float32) + F(0.5)) / F(H))[:, None], (H, W))
        world = recon(view, u, v, depth[..., 1])
        cam = np.asarray(view["m_CameraDirectionOrPosition"], np.float32).reshape(-1)
        to_cam = [(cam[k] - world[k]).astype(np.float32) for k in range(3)]
        length = np.sqrt((to_cam[0] * to_cam[0] + to_cam[1] * to_cam[1]) + to_cam[2] * to_cam[2]).astype(np.float32)
        pts = dict(position=np.stack(world, -1).reshape(-1, 3), normal=normal[..., :3].reshape(-1, 3),
                   view=np.stack([(c / length).astype(np.float32) for c in to_cam], -1).reshape(-1, 3))
        q = query(vol, irradiance, distance, pts)
        out = np.concatenate([(q[:, :3] * F(intensity)).astype(np.float32), np.ones((H * W, 1), np.float32)], -1).reshape(H, W, 4)
        out[depth[..., 0] == MISS] = 0
        return out
