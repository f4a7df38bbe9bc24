"""NumPy float32 restatement of the temporal stage (hrpt_temporal_accumulate): the reference's
src/shaders/SSGITemporalReproject.hlsl with SampleTextureCatmullRom and ReconstructWorldPos of src/shaders/Common.hlsli, written from the
HLSL and the issue's statement, independent of hobbyrenderer_amd/csrc/pt_temporal.h. It is the yardstick of tests/test_temporal_cpu.py and
tests/test_temporal_gpu.py: the library must produce the same BITS.

Every operation is an IEEE binary32 + - * / sqrt floor or a comparison in the order the HLSL writes it (sums and dot products left to
right), which NumPy rounds exactly like the C++ / HIP build (no FMA contraction there). min / max / clamp are the select forms of
hobbyrt/detmath.h; log2, exp and pow come from the CPU oracle (oracle.binding: or_log2, or_exp, or_pow), log(x) = log2(x) * 0.69314718.

What the HLSL leaves open is fixed as follows:
  * pixel uv ((px + 0.5) / W, (py + 0.5) / H); the linear-clamp sampler is the one of the bloom stage (x = u * W - 0.5, x0 = floor(x),
    fx = x - x0, texels x0 and x0 + 1 clamped to the image, a * (1 - fx) + b * fx along x, then along y), on all four channels
  * point sampling at uv r reads texel (clamp(floor(r.x * W), 0, W - 1), clamp(floor(r.y * H), 0, H - 1))
  * the depth plane holds VIEW depth vd in .y; device depth z = (vd * P[2][2] + P[3][2]) / vd with P = m_MatViewToClip
  * miss: depth.x == 1e10 -> (colour, age 0) passes through; a reprojection onto a miss texel has confidence 0
  * no history: acc = 0 and confidence = 0
"""
import numpy as np

F = np.float32
MISS = F(1e10)
LN2 = F(0.69314718)
EPSILON = F(1e-5)          # srrhi::CommonConsts::kEpsilon


def _fmap(name):
    from oracle.binding import lib
    fn = getattr(lib(), name)

    def apply(*arrays):
        arrays = np.broadcast_arrays(*[np.asarray(a, np.float32) for a in arrays])
        flat = [a.ravel().tolist() for a in arrays]
        return np.array([fn(*xs) for xs in zip(*flat)], np.float32).reshape(arrays[0].shape)
    return apply


def _log(x):
    return (_fmap("or_log2")(x) * LN2).astype(np.float32)


def _exp(x):
    return _fmap("or_exp")(x)


def _pow(x, y):
    return _fmap("or_pow")(x, np.full(np.shape(x), y, np.float32))


def _min(a, b):            # hrt_min: (a <= b || b != b) ? a : b
    a, b = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32))
    return np.where((a <= b) | (b != b), a, b).astype(np.float32)


def _max(a, b):            # hrt_max: (a >= b || b != b) ? a : b
    a, b = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32))
    return np.where((a >= b) | (b != b), a, b).astype(np.float32)


def _clamp(x, lo, hi):
    return _min(_max(x, F(lo)), F(hi))


def _saturate(x):
    return np.where(x > 0, np.where(x < 1, x, F(1)), F(0)).astype(np.float32)


def _lerp(a, b, t):
    return (a + t * (b - a)).astype(np.float32)


def _length(*c):
    s = c[0] * c[0] + c[1] * c[1]
    if len(c) == 3:
        s = s + c[2] * c[2]
    return np.sqrt(s).astype(np.float32)


# ---- samplers ----------------------------------------------------------------------------------------------------------------------------
def _axis(coord, n):
    x = coord * F(n) - F(0.5)
    x0 = np.floor(x)
    f = (x - x0).astype(np.float32)
    i = _clamp(x0, -1, n).astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), f


def sample_linear(tex, u, v):
    """SampleLevel(linearClamp, (u, v), 0) of tex[h, w, 4], all four channels."""
    h, w = tex.shape[:2]
    x0, x1, fx = _axis(u, w)
    y0, y1, fy = _axis(v, h)
    fx, fy = fx[..., None], fy[..., None]
    top = tex[y0, x0] * (F(1) - fx) + tex[y0, x1] * fx
    bottom = tex[y1, x0] * (F(1) - fx) + tex[y1, x1] * fx
    return (top * (F(1) - fy) + bottom * fy).astype(np.float32)


def point_index(r, n):
    return _clamp(np.floor(r * F(n)), 0, n - 1).astype(np.int64)


def _catmull_axis(uv, res):
    sample_pos = uv * res
    tex_pos1 = np.floor(sample_pos - F(0.5)) + F(0.5)
    f = sample_pos - tex_pos1
    w0 = f * (F(-0.5) + f * (F(1) - F(0.5) * f))
    w1 = F(1) + f * f * (F(-2.5) + F(1.5) * f)
    w2 = f * (F(0.5) + f * (F(2) - F(1.5) * f))
    w3 = f * f * (F(-0.5) + F(0.5) * f)
    w12 = w1 + w2
    offset12 = w2 / (w1 + w2)
    tex_pos0 = tex_pos1 - F(1)
    tex_pos3 = tex_pos1 + F(2)
    tex_pos12 = tex_pos1 + offset12
    return {"w": (w0, w12, w3), "uv": (tex_pos0 / res, tex_pos12 / res, tex_pos3 / res), "c": (tex_pos1 / res, (tex_pos1 + F(1)) / res)}


def catmull_rom(tex, u, v, res_x, res_y):
    """SampleTextureCatmullRom(tex, linearClamp, (u, v), (res_x, res_y)), Common.hlsli:111-164."""
    X, Y = _catmull_axis(u, res_x), _catmull_axis(v, res_y)
    result = np.zeros(u.shape + (4,), np.float32)
    for j in range(3):
        for i in range(3):
            s = sample_linear(tex, X["uv"][i], Y["uv"][j])
            result = result + s * X["w"][i][..., None] * Y["w"][j][..., None]
    c00 = sample_linear(tex, X["c"][0], Y["c"][0])
    c10 = sample_linear(tex, X["c"][1], Y["c"][0])
    c01 = sample_linear(tex, X["c"][0], Y["c"][1])
    c11 = sample_linear(tex, X["c"][1], Y["c"][1])
    lo = _min(_min(c00, c10), _min(c01, c11))
    hi = _max(_max(c00, c10), _max(c01, c11))
    return _min(_max(_max(result, F(0)), lo), hi)


# ---- ReconstructWorldPos from a view depth -------------------------------------------------------------------------------------------------
def recon(view, u, v, vd):
    P = np.asarray(view["m_MatViewToClip"], np.float32)
    M = np.asarray(view["m_MatClipToWorld"], np.float32)
    z = (vd * P[2, 2] + P[3, 2]) / vd
    cx = u * F(2) + F(-1)
    cy = v * F(-2) + F(1)
    h = [((cx * M[0, k] + cy * M[1, k]) + z * M[2, k]) + F(1) * M[3, k] for k in range(4)]
    return [(h[k] / h[3]).astype(np.float32) for k in range(3)]


# ---- the pass --------------------------------------------------------------------------------------------------------------------------------
def temporal(color, motion, depth, normal, history, view, prev_view, blend=0.9, linear=False, details=False):
    """(colorOut, historyOut) of float32 [H, W, 4] images; history None = no history. details: also a dict of intermediate images."""
    with np.errstate(all="ignore"):
        color, motion, depth, normal = [np.ascontiguousarray(a, np.float32) for a in (color, motion, depth, normal)]
        H, W = color.shape[:2]
        size = np.asarray(view["m_ViewportSize"], np.float32)
        size_inv = np.asarray(view["m_ViewportSizeInv"], np.float32)
        assert size[0] == W and size[1] == H
        miss = depth[..., 0] == MISS

        u = np.broadcast_to(((np.arange(W, dtype=np.float32) + F(0.5)) / F(W))[None, :], (H, W))
        v = np.broadcast_to(((np.arange(H, dtype=np.float32) + F(0.5)) / F(H))[:, None], (H, W))
        world = recon(view, u, v, depth[..., 1])
        cam = np.asarray(view["m_CameraDirectionOrPosition"], np.float32)

        vel_u = motion[..., 0] * size_inv[0]
        vel_v = motion[..., 1] * size_inv[1]
        ru, rv = u + vel_u, v + vel_v
        jitter = (np.asarray(prev_view["m_PixelOffset"], np.float32) - np.asarray(view["m_PixelOffset"], np.float32)) * size_inv
        nu, nv = ru - jitter[0], rv - jitter[1]

        # SSGIValidateReprojection
        if history is None:
            confidence = np.zeros((H, W), np.float32)
            acc = np.zeros((H, W, 4), np.float32)
        else:
            history = np.ascontiguousarray(history, np.float32)
            outside = (nu < 0) | (nu > 1) | (nv < 0) | (nv > 1)
            qx, qy = point_index(nu, W), point_index(nv, H)
            last_depth = depth[qy, qx]
            last_motion = motion[qy, qx]
            lvu, lvv = last_motion[..., 0] * size_inv[0], last_motion[..., 1] * size_inv[1]
            last_world = recon(view, nu, nv, last_depth[..., 1])
            view_dist = _length(world[0] - cam[0], world[1] - cam[1], world[2] - cam[2])
            dist_factor = F(1) + F(1) / (view_dist + F(1))
            d = [world[k] - last_world[k] for k in range(3)]
            disoccl = np.zeros((H, W), np.float32)
            disoccl = disoccl + _length(vel_u - lvu, vel_v - lvv) / F(0.005) * dist_factor
            disoccl = disoccl + np.abs((d[0] * normal[..., 0] + d[1] * normal[..., 1]) + d[2] * normal[..., 2]) / F(2.5) * dist_factor
            disoccl = disoccl + _length(*d) / F(2.5) * dist_factor
            disoccl = _min(disoccl / F(3), F(1))
            confidence = np.where(outside | (last_depth[..., 0] == MISS), F(0), F(1) - disoccl).astype(np.float32)
            acc = catmull_rom(history, ru, rv, size[0], size[1])
        raw_confidence = confidence

        move = _saturate(_length(vel_u * size[0], vel_v * size[1]) - F(1))

        # SSGITemporalAccumulate
        inp = color[..., :3]
        acc_rgb = acc[..., :3]
        if not linear:
            acc_rgb = _log(acc_rgb + F(1))
            inp = _log(inp + F(1))
        acc_a = acc[..., 3] + F(1)
        confidence = _pow(confidence, 0.25)
        accum_blend = F(1) - F(1) / (acc_a + F(1))
        accum_blend = _lerp(F(0), accum_blend, confidence)
        max_value = _lerp(F(1), F(blend), move)
        mix = _min(accum_blend, max_value)
        out = _lerp(inp, acc_rgb, mix[..., None])
        age = F(1) / _max(F(1) - mix, EPSILON) - F(1)
        if not linear:
            out = _exp(out) - F(1)

        history_out = np.concatenate([out, age[..., None]], -1).astype(np.float32)
        color_out = np.concatenate([out, color[..., 3:4]], -1).astype(np.float32)
        history_out[miss] = np.concatenate([color[..., :3], np.zeros((H, W, 1), np.float32)], -1)[miss]
        color_out[miss] = color[miss]
    if details:
        return color_out, history_out, {"confidence": raw_confidence, "mix": mix, "move": move, "miss": miss, "reproj": (ru, rv), "nojitter": (nu, nv)}
    return color_out, history_out
