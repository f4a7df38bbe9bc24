"""NumPy float32 restatement of the upscale stage (hrpt_upscale), written from the stage's statement in prose,
independent of hobbyrenderer_amd/csrc/pt_upscale.h. It is the yardstick of tests/test_upscale_cpu.py and tests/test_upscale_gpu.py: the
library must produce the same BITS.

Every operation is an IEEE binary32 + - * / floor or a comparison in the order the statement writes it (sums left to right), which NumPy
rounds exactly like the C++ / HIP build (no FMA contraction there). min / max / clamp are the select forms of hobbyrt/detmath.h; exp comes
from the CPU oracle (or_exp); SampleTextureCatmullRom and the samplers under it are those of tests/temporal_reference.py.

The statement, per display pixel (X, Y) of W x H over a w x h frame, rx = w / W, sx = W / w (ry, sy likewise), jitter (jx, jy):
  p = ((X + 0.5) * rx, (Y + 0.5) * ry); base texel bi = clamp(floor(p.x - jx), 0, w - 1), bj likewise
  taps dj = -1..1, di = -1..1 row-major at texel (clamp(bi + di), clamp(bj + dj)); the tap's sample lies at q = (ti + 0.5 + jx, tj + 0.5 + jy),
  d = ((q.x - p.x) * sx, (q.y - p.y) * sy), g = exp(-min(kernel * (d.x^2 + d.y^2), 80))
  lo / hi = per-channel range of the taps (min / max from +inf / -inf; with clamping off they start, and stay, at -inf / +inf);
  cur = clamp(sum(g rgb) / sum(g), lo, hi); beta = max g; alphaOut = color(bi, bj).a
  the first hit tap (depth.x != 1e10) with the smallest depth.y below +inf gives the motion m; none: (cur, 0) and (cur, alphaOut)
  reproj = (U + m.x * sizeInv.x - jitterOffsetUV.x, ...); no history or reproj not inside [0, 1]^2: out = cur, n' = beta
  else h4 = catmull_rom(history, reproj); hc = clamp(h4.rgb, lo, hi); n = min(h4.w, maxHistory);
  t = beta / (n + beta); out = hc + t * (cur - hc); n' = min(n + beta, maxHistory)
"""
import numpy as np

import temporal_reference as TR
from temporal_reference import F, MISS, _max, _min

INF = F(np.inf)


def _exp(x):
    """or_exp of every element; the distinct arguments are few (the tap offsets repeat with the scale ratio), so each is evaluated once."""
    values, inverse = np.unique(np.asarray(x, np.float32).view(np.uint32), return_inverse=True)
    return TR._exp(values.view(np.float32))[inverse].reshape(np.shape(x))


def _base(n_display, n_render, jitter):
    """(p, base texel) along one axis: float32 [n_display], int64 [n_display]."""
    r = F(n_render) / F(n_display)
    p = ((np.arange(n_display, dtype=np.float32) + F(0.5)) * r).astype(np.float32)
    b = _min(_max(np.floor(p - F(jitter)), F(0)), F(n_render - 1)).astype(np.int64)
    return p, b


def upscale(color, depth, motion, history, display_size, view, prev_view, jitter=(0.0, 0.0), kernel=2.29, max_history=8.0, clamp=True, details=False):
    """(colorOut, historyOut) of float32 [H, W, 4] images from a float32 [h, w, 4] frame; history None = no history. details: also a dict
    of the intermediate images cur, beta, lo, hi, tap (ti, tj; -1 where no tap is a hit), reproj and the mask of pixels that blended."""
    with np.errstate(all="ignore"):
        color, depth, motion = [np.ascontiguousarray(a, np.float32) for a in (color, depth, motion)]
        h, w = color.shape[:2]
        W, H = display_size
        size = np.asarray(view["m_ViewportSize"], np.float32)
        size_inv = np.asarray(view["m_ViewportSizeInv"], np.float32)
        assert size[0] == w and size[1] == h
        jx, jy = F(jitter[0]), F(jitter[1])
        sx, sy = F(W) / F(w), F(H) / F(h)
        px, bi = _base(W, w, jx)
        py, bj = _base(H, h, jy)

        sum_rgb = np.zeros((H, W, 3), np.float32)
        sum_g = np.zeros((H, W), np.float32)
        beta = np.zeros((H, W), np.float32)
        lo = np.full((H, W, 3), INF if clamp else -INF, np.float32)          # clamping off: the range is all of the reals from the start
        hi = np.full((H, W, 3), -INF if clamp else INF, np.float32)
        best = np.full((H, W), INF, np.float32)
        mi = np.full((H, W), -1, np.int64)
        mj = np.full((H, W), -1, np.int64)
        for dj in (-1, 0, 1):
            tj = np.clip(bj + dj, 0, h - 1)
            dy = ((((tj.astype(np.float32) + F(0.5)) + jy) - py) * sy).astype(np.float32)
            for di in (-1, 0, 1):
                ti = np.clip(bi + di, 0, w - 1)
                dx = ((((ti.astype(np.float32) + F(0.5)) + jx) - px) * sx).astype(np.float32)
                r2 = (dx * dx)[None, :] + (dy * dy)[:, None]
                g = _exp(-_min(F(kernel) * r2, F(80.0)))
                c = color[tj[:, None], ti[None, :]]
                sum_rgb = sum_rgb + g[..., None] * c[..., :3]
                sum_g = sum_g + g
                lo, hi = _min(lo, c[..., :3]), _max(hi, c[..., :3])
                beta = _max(beta, g)
                d = depth[tj[:, None], ti[None, :]]
                key = np.where(d[..., 0] == MISS, INF, d[..., 1]).astype(np.float32)
                nearer = key < best
                best = np.where(nearer, key, best)
                mi = np.where(nearer, np.broadcast_to(ti[None, :], (H, W)), mi)
                mj = np.where(nearer, np.broadcast_to(tj[:, None], (H, W)), mj)
        cur = (sum_rgb / sum_g[..., None]).astype(np.float32)
        cur = _min(_max(cur, lo), hi)                        # takes back the rounding of the quotient: cur never leaves the taps' range
        alpha = color[bj[:, None], bi[None, :], 3]
        chosen = mi >= 0

        m = motion[np.maximum(mj, 0), np.maximum(mi, 0)]
        U = np.broadcast_to(((np.arange(W, dtype=np.float32) + F(0.5)) / F(W))[None, :], (H, W))
        V = np.broadcast_to(((np.arange(H, dtype=np.float32) + F(0.5)) / F(H))[:, None], (H, W))
        offset = (np.asarray(prev_view["m_PixelOffset"], np.float32) - np.asarray(view["m_PixelOffset"], np.float32)) * size_inv
        ru = (U + m[..., 0] * size_inv[0]) - offset[0]
        rv = (V + m[..., 1] * size_inv[1]) - offset[1]
        inside = (ru >= 0) & (ru <= 1) & (rv >= 0) & (rv <= 1)

        out, n1 = cur, beta
        blended = np.zeros((H, W), bool)
        if history is not None:
            history = np.ascontiguousarray(history, np.float32)
            assert history.shape == (H, W, 4)
            blended = chosen & inside
            h4 = TR.catmull_rom(history, ru, rv, F(W), F(H))
            hc = _min(_max(h4[..., :3], lo), hi)
            n = _min(h4[..., 3], F(max_history))
            t = beta / (n + beta)
            mixed = (hc + t[..., None] * (cur - hc)).astype(np.float32)
            out = np.where(blended[..., None], mixed, cur)
            n1 = np.where(blended, _min(n + beta, F(max_history)), beta)
        n1 = np.where(chosen, n1, F(0)).astype(np.float32)
        history_out = np.concatenate([out, n1[..., None]], -1).astype(np.float32)
        color_out = np.concatenate([out, alpha[..., None]], -1).astype(np.float32)
    if details:
        return color_out, history_out, {"cur": cur, "beta": beta, "lo": lo, "hi": hi, "tap": (mi, mj), "reproj": (ru, rv), "blended": blended}
    return color_out, history_out


def bilinear_upsample(frame, display_size):
    """The yardstick of the convergence tests: the linear-clamp sampler over one render-size frame at every display pixel's uv."""
    W, H = display_size
    U = np.broadcast_to(((np.arange(W, dtype=np.float32) + F(0.5)) / F(W))[None, :], (H, W))
    V = np.broadcast_to(((np.arange(H, dtype=np.float32) + F(0.5)) / F(H))[:, None], (H, W))
    return TR.sample_linear(np.ascontiguousarray(frame, np.float32), U, V)
