"""Float64 statements of the two consumers of the motion plane, with decision margins -- TEST INFRASTRUCTURE.

temporal64 is written from SSGITemporalReproject.hlsl:28-47 (SSGIValidateReprojection), :50-82 (SSGITemporalAccumulate), :97-132 and
:155-167 (the diffuse channel of SSGITemporal_PSMain) and from Common.hlsli:50-53 (UVToClipXY), :111-164 (SampleTextureCatmullRom) and
:167-172 (ReconstructWorldPos). What the HLSL leaves open follows the five rules of DESIGN.md section 17: pixel uv is (p + 0.5) / size
and the linear-clamp sampler reads x = u * W - 0.5, floor, fraction, indices clamped to the image, a (1 - t) + b t along x then y; a point
sample at uv r reads texel clamp(floor(r * size), 0, size - 1); the depth plane holds the VIEW depth, so the device depth of
ReconstructWorldPos is z = (vd * P[2][2] + P[3][2]) / vd with P = m_MatViewToClip; a reprojection onto a miss texel has confidence 0; and
without history acc = 0 and confidence = 0. upscale64 is written from the numbered definition of DESIGN.md section 24.

Neither is written from pt_temporal.h, pt_upscale.h, temporal_reference.py or upscale_reference.py, and nothing is imported from them.
Inputs are binary32 values at their exact value (or float64 planes of an ideal chain); log, exp, pow and sqrt are libm's (NumPy float64).
A view is anything indexable by the field names of PlanarViewConstants: a record (binary32, carried exactly) or a dict of float64 arrays.

Each returns, per pixel, the output, the history, the intermediate quantities and a DECISION MARGIN: the least normalised distance to a
threshold where a binary32 evaluation may take the other side. Thresholds of temporal64: the [0, 1] inside tests of the validation's uv;
the distance of uv * size to an integer at the validation's point sample, relative to max(|uv * size|, 1); depth.x == 1e10 on the pixel
and on the sampled texel (|x / 1e10 - 1| for a hit; a miss holds the ASSIGNED constant, equal in every precision: no margin lost); the
two ends of moveFactor's saturate; accumBlend against maxValue in min(accumBlend, maxValue); disoccl / 3 against 1. Of upscale64: the distance of p - j to an integer (base texel); the
relative gap between the two smallest depth keys (tap choice) and of each key to 1e10; the inside tests of reproj; n against maxHistory.
The range clamps need none: clamp(x, lo, hi), the anti-ringing clamp of SampleTextureCatmullRom and the neighbourhood clamp are
continuous in x, lo and hi, and so are saturate and min -- the ends of saturate and min are listed all the same, because pow(c, 0.25)
behind min(disoccl / 3, 1) has an unbounded derivative at c = 0 and the others cost nothing. floor(samplePos - 0.5) of the Catmull-Rom
footprint needs none either: the filter is continuous across the step (f = 1 on one side equals f = 0 on the other, tap for tap)."""
import numpy as np

F = np.float64
INF = np.inf
FAR = F(np.float32(1e10))
c32 = lambda x: F(np.float32(x))      # noqa: E731  a shader literal at its binary32 value


def _m(view, name):
    return np.asarray(view[name], F)


def _recon(uv, vd, view):
    """ReconstructWorldPos(uv, device depth of view depth vd, m_MatClipToWorld), Common.hlsli:167-172."""
    P, M = _m(view, "m_MatViewToClip"), _m(view, "m_MatClipToWorld")
    with np.errstate(all="ignore"):
        z = (vd * P[2, 2] + P[3, 2]) / vd
        clip = np.stack([uv[..., 0] * 2.0 - 1.0, uv[..., 1] * -2.0 + 1.0, z, np.ones_like(z)], -1)
        h = clip @ M
        return h[..., :3] / h[..., 3:4]


def _axis(u, n):
    x = u * n - 0.5
    i = np.floor(x)
    t = x - i
    i = i.astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), t


def sample_linear_clamp(img, uv):
    H, W = img.shape[:2]
    x0, x1, tx = _axis(uv[..., 0], W)
    y0, y1, ty = _axis(uv[..., 1], H)
    tx, ty = tx[..., None], ty[..., None]
    top = img[y0, x0] * (1.0 - tx) + img[y0, x1] * tx
    bottom = img[y1, x0] * (1.0 - tx) + img[y1, x1] * tx
    return top * (1.0 - ty) + bottom * ty


def catmull_rom(img, uv, resolution):
    """SampleTextureCatmullRom, Common.hlsli:111-164, through the linear-clamp sampler; uv [..., 2], resolution (W, H)."""
    res = np.asarray(resolution, F)
    pos = uv * res
    p1 = np.floor(pos - 0.5) + 0.5
    f = pos - p1
    w0 = f * (-0.5 + f * (1.0 - 0.5 * f))
    w1 = 1.0 + f * f * (-2.5 + 1.5 * f)
    w2 = f * (0.5 + f * (2.0 - 1.5 * f))
    w3 = f * f * (-0.5 + 0.5 * f)
    w12 = w1 + w2
    o12 = w2 / (w1 + w2)
    p0, p3, p12 = (p1 - 1.0) / res, (p1 + 2.0) / res, (p1 + o12) / res
    p1u, p2u = p1 / res, (p1 + 1.0) / res
    at = lambda x, y: sample_linear_clamp(img, np.stack([x[..., 0], y[..., 1]], -1))      # noqa: E731
    wt = lambda a, b: (a[..., 0] * b[..., 1])[..., None]                                 # noqa: E731
    result = (at(p0, p0) * wt(w0, w0) + at(p12, p0) * wt(w12, w0) + at(p3, p0) * wt(w3, w0)
              + at(p0, p12) * wt(w0, w12) + at(p12, p12) * wt(w12, w12) + at(p3, p12) * wt(w3, w12)
              + at(p0, p3) * wt(w0, w3) + at(p12, p3) * wt(w12, w3) + at(p3, p3) * wt(w3, w3))
    c = [at(p1u, p1u), at(p2u, p1u), at(p1u, p2u), at(p2u, p2u)]
    lo = np.minimum(np.minimum(c[0], c[1]), np.minimum(c[2], c[3]))
    hi = np.maximum(np.maximum(c[0], c[1]), np.maximum(c[2], c[3]))
    return np.clip(np.maximum(result, 0.0), lo, hi)


def _length(a):
    return np.sqrt((a * a).sum(-1))


def _far_margin(x):
    """depth.x == 1e10: a render ASSIGNS the constant on a miss, so equality holds in every precision (no margin to lose); a hit's t is
    judged by its relative distance."""
    return np.where(x == FAR, INF, np.abs(x / FAR - 1.0))


def _inside_margin(r):
    return np.minimum(np.abs(r), np.abs(1.0 - r)).min(-1)


def temporal64(color, motion, depth, normal, history, view, prev_view, blend=0.9, linear=False, mutation=None):
    """One frame of the temporal stage. Images [H, W, 4]; history None: no history. Returns dict(out, history, confidence, mix, reproj
    (the uv the history is read at), validated (the uv the validation reads), miss, margin). mutation (section 33 (b)): 'motion_negated',
    'motion_zeroed', 'motion_as_uv', 'jitter_offset_sign', 'views_swapped'."""
    color, motion, depth, normal = (np.asarray(a, F) for a in (color, motion, depth, normal))
    H, W = color.shape[:2]
    if mutation == "views_swapped":
        view, prev_view = prev_view, view
    size, size_inv = _m(view, "m_ViewportSize"), _m(view, "m_ViewportSizeInv")
    assert tuple(size) == (W, H)
    x, y = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    uv = np.stack([(x + 0.5) / W, (y + 0.5) / H], -1)
    miss = depth[..., 0] == FAR
    margin = _far_margin(depth[..., 0])
    world = _recon(uv, depth[..., 1], view)
    N = normal[..., :3]
    cam = _m(view, "m_CameraDirectionOrPosition")[:3]
    mv = motion[..., :2]
    if mutation == "motion_negated":
        mv = -mv
    elif mutation == "motion_zeroed":
        mv = mv * 0.0
    velocity = mv if mutation == "motion_as_uv" else mv * size_inv
    reproj = uv + velocity
    offset = (_m(prev_view, "m_PixelOffset") - _m(view, "m_PixelOffset")) * size_inv
    validated = reproj + offset if mutation == "jitter_offset_sign" else reproj - offset
    # SSGIValidateReprojection
    inside = ((validated >= 0.0) & (validated <= 1.0)).all(-1)
    m_valid = _inside_margin(validated)
    scaled = validated * size
    with np.errstate(all="ignore"):
        m_valid = np.minimum(m_valid, (np.abs(scaled - np.round(scaled)) / np.maximum(np.abs(scaled), 1.0)).min(-1))
        qx = np.clip(np.floor(scaled[..., 0]), 0, W - 1).astype(np.int64)
        qy = np.clip(np.floor(scaled[..., 1]), 0, H - 1).astype(np.int64)
    last_depth = depth[qy, qx]
    last_velocity = -motion[qy, qx, :2] if mutation == "motion_negated" else motion[qy, qx, :2] * (0.0 if mutation == "motion_zeroed" else 1.0)
    last_velocity = last_velocity if mutation == "motion_as_uv" else last_velocity * size_inv
    last_world = _recon(validated, last_depth[..., 1], view)
    last_miss = last_depth[..., 0] == FAR
    m_valid = np.minimum(m_valid, _far_margin(last_depth[..., 0]))
    with np.errstate(all="ignore"):
        dist_factor = 1.0 + 1.0 / (_length(world - cam) + 1.0)
        delta = world - last_world
        disoccl = (_length(velocity - last_velocity) / c32(0.005) * dist_factor + np.abs((delta * N).sum(-1)) / 2.5 * dist_factor
                   + _length(delta) / 2.5 * dist_factor)
        disoccl = np.where(np.isfinite(disoccl), disoccl, INF)
        confidence = 1.0 - np.minimum(disoccl / 3.0, 1.0)
        m_valid = np.minimum(m_valid, np.where(last_miss, INF, np.abs(disoccl / 3.0 - 1.0)))
    confidence = np.where(inside & ~last_miss, confidence, 0.0)
    margin = np.minimum(margin, np.where(inside, m_valid, _inside_margin(validated)))
    # moveFactor
    speed = _length(velocity * size)
    move = np.clip(speed - 1.0, 0.0, 1.0)
    margin = np.minimum(margin, np.minimum(np.abs(speed - 1.0), np.abs(speed - 2.0)))
    # SSGITemporalAccumulate
    if history is None:
        acc = np.zeros_like(color)
        confidence = np.zeros_like(confidence)
    else:
        acc = catmull_rom(np.asarray(history, F), reproj, size)
    to = (lambda c: c) if linear else (lambda c: np.log(c + 1.0))
    back = (lambda c: c) if linear else (lambda c: np.exp(c) - 1.0)
    with np.errstate(all="ignore"):
        a_rgb, inp = to(acc[..., :3]), to(color[..., :3])
        age = acc[..., 3] + 1.0
        conf = np.power(confidence, 0.25)
        accum_blend = (1.0 - 1.0 / (age + 1.0)) * conf
        max_value = 1.0 + move * (blend - 1.0)
        mix = np.minimum(accum_blend, max_value)
        margin = np.minimum(margin, np.abs(accum_blend - max_value))
        rgb = back(inp + mix[..., None] * (a_rgb - inp))
        out_age = 1.0 / np.maximum(1.0 - mix, c32(1e-5)) - 1.0
    hist_out = np.concatenate([rgb, out_age[..., None]], -1)
    hist_out[miss] = np.concatenate([color[miss][:, :3], np.zeros((int(miss.sum()), 1))], -1)
    out = np.concatenate([hist_out[..., :3], color[..., 3:4]], -1)
    margin = np.where(miss, INF, margin)
    return dict(out=out, history=hist_out, confidence=np.where(miss, 0.0, confidence), mix=np.where(miss, 0.0, mix), reproj=reproj,
                validated=validated, miss=miss, margin=margin)


def upscale64(color, depth, motion, history, display_size, view, prev_view, jitter, kernel=2.29, max_history=8.0, no_clamp=False, mutation=None):
    """One frame of the upscale stage, DESIGN.md section 24, steps 1-7. Images [h, w, 4], history [H, W, 4] or None. Returns dict(out,
    history, cur, reproj, tap (index of the chosen tap in row-major order, -1: none), beta, margin). mutation (section 33 (b)):
    'jitter_negated', 'jitter_ignored', 'taps_unscaled', 'motion_negated', 'motion_zeroed', 'motion_as_uv', 'jitter_offset_sign',
    'views_swapped'."""
    color, depth, motion = (np.asarray(a, F) for a in (color, depth, motion))
    h, w = color.shape[:2]
    W, H = int(display_size[0]), int(display_size[1])
    if mutation == "views_swapped":
        view, prev_view = prev_view, view
    kernel, max_history = c32(kernel), c32(max_history)
    jx, jy = c32(jitter[0]), c32(jitter[1])
    if mutation == "jitter_negated":
        jx, jy = -jx, -jy
    elif mutation == "jitter_ignored":
        jx, jy = 0.0, 0.0
    rx, sx, ry, sy = w / W, W / w, h / H, H / h
    size_inv = _m(view, "m_ViewportSizeInv")
    offset = (_m(prev_view, "m_PixelOffset") - _m(view, "m_PixelOffset")) * size_inv
    X, Y = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    px, py = (X + 0.5) * rx, (Y + 0.5) * ry
    fx, fy = px - jx, py - jy
    margin = np.minimum(np.abs(fx - np.round(fx)), np.abs(fy - np.round(fy)))
    bi = np.clip(np.floor(fx), 0, w - 1).astype(np.int64)
    bj = np.clip(np.floor(fy), 0, h - 1).astype(np.int64)
    sum_c, sum_g = np.zeros((H, W, 3)), np.zeros((H, W))
    lo, hi = np.full((H, W, 3), INF), np.full((H, W, 3), -INF)
    beta = np.zeros((H, W))
    best = np.full((H, W), INF)
    tap, tap_i, tap_j = np.full((H, W), -1), np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    k = 0
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            ti, tj = np.clip(bi + di, 0, w - 1), np.clip(bj + dj, 0, h - 1)
            qx, qy = (ti + 0.5) + jx, (tj + 0.5) + jy
            dx, dy = (qx - px), (qy - py)
            if mutation != "taps_unscaled":
                dx, dy = dx * sx, dy * sy
            g = np.exp(-np.minimum(kernel * (dx * dx + dy * dy), 80.0))
            c = color[tj, ti, :3]
            sum_c += g[..., None] * c
            sum_g += g
            if not no_clamp:
                lo, hi = np.minimum(lo, c), np.maximum(hi, c)
            beta = np.maximum(beta, g)
            d = depth[tj, ti]
            key = np.where((d[..., 0] == FAR) | ~(d[..., 1] < INF), INF, d[..., 1])
            margin = np.minimum(margin, _far_margin(d[..., 0]))
            better = key < best
            tap, tap_i, tap_j = np.where(better, k, tap), np.where(better, ti, tap_i), np.where(better, tj, tap_j)
            best = np.where(better, key, best)
            k += 1
    if no_clamp:
        lo, hi = np.full((H, W, 3), -INF), np.full((H, W, 3), INF)
    cur = np.clip(sum_c / sum_g[..., None], lo, hi)
    alpha = color[bj, bi, 3]
    chosen = tap >= 0
    # the tap choice: the gap to the smallest key of ANOTHER texel (two taps of the same texel, clamped at a border, tie in every precision
    # and the first wins; two texels with equal keys have margin 0)
    second = np.full((H, W), INF)
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            ti, tj = np.clip(bi + di, 0, w - 1), np.clip(bj + dj, 0, h - 1)
            d = depth[tj, ti]
            key = np.where((d[..., 0] == FAR) | ~(d[..., 1] < INF), INF, d[..., 1])
            second = np.where((ti != tap_i) | (tj != tap_j), np.minimum(second, key), second)
    with np.errstate(all="ignore"):
        margin = np.minimum(margin, np.where(chosen & np.isfinite(second), (second - best) / np.abs(second), INF))
    m = motion[tap_j, tap_i, :2]
    if mutation == "motion_negated":
        m = -m
    elif mutation == "motion_zeroed":
        m = m * 0.0
    U = np.stack([(X + 0.5) / W, (Y + 0.5) / H], -1)
    reproj = U + (m if mutation == "motion_as_uv" else m * size_inv)
    reproj = reproj + offset if mutation == "jitter_offset_sign" else reproj - offset
    inside = ((reproj >= 0.0) & (reproj <= 1.0)).all(-1)
    margin = np.where(chosen, np.minimum(margin, _inside_margin(reproj)), margin)
    use = chosen & inside & (history is not None)
    out, n_out = cur.copy(), np.where(chosen, beta, 0.0)
    if history is not None:
        h4 = catmull_rom(np.asarray(history, F), reproj, (W, H))
        hc = np.clip(h4[..., :3], lo, hi)
        n = np.minimum(h4[..., 3], max_history)
        with np.errstate(all="ignore"):
            margin = np.where(use, np.minimum(margin, np.abs(h4[..., 3] / max_history - 1.0)), margin)
            t = beta / (n + beta)
            blended = hc + t[..., None] * (cur - hc)
        out = np.where(use[..., None], blended, cur)
        n_out = np.where(use, np.minimum(n + beta, max_history), n_out)
        margin = np.where(use, np.minimum(margin, np.abs((n + beta) / max_history - 1.0)), margin)
    return dict(out=np.concatenate([out, alpha[..., None]], -1), history=np.concatenate([out, n_out[..., None]], -1), cur=cur, reproj=reproj,
                tap=tap, beta=beta, chosen=chosen, margin=margin, tap_texel=(tap_i, tap_j))
