"""Texture sampling as DESIGN.md section 2 and the contract comments of csrc/pt_texture.h (sample_texture_level / sample_texture_grad)
state it, in plain numpy: an independent statement of "bilinear / trilinear filtering of these texels", written from the text and not from
the C of either the device code or the oracle.

* Samplers (src/CommonResources.cpp:117-128 of the reference): 0 / 1 anisotropic, 2 / 3 point, 4 / 5 linear; odd = wrap, even = clamp;
  every other index is linear clamp. Anisotropic filters like linear (the only gradient caller passes an isotropic footprint).
* Footprint, in binary32, one correctly rounded operation per step: x = u * w, minus 0.5 unless the sampler is a point sampler,
  x0 = floor(x), tx = x - x0 (0 for point samplers), texel columns x0 and x0 + 1 wrapped (mathematical modulo) or clamped to [0, w - 1];
  the same in y. Every step is a single IEEE operation, so numpy's float32 gives the same footprint as any conforming implementation and
  no probe sits on a discontinuity. Domain: finite uv with |uv * size| < 2^24 (beyond that the float-to-int conversion is undefined).
* Texels decode to real numbers: UNORM b / 255; sRGB the IEC 61966-2-1 formula for r, g, b and b / 255 for alpha; binary16 / binary32
  exactly. The blends a(1 - t) + bt along x, then along y, then between two levels are evaluated here in float64 on the decoded values.
* Level l of a w x h texture is max(1, w >> l) x max(1, h >> l) texels and starts where level l - 1 ends, tightly packed; recomputed here
  from (w, h, mip count) alone.
* The level of detail is an INPUT here (the caller constructs gradients whose level of detail is exact): clamped to [0, mips - 1]; linear /
  anisotropic samplers blend floor(lod) and the next level with the fractional part, point samplers take floor(lod + 0.5).

Error bound of an fp32 implementation against this reference (M = the largest |texel| of the footprint): each a(1 - t) + bt evaluated in fp32
has at most four roundings that matter (1 - t, the two products, the sum), each at most 2^-24 relative to a quantity bounded by M, so it adds
at most 4 * 2^-24 * M; a convex blend does not amplify the error of its inputs. The two row blends run side by side, so one level costs two
blends deep = 8 units, and a level blend on top 12; one more unit covers the (1 + u) factors dropped in that first-order count and the
rounding of a decoded UNORM / sRGB texel to binary32 (an incoming error of at most one unit, which the convex blends pass on unamplified):
TOL_ONE_LEVEL = 9 * 2^-24 * M, TOL_TWO_LEVELS = 13 * 2^-24 * M. A wrong weight, neighbour or level misses by orders of magnitude more."""
import numpy as np

F32, F64 = np.float32, np.float64
FORMAT_RGBA8_UNORM, FORMAT_RGBA8_SRGB, FORMAT_RGBA16_FLOAT, FORMAT_RGBA32_FLOAT = 0, 1, 2, 3
UNIT = 2.0 ** -24
TOL_ONE_LEVEL, TOL_TWO_LEVELS = 9 * UNIT, 13 * UNIT


def sampler_modes(sampler):
    """(wrap, point) of a sampler index."""
    sampler = int(sampler)
    return (sampler in (1, 3, 5)), (sampler in (2, 3))


def level_layout(w, h, mips):
    """[(level width, level height, first texel of the level)] of a chain of `mips` levels."""
    out, first = [], 0
    for l in range(max(1, int(mips))):
        lw, lh = max(1, w >> l), max(1, h >> l)
        out.append((lw, lh, first))
        first += lw * lh
    return out


def srgb_to_linear(b):
    """IEC 61966-2-1 decoding of the byte values b, float64."""
    c = np.asarray(b, F64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def decode_levels(raw, w, h, fmt, mips):
    """Every level of a texture given as its raw bytes (level 0 first, tightly packed), decoded to float64 arrays (lh, lw, 4)."""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    kind = {FORMAT_RGBA8_UNORM: np.uint8, FORMAT_RGBA8_SRGB: np.uint8, FORMAT_RGBA16_FLOAT: np.float16, FORMAT_RGBA32_FLOAT: np.float32}[fmt]
    texels = raw.view(kind).reshape(-1, 4)
    layout = level_layout(w, h, mips)
    assert len(texels) == layout[-1][2] + layout[-1][0] * layout[-1][1], "the data does not hold exactly the chain"
    out = []
    for lw, lh, first in layout:
        t = texels[first:first + lw * lh].reshape(lh, lw, 4)
        if fmt == FORMAT_RGBA8_UNORM:
            v = t.astype(F64) / 255.0
        elif fmt == FORMAT_RGBA8_SRGB:
            v = np.concatenate([srgb_to_linear(t[..., :3]), t[..., 3:].astype(F64) / 255.0], -1)
        else:
            v = t.astype(F64)
        out.append(v)
    return out


def _axis(u, n, wrap, point):
    """One axis of the footprint, binary32 step by step: (i0, i1, t)."""
    x = u.astype(F32) * F32(n)
    if not point:
        x = x - F32(0.5)
    i = np.floor(x)
    t = np.zeros_like(x) if point else x - i
    assert x.dtype == F32 and t.dtype == F32
    assert np.isfinite(x).all() and (np.abs(x) < 2.0 ** 24).all(), "uv outside the numeric contract's domain"
    i = i.astype(np.int64)
    if wrap:
        return np.mod(i, n), np.mod(i + 1, n), t
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), t


def footprint(uv, lw, lh, sampler):
    """x0, x1, y0, y1 (texel indices) and tx, ty (binary32 weights) of the probes uv (n, 2) on a level of lw x lh texels."""
    wrap, point = sampler_modes(sampler)
    uv = np.asarray(uv, F32).reshape(-1, 2)
    x0, x1, tx = _axis(uv[:, 0], lw, wrap, point)
    y0, y1, ty = _axis(uv[:, 1], lh, wrap, point)
    return x0, x1, y0, y1, tx, ty


def sample_level(level, sampler, uv):
    """One level (float64 (lh, lw, 4), from decode_levels) filtered at uv (n, 2). Returns (value float64 (n, 4), M (n,) = the largest
    |texel| of the footprint, exact (n,) = the result is one texel: point sampler, or both weights zero)."""
    lh, lw = level.shape[:2]
    x0, x1, y0, y1, tx, ty = footprint(uv, lw, lh, sampler)
    _, point = sampler_modes(sampler)
    t00 = level[y0, x0]
    if point:
        return t00, np.abs(t00).max(-1), np.ones(len(t00), bool)
    t10, t01, t11 = level[y0, x1], level[y1, x0], level[y1, x1]
    wx, wy = tx.astype(F64)[:, None], ty.astype(F64)[:, None]
    top = t00 * (1.0 - wx) + t10 * wx
    bottom = t01 * (1.0 - wx) + t11 * wx
    value = top * (1.0 - wy) + bottom * wy
    m = np.abs(np.stack([t00, t10, t01, t11])).max((0, 2))
    return value, m, (tx == 0) & (ty == 0)


def select_levels(lod, mips, sampler):
    """(first level, second level, blend weight) for a level of detail (float64 array): the weight is 0 where one level is sampled."""
    lod = np.clip(np.asarray(lod, F64), 0.0, float(mips - 1))
    _, point = sampler_modes(sampler)
    if point:
        l0 = np.floor(lod + 0.5).astype(np.int64)
        return l0, l0, np.zeros_like(lod)
    l0 = np.floor(lod).astype(np.int64)
    l1 = np.minimum(l0 + 1, mips - 1)
    f = np.where(l1 == l0, 0.0, lod - l0)
    return l0, l1, f


def sample_lod(levels, sampler, uv, lod):
    """SampleGrad with a known level of detail per probe. Returns (value (n, 4), M (n,), two (n,) = two levels were blended)."""
    uv = np.asarray(uv, F32).reshape(-1, 2)
    l0, l1, f = select_levels(np.broadcast_to(np.asarray(lod, F64), (len(uv),)), len(levels), sampler)
    value, m, two = np.zeros((len(uv), 4)), np.zeros(len(uv)), f != 0.0
    for l in np.unique(l0):
        sel = l0 == l
        value[sel], m[sel], _ = sample_level(levels[l], sampler, uv[sel])
    for l in np.unique(l1[two]):
        sel = two & (l1 == l)
        v1, m1, _ = sample_level(levels[l], sampler, uv[sel])
        w = f[sel][:, None]
        value[sel] = value[sel] * (1.0 - w) + v1 * w
        m[sel] = np.maximum(m[sel], m1)
    return value, m, two
