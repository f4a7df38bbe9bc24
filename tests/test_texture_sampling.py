"""Texture sampling pinned to an independent reference, off the render path (CPU part): the oracle's sampler (or_sample_texture /
or_sample_texture_grad) against tests/texture_reference.py, a float64 statement of the written contract, over every format x sampler x
size class the shader can meet -- point samplers, sampler indices above 5, RGBA32F, 1 x N and non-power-of-two sizes, chains whose short
side reaches 1 first, clamp and wrap far outside [0, 1], negative uv, levels of detail exactly on a level, half-way and beyond both ends.
Image parity cannot show an error the device code and the oracle share (a wrong half-texel offset, a transposed weight, a wrong level
size); this can. The GPU part (tests/test_texture_sampling_gpu.py) runs the same probes through hrpt_selftest_sample_textures.

Tolerance (derivation in texture_reference.py): |got - ref| <= 9 * 2^-24 * M for one level, 13 * 2^-24 * M for a blend of two levels,
M = the largest |texel| of the footprint: 4 units per fp32 a(1 - t) + bt (the rounding of 1 - t, two products, a sum), two blends deep
for one level and three for two, convex blends passing incoming error on unamplified, plus one unit for the (1 + u) factors and the
rounding of a decoded 8-bit texel. Where the footprint is a single texel (point samplers everywhere, linear ones where both weights are
zero) the result must be that texel's binary32 decode exactly."""
import functools

import numpy as np
import pytest

import texture_reference as R
from hobbyrenderer_amd import scenes, structs as S

F32 = np.float32
# (width, height, levels): single-level sizes, then full chains down to 1 x 1 (32 x 4 and 33 x 17: the short side is 1 for several levels)
SIZES = [(1, 1, 1), (1, 7, 1), (7, 1, 1), (2, 2, 1), (5, 3, 1), (16, 16, 1), (16, 16, 5), (32, 4, 6), (33, 17, 6)]
SAMPLERS = [0, 1, 2, 3, 4, 5, 6, 0xFFFFFFFF]
LINEAR_CLAMP, LINEAR_WRAP, POINT_CLAMP, POINT_WRAP = 4, 5, 2, 3
FORMATS = [S.TEXTURE_FORMAT_RGBA8_UNORM, S.TEXTURE_FORMAT_RGBA8_SRGB, S.TEXTURE_FORMAT_RGBA16_FLOAT, S.TEXTURE_FORMAT_RGBA32_FLOAT]
FORMAT_IDS = ["unorm8", "srgb8", "rgba16f", "rgba32f"]
UV_RANGE = 3.25
FIRST_TEXTURE = 11          # SceneBuilder keeps the reference's 11 default-texture slots (left unbound here) in front


def random_texture(rng, w, h, fmt, mips, positive=False):
    """Random texels of every level; the float formats include negative values and values above 1 unless `positive`."""
    n = sum(lw * lh for lw, lh, _ in R.level_layout(w, h, mips))
    if fmt in (S.TEXTURE_FORMAT_RGBA8_UNORM, S.TEXTURE_FORMAT_RGBA8_SRGB):
        data = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    else:
        v = rng.random((n, 4)) * 1.5 if positive else rng.normal(size=(n, 4)) * 1.5
        data = v.astype(np.float16 if fmt == S.TEXTURE_FORMAT_RGBA16_FLOAT else np.float32)
    return S.Texture(data, w, h, fmt, mips)


def dummy_luts():
    """Sampling never reads the atmosphere tables: zeros of the right shapes keep the CPU tests off the 40-second precomputation."""
    return (np.zeros(S.LUT_TRANSMITTANCE_SHAPE, F32), np.zeros(S.LUT_SCATTERING_SHAPE, F32), np.zeros(S.LUT_IRRADIANCE_SHAPE, F32))


def probe_scene(luts, textures, materials):
    """One quad, the given textures (indices from FIRST_TEXTURE) and one material per dict of `materials` (indices from 1)."""
    b = scenes.SceneBuilder()
    m = b.add_mesh(*scenes.generate_floor_quad())
    b.add_instance(m, b.add_material())
    for t in textures:
        b.add_texture(t)
    for kw in materials:
        b.add_material(**kw)
    return b.finalize(luts)


def _axis_candidates(sizes):
    """Every texel centre (i + 0.5) / n and edge i / n of every level size up to UV_RANGE, 0, -0.0, 1 and the negatives of all of these."""
    vals = [np.array([0.0, 1.0], F32)]
    for n in sorted(set(sizes)):
        i = np.arange(0, int(np.ceil(UV_RANGE * n)) + 1).astype(F32)
        vals += [(i + F32(0.5)) / F32(n), i / F32(n)]
    v = np.unique(np.concatenate(vals))
    v = v[v <= UV_RANGE]
    return np.concatenate([v, -v])             # -v holds -0.0


def uv_probes(rng, w, h, mips):
    """The probe grid of one texture: every axis candidate at least twice (paired at random with a candidate of the other axis), every
    pair of level-0 texel centres, centre pairs in the repeats of the texture, and 300 random points."""
    layout = R.level_layout(w, h, mips)
    xs, ys = _axis_candidates([l[0] for l in layout]), _axis_candidates([l[1] for l in layout])
    n = max(len(xs), len(ys))
    parts = [np.stack([xs[rng.permutation(n) % len(xs)], ys[rng.permutation(n) % len(ys)]], 1) for _ in range(2)]
    i, j = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
    i = np.concatenate([i.reshape(-1), rng.integers(-3 * w, 3 * w, 300)]).astype(F32)
    j = np.concatenate([j.reshape(-1), rng.integers(-3 * h, 3 * h, 300)]).astype(F32)
    parts.append(np.stack([(i + F32(0.5)) / F32(w), (j + F32(0.5)) / F32(h)], 1))
    parts.append(rng.uniform(-UV_RANGE, UV_RANGE, (300, 2)).astype(F32))
    uv = np.concatenate(parts).astype(F32)
    assert (np.abs(uv) <= UV_RANGE).all()
    return uv


def exact_gradient(k, n):
    """A binary32 g with fl(g * n) == 2^k exactly (g = 2^k / n itself when n is a power of two)."""
    target = F32(2.0 ** k)
    g = target / F32(n)
    for c in (g, np.nextafter(g, F32(np.inf)), np.nextafter(g, F32(-np.inf))):
        if F32(c * F32(n)) == target:
            return c
    raise AssertionError(f"no binary32 gradient gives 2^{k} over {n} texels")


def gradient_probes(rng, uv, w, h, mips, per_lod):
    """Gradients whose level of detail is exact: ddx = (2^k / w, 0), ddy = 0 gives rho^2 = 4^k, lod = k; ddx = (2^k / w, 2^k / h) gives
    rho^2 = 2 * 4^k, lod = k + 0.5 (odd k: the same in ddy, ddx = 0: the max of the two picks either); k from below 0 to beyond the last
    level so that both clamps are hit; and zero gradients (level 0). Returns (uv, ddx, ddy, lod): one block of the same `per_lod` points per
    level of detail."""
    ks = range(-2, mips + 2) if mips > 1 else (-1, 0, 2)
    rows = [((0.0, 0.0), 0.0)]
    for k in ks:
        gx, gy = exact_gradient(k, w), exact_gradient(k, h)
        rows += [((gx, 0.0), float(k)), ((gx, gy), k + 0.5)]
    out = [[], [], [], []]
    sub = uv[rng.choice(len(uv), min(len(uv), per_lod), replace=False)]          # the same points at every level of detail
    for r, (g, lod) in enumerate(rows):
        gg = np.tile(np.array(g, F32), (len(sub), 1))
        zz = np.zeros_like(gg)
        for lst, a in zip(out, (sub, zz if r % 2 else gg, gg if r % 2 else zz, np.full(len(sub), lod))):
            lst.append(a)
    return tuple(np.concatenate(a) for a in out)


def contract_lod(ddx, ddy, w, h, log2):
    """The level of detail before the clamp as the contract computes it, binary32 step by step (log2: the shared hrt_log2)."""
    ax, ay, bx, by = ddx[:, 0] * F32(w), ddx[:, 1] * F32(h), ddy[:, 0] * F32(w), ddy[:, 1] * F32(h)
    rho2 = np.maximum(ax * ax + ay * ay, bx * bx + by * by)
    assert rho2.dtype == F32
    return np.array([F32(0.5) * F32(log2(float(r))) if r > 0 else F32(0.0) for r in rho2], F32)


class Case:
    """One format: the nine textures of SIZES, one material per (texture, sampler) with the texture in the albedo slot, the probes of
    every texture, and the reference's answers. 8-bit formats share their bytes so that sRGB against UNORM is a comparison."""

    def __init__(self, fmt):
        self.fmt = fmt
        eight = fmt in (S.TEXTURE_FORMAT_RGBA8_UNORM, S.TEXTURE_FORMAT_RGBA8_SRGB)
        rng = np.random.default_rng(1000 if eight else 1000 + fmt)
        self.textures = [random_texture(rng, w, h, fmt, mips) for w, h, mips in SIZES]
        self.levels = [R.decode_levels(t.data, w, h, fmt, mips) for t, (w, h, mips) in zip(self.textures, SIZES)]
        self.materials = [dict(m_TextureFlags=S.TEXFLAG_ALBEDO, m_AlbedoTextureIndex=FIRST_TEXTURE + ti, m_AlbedoSamplerIndex=s)
                          for ti in range(len(SIZES)) for s in SAMPLERS]
        prng = np.random.default_rng(77)          # the probes do not depend on the format
        self.uv, self.grad = [], []
        for w, h, mips in SIZES:
            uv = uv_probes(prng, w, h, mips)
            self.uv.append(uv)
            self.grad.append(gradient_probes(prng, uv, w, h, mips, 96 if mips > 1 else 64))

    def material(self, ti, si):
        return 1 + ti * len(SAMPLERS) + si

    def scene(self, luts):
        return probe_scene(luts, self.textures, self.materials)

    @functools.cached_property
    def reference(self):
        """{(texture, sampler slot): ((value, M, exact) at level 0, (value, M, two) of the gradient probes)}"""
        out = {}
        for ti in range(len(SIZES)):
            guv, _, _, lod = self.grad[ti]
            for si, s in enumerate(SAMPLERS):
                out[ti, si] = (R.sample_level(self.levels[ti][0], s, self.uv[ti]), R.sample_lod(self.levels[ti], s, guv, lod))
        return out

    @functools.cached_property
    def oracle(self):
        """{(texture, sampler slot): (level-0 results, gradient results)} of the oracle, float32 (n, 4) each."""
        from oracle.binding import Oracle
        o = Oracle(self.scene(dummy_luts()))
        out = {}
        for ti in range(len(SIZES)):
            guv, ddx, ddy, _ = self.grad[ti]
            for si, s in enumerate(SAMPLERS):
                out[ti, si] = (o.sample_texture(FIRST_TEXTURE + ti, s, self.uv[ti]), o.sample_texture_grad(FIRST_TEXTURE + ti, s, guv, ddx, ddy))
        o.close()
        return out


@functools.lru_cache(maxsize=None)
def case(fmt):
    return Case(fmt)


def assert_exact_texels(c, got, who):
    """Where the footprint is one texel the result is that texel's binary32 decode, bit for bit: np.float32 of the float64 decode (for
    sRGB that is how include/hobbyrt/srgb_table.h says it was generated; for UNORM it equals the binary32 division, checked below)."""
    for (ti, si), ((value, _, exact), _) in c.reference.items():
        lvl0 = got[ti, si][0]
        _, point = R.sampler_modes(SAMPLERS[si])
        assert exact.all() if point else exact.sum() >= min(SIZES[ti][0] * SIZES[ti][1], 4), (SIZES[ti], SAMPLERS[si], int(exact.sum()))
        want = value[exact].astype(F32)
        bad = lvl0[exact].view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), f"{who}: {int(bad.sum())} single-texel results differ from the decoded texel, {SIZES[ti]} sampler {SAMPLERS[si]}: " \
                              f"uv {c.uv[ti][exact][bad.any(1)][0]} got {lvl0[exact][bad.any(1)][0]} want {want[bad.any(1)][0]}"


def assert_within_tolerance(c, got, who):
    """Every probe within 9 (one level) / 13 (two levels) units of 2^-24 * M of the float64 reference; returns the largest misses in units."""
    worst = [0.0, 0.0]
    for (ti, si), ((value, m, _), (gvalue, gm, two)) in c.reference.items():
        lvl0, grad = got[ti, si]
        for name, g, v, mm, tol in (("level 0", lvl0, value, m, np.full(len(m), R.TOL_ONE_LEVEL)),
                                    ("gradient", grad, gvalue, gm, np.where(two, R.TOL_TWO_LEVELS, R.TOL_ONE_LEVEL))):
            err = np.abs(g.astype(np.float64) - v).max(1)
            units = err / (R.UNIT * np.maximum(mm, 1e-300))
            for k, sel in enumerate((tol == R.TOL_ONE_LEVEL, tol == R.TOL_TWO_LEVELS)):
                if sel.any():
                    worst[k] = max(worst[k], float(units[sel].max()))
            bad = err > tol * mm
            assert not bad.any(), f"{who}, {name}: {int(bad.sum())} of {len(bad)} probes beyond the bound, {SIZES[ti]} sampler {SAMPLERS[si]}: " \
                                  f"worst {units.max():.1f} units of 2^-24 M at probe {int(units.argmax())}"
    print(f"{who} {FORMAT_IDS[c.fmt]}: worst one-level error {worst[0]:.2f}, two-level {worst[1]:.2f} units of 2^-24 M (bounds 9 / 13)")
    return worst


def assert_sensitivity(c, got, who):
    """Each axis of the matrix must matter, or the comparison above compared nothing: wrap against clamp outside [0, 1], point against
    linear off the texel centres, level k against k + 1."""
    slot = {s: i for i, s in enumerate(SAMPLERS)}
    for ti, (w, h, mips) in enumerate(SIZES):
        if w * h == 1:
            continue                        # one texel: every sampler returns it everywhere
        uv = c.uv[ti]
        outside = ((uv < 0) | (uv > 1)).any(1)
        inside = ((uv * F32([w, h]) >= 0.5) & (uv * F32([w, h]) <= F32([w, h]) - F32(0.5))).all(1)
        for clamp, wrap in ((LINEAR_CLAMP, LINEAR_WRAP), (POINT_CLAMP, POINT_WRAP), (0, 1)):
            a, b = got[ti, slot[clamp]][0], got[ti, slot[wrap]][0]
            assert (a[outside] != b[outside]).any(1).mean() > 0.25, f"{who}: wrap and clamp agree outside [0, 1], {SIZES[ti]} samplers {clamp} / {wrap}"
            assert np.array_equal(a[inside], b[inside]) and inside.sum() >= 4, f"{who}: wrap and clamp differ where no texel index leaves the texture, {SIZES[ti]}"
        off = ~c.reference[ti, slot[LINEAR_WRAP]][0][2]
        a, b = got[ti, slot[POINT_WRAP]][0], got[ti, slot[LINEAR_WRAP]][0]
        assert (a[off] != b[off]).any(1).mean() > 0.5, f"{who}: point and linear agree off the texel centres, {SIZES[ti]}"
        for s in (6, 0xFFFFFFFF):           # above 5: linear clamp
            assert np.array_equal(got[ti, slot[s]][0], got[ti, slot[LINEAR_CLAMP]][0]) and np.array_equal(got[ti, slot[s]][1], got[ti, slot[LINEAR_CLAMP]][1])
        if mips > 1:
            lod = c.grad[ti][3]
            n = int((lod == 0.5).sum())     # points per level of detail (the same points in every block)
            for s in (LINEAR_WRAP, POINT_CLAMP):
                g = got[ti, slot[s]][1]
                at = {float(l): g[lod == l][-n:] for l in np.unique(lod)}
                for k in range(mips - 1):
                    assert (at[k] != at[k + 1]).any(1).mean() > 0.5, f"{who}: levels {k} and {k + 1} give the same samples, {SIZES[ti]} sampler {s}"
                    if s == LINEAR_WRAP:
                        assert (at[k + 0.5] != at[k]).any(1).mean() > 0.5 and (at[k + 0.5] != at[k + 1]).any(1).mean() > 0.5, \
                            f"{who}: the half-way blend equals one of its levels, {SIZES[ti]}"
                    else:                   # point samplers take the nearest level, and half-way is the upper one
                        assert np.array_equal(at[k + 0.5], at[k + 1]), f"{who}: point sampling at lod {k + 0.5} is not level {k + 1}, {SIZES[ti]}"
                assert np.array_equal(at[-2.0], at[0.0]) and np.array_equal(at[mips + 1.0], at[mips - 1.0]), f"{who}: the level of detail is not clamped to the chain, {SIZES[ti]}"
                if s == POINT_CLAMP:        # the last level is 1 x 1: its one texel everywhere
                    assert (at[mips - 1.0] == at[mips - 1.0][0]).all(), f"{who}: the last level is not a single texel, {SIZES[ti]}"


def test_log2_is_exact_on_the_powers_of_two_the_gradient_probes_use():
    from oracle.binding import lib
    for e in range(-12, 40):
        assert lib().or_log2(2.0 ** e) == float(e), e


def test_gradient_probes_have_the_stated_level_of_detail():
    """rho^2 and 0.5 * log2(rho^2) evaluated in binary32 as the contract states them give exactly k or k + 0.5 for every gradient probe."""
    from oracle.binding import lib
    c = case(S.TEXTURE_FORMAT_RGBA8_UNORM)
    seen = set()
    for (w, h, mips), (_, ddx, ddy, lod) in zip(SIZES, c.grad):
        rows = np.unique(np.concatenate([ddx, ddy, lod[:, None].astype(F32)], 1), axis=0)
        got = contract_lod(rows[:, 0:2], rows[:, 2:4], w, h, lib().or_log2)
        assert np.array_equal(got, rows[:, 4]), (w, h)
        seen |= set(np.clip(rows[:, 4], 0, mips - 1) - np.floor(np.clip(rows[:, 4], 0, mips - 1)))
        if mips > 1:
            assert rows[:, 4].min() < 0 and rows[:, 4].max() > mips - 1          # both clamps are hit
    assert seen == {0.0, 0.5}


def test_unorm_decode_is_the_binary32_division():
    b = np.arange(256)
    assert np.array_equal((b / 255.0).astype(F32), b.astype(F32) / F32(255.0))


def test_reference_restates_the_layout_independently():
    """Level sizes and offsets of the reference (recomputed from w, h and the level count) against the package's own helpers."""
    for (w, h, mips), t in zip(SIZES, case(S.TEXTURE_FORMAT_RGBA32_FLOAT).textures):
        lv = R.decode_levels(t.data, w, h, t.format, mips)
        assert [(x.shape[1], x.shape[0]) for x in lv] == S.mip_dims(w, h, mips)
        for l in range(mips):
            assert np.array_equal(lv[l], t.level(l).astype(np.float64))
    assert R.level_layout(32, 4, 6) == [(32, 4, 0), (16, 2, 128), (8, 1, 160), (4, 1, 168), (2, 1, 172), (1, 1, 174)]


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_oracle_sampler_equals_the_reference(fmt):
    """or_sample_texture / or_sample_texture_grad over the whole matrix: exact single-texel results, the derived bound elsewhere, and every
    axis of the matrix changing the result."""
    c = case(fmt)
    assert_exact_texels(c, c.oracle, "oracle")
    assert_within_tolerance(c, c.oracle, "oracle")
    assert_sensitivity(c, c.oracle, "oracle")


def test_srgb_and_unorm_decode_the_same_bytes_differently():
    u, s = case(S.TEXTURE_FORMAT_RGBA8_UNORM), case(S.TEXTURE_FORMAT_RGBA8_SRGB)
    for ti in range(len(SIZES)):
        assert np.array_equal(u.textures[ti].data, s.textures[ti].data)
        for si in range(len(SAMPLERS)):
            for k in range(2):
                a, b = u.oracle[ti, si][k], s.oracle[ti, si][k]
                assert np.array_equal(a[:, 3], b[:, 3]) and (a[:, :3] != b[:, :3]).any(1).mean() > 0.9, (SIZES[ti], SAMPLERS[si])


def test_oracle_samples_unbound_and_out_of_range_textures_as_zero():
    from oracle.binding import Oracle
    c = case(S.TEXTURE_FORMAT_RGBA8_UNORM)
    o = Oracle(c.scene(dummy_luts()))
    uv = c.uv[4][:16]
    for tex in (0, FIRST_TEXTURE + len(SIZES), 0xFFFFFFFF):
        assert not o.sample_texture(tex, 1, uv).any() and not o.sample_texture_grad(tex, 1, uv, uv, uv).any()
    assert o.sample_texture(FIRST_TEXTURE + 4, 1, uv).any()
    o.close()
