"""Texture sampling of the device code pinned off the render path (GPU part): hrpt_selftest_sample_textures runs sample_texture,
pbr_textures_batched and sample_texture_grad of csrc/pt_surface.h and csrc/pt_texture.h as they are, one thread per probe, over an uploaded scene's own texture
and material tables (so the upload's level offsets, sizes and formats are under test too). The probes, the float64 reference and the
tolerances are those of tests/test_texture_sampling.py / tests/texture_reference.py:

* probe == oracle bit for bit (one-by-one and gradient results, the whole format x sampler x size matrix, plus generic random gradients,
  which are compared device against oracle only: a float64 level of detail would switch levels at slightly different places);
* batched == one-by-one bit for bit wherever the batched fetch accepts the material, and it must accept exactly the all-8-bit ones;
* probe against the float64 reference directly, the comparison that does not go through the oracle;
* a "sampler chart" scene for what the probe does not reach: the wavefront shade kernel with its LDS material tables and the any-hit
  alpha passes, under both frame paths."""
import numpy as np
import pytest

import test_texture_sampling as T
from hobbyrenderer_amd import scenes, structs as S

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    from hobbyrenderer_amd.native import PathTracerContext
    c = PathTracerContext(0)
    yield c
    c.close()


def _probes(material, uv, ddx=None, ddy=None, flags=S.TEXFLAG_ALBEDO):
    p = np.zeros(len(uv), S.TextureProbe)
    p["material"], p["uv"], p["texFlags"] = material, uv, flags
    if ddx is not None:
        p["ddx"], p["ddy"] = ddx, ddy
    return p


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_probe_argument_errors(luts):
    from hobbyrenderer_amd.native import PathTracerContext, lib
    c = PathTracerContext(0)
    try:
        p, r = np.zeros(2, S.TextureProbe), np.zeros(2, S.TextureProbeResult)
        assert lib.hrpt_selftest_sample_textures(c._h, p.ctypes.data, r.ctypes.data, 2) == -4        # no scene
        assert lib.hrpt_selftest_sample_textures(None, p.ctypes.data, r.ctypes.data, 2) == -1
        c.upload_scene(T.case(S.TEXTURE_FORMAT_RGBA8_UNORM).scene(luts))
        assert lib.hrpt_selftest_sample_textures(c._h, None, r.ctypes.data, 2) == -1
        assert lib.hrpt_selftest_sample_textures(c._h, p.ctypes.data, None, 2) == -1
        assert lib.hrpt_selftest_sample_textures(c._h, None, None, 0) == 0                           # nothing to do
        p["material"] = 1 << 20
        assert lib.hrpt_selftest_sample_textures(c._h, p.ctypes.data, r.ctypes.data, 2) == -1        # no such material
        assert len(c.selftest_sample_textures(np.zeros(0, S.TextureProbe))) == 0
    finally:
        c.close()


@pytest.mark.parametrize("fmt", T.FORMATS, ids=T.FORMAT_IDS)
def test_probe_equals_the_oracle_and_the_reference(ctx, luts, fmt):
    c = T.case(fmt)
    ctx.upload_scene(c.scene(luts))
    eight = fmt in (S.TEXTURE_FORMAT_RGBA8_UNORM, S.TEXTURE_FORMAT_RGBA8_SRGB)
    parts, spans, at = [], {}, 0
    for ti in range(len(T.SIZES)):
        guv, ddx, ddy, _ = c.grad[ti]
        for si in range(len(T.SAMPLERS)):
            a, b = _probes(c.material(ti, si), c.uv[ti]), _probes(c.material(ti, si), guv, ddx, ddy)
            parts += [a, b]
            spans[ti, si] = (at, at + len(a), at + len(a) + len(b))
            at += len(a) + len(b)
    res = ctx.selftest_sample_textures(np.concatenate(parts))
    got = {}
    for key, (i0, i1, i2) in spans.items():
        got[key] = (res["single"][i0:i1, 0], res["grad"][i1:i2])
        olvl0, ograd = c.oracle[key]
        where = (T.SIZES[key[0]], T.SAMPLERS[key[1]])
        assert np.array_equal(_bits(got[key][0]), _bits(olvl0)), f"one-by-one sampling differs from the oracle, {where}"
        assert np.array_equal(_bits(got[key][1]), _bits(ograd)), f"gradient sampling differs from the oracle, {where}"
        # a level-0 probe carries zero gradients: its gradient result is the level-0 sample again, and so is a gradient probe's one-by-one result
        assert np.array_equal(_bits(res["grad"][i0:i1]), _bits(olvl0))
        r = res[i0:i2]
        assert not r["single"][:, 1:].any() and not r["batched"][:, 1:].any(), "an unflagged slot sampled something"
        if eight:
            assert (r["batchedAccepted"] == 1).all(), f"the batched fetch declined an all-8-bit material, {where}"
            assert np.array_equal(_bits(r["batched"][:, 0]), _bits(r["single"][:, 0])), f"batched differs from one-by-one, {where}"
        else:
            assert (r["batchedAccepted"] == 0).all() and not r["batched"].any(), f"the batched fetch took a float texture, {where}"
    T.assert_exact_texels(c, got, "device")
    T.assert_within_tolerance(c, got, "device")
    T.assert_sensitivity(c, got, "device")


@pytest.mark.parametrize("fmt", T.FORMATS, ids=T.FORMAT_IDS)
def test_generic_random_gradients_equal_the_oracle(ctx, luts, fmt):
    """Random uv, random ddx and ddy of random magnitude (2^-9 .. 2^3 of the texture, so every level and both clamps): device == oracle bit
    for bit. No reference here: its float64 level of detail would switch levels at slightly different places than the fp32 one."""
    from oracle.binding import Oracle, lib
    c = T.case(fmt)
    sc = c.scene(luts)
    ctx.upload_scene(sc)
    o = Oracle(sc)
    rng = np.random.default_rng(5)
    n = 160
    try:
        for ti, (w, h, mips) in enumerate(T.SIZES):
            uv = rng.uniform(-T.UV_RANGE, T.UV_RANGE, (n, 2)).astype(F32)
            ddx, ddy = ((rng.normal(size=(n, 2)) * np.exp2(rng.uniform(-9, 3, (n, 1)))).astype(F32) for _ in range(2))
            for si, s in enumerate(T.SAMPLERS):
                got = ctx.selftest_sample_textures(_probes(c.material(ti, si), uv, ddx, ddy))["grad"]
                want = o.sample_texture_grad(T.FIRST_TEXTURE + ti, s, uv, ddx, ddy)
                assert np.array_equal(_bits(got), _bits(want)), (T.SIZES[ti], s)
            lod = np.clip(T.contract_lod(ddx, ddy, w, h, lib().or_log2), 0, mips - 1)
            assert set(np.floor(lod).astype(int)) == set(range(mips)), "the random gradients do not reach every level"
    finally:
        o.close()


def _mixed_case():
    """One scene with 8-bit and float textures and materials that combine them over the four slots."""
    rng = np.random.default_rng(31)
    sizes = [(5, 3, 1), (16, 16, 5), (33, 17, 6), (1, 7, 1)]
    textures = [T.random_texture(rng, w, h, fmt, mips) for fmt in T.FORMATS for w, h, mips in sizes]
    count = T.FIRST_TEXTURE + len(textures)
    eight = list(range(T.FIRST_TEXTURE, T.FIRST_TEXTURE + 8))
    half, full = list(range(T.FIRST_TEXTURE + 8, T.FIRST_TEXTURE + 12)), list(range(T.FIRST_TEXTURE + 12, count))
    A, N, RM, E = S.TEXFLAG_ALBEDO, S.TEXFLAG_NORMAL, S.TEXFLAG_ROUGHNESS_METALLIC, S.TEXFLAG_EMISSIVE
    mats = []          # (flags, [texture of albedo, roughness-metallic, emissive, normal], [sampler ...])

    def pick(pool):
        return int(rng.choice(pool))
    for flags in list(range(1, 16)) * 2:                            # every mask of one to four flagged slots, all 8-bit, twice
        mats.append((flags, [pick(eight) for _ in range(4)], [pick(T.SAMPLERS) for _ in range(4)]))
    for bad in (count, count + 5, 0xFFFFFFFF, 3):                   # a flagged slot that names no texture (3: an unbound default slot)
        for slot in range(4):
            tex = [pick(eight) for _ in range(4)]
            tex[slot] = bad
            mats.append((15, tex, [pick(T.SAMPLERS) for _ in range(4)]))
    mats.append((A | E, [eight[0], eight[1], half[0], eight[2]], [1, 0, 4, 5]))            # 8-bit with RGBA16F: declined
    mats.append((A | N, [full[1], eight[1], eight[2], eight[3]], [5, 0, 4, 3]))            # RGBA32F with 8-bit: declined
    mats.append((15, [eight[4], half[2], full[2], eight[6]], [2, 3, 7, 1]))                # all three kinds: declined
    mats.append((A | RM, [half[1], full[0], eight[0], eight[1]], [1, 5, 0, 0]))            # float only: declined
    mats.append((A | N, [eight[5], half[0], full[3], eight[7]], [1, 2, 3, 4]))             # float textures in UNFLAGGED slots: accepted
    mats.append((E, [count, eight[3], half[3], 3], [1, 1, 5, 1]))                          # only float flagged, others name nothing: declined
    materials = [dict(m_TextureFlags=f, m_AlbedoTextureIndex=t[0], m_RoughnessMetallicTextureIndex=t[1], m_EmissiveTextureIndex=t[2],
                      m_NormalTextureIndex=t[3], m_AlbedoSamplerIndex=s[0], m_RoughnessSamplerIndex=s[1], m_EmissiveSamplerIndex=s[2],
                      m_NormalSamplerIndex=s[3]) for f, t, s in mats]

    def is_8bit(t):
        return T.FIRST_TEXTURE <= t < T.FIRST_TEXTURE + 8

    def bound(t):
        return T.FIRST_TEXTURE <= t < count
    accepted = [all(is_8bit(t) or not bound(t) for k, t in enumerate(tex) if f & S.TEXTURE_PROBE_SLOT_FLAGS[k]) for f, tex, _ in mats]
    return textures, mats, materials, accepted


def test_batched_fetch_equals_one_by_one_on_mixed_materials(ctx, luts):
    """Materials with one to four flagged slots, another texture, size and sampler per slot, slots that name no texture (zeros), and
    materials that mix 8-bit with float textures (the batched fetch must decline those and only those)."""
    from oracle.binding import Oracle
    textures, mats, materials, accepted = _mixed_case()
    sc = T.probe_scene(luts, textures, materials)
    ctx.upload_scene(sc)
    rng = np.random.default_rng(8)
    uv = np.concatenate([rng.uniform(-T.UV_RANGE, T.UV_RANGE, (300, 2)), rng.integers(-3 * 33, 3 * 33, (100, 2)) / 33.0 + (0.5 / 33.0),
                         rng.integers(-6, 7, (40, 2)) * 0.5]).astype(F32)
    res = ctx.selftest_sample_textures(np.concatenate([_probes(1 + mi, uv, flags=f) for mi, (f, _, _) in enumerate(mats)]))
    o = Oracle(sc)
    try:
        assert sum(accepted) >= 46 and len(accepted) - sum(accepted) == 5
        for mi, (flags, tex, smp) in enumerate(mats):
            r = res[mi * len(uv):(mi + 1) * len(uv)]
            for k in range(4):
                want = o.sample_texture(tex[k], smp[k], uv) if flags & S.TEXTURE_PROBE_SLOT_FLAGS[k] else np.zeros((len(uv), 4), F32)
                assert np.array_equal(_bits(r["single"][:, k]), _bits(want)), (mi, k)
                if flags & S.TEXTURE_PROBE_SLOT_FLAGS[k] and T.FIRST_TEXTURE <= tex[k] < T.FIRST_TEXTURE + len(textures):
                    assert want.any()
            assert (r["batchedAccepted"] == int(accepted[mi])).all(), f"material {mi} (flags {flags}, textures {tex}): accepted {int(r['batchedAccepted'][0])}"
            if accepted[mi]:
                assert np.array_equal(_bits(r["batched"]), _bits(r["single"])), f"batched differs from one-by-one, material {mi} (flags {flags}, textures {tex}, samplers {smp})"
            else:
                assert not r["batched"].any()
    finally:
        o.close()


CHART_SAMPLERS = [2, 3, 5, 7]
CHART_SIZES = [(5, 3, 1), (32, 4, 6), (33, 17, 6)]
CHART_TWIN = {2: 3, 3: 2, 5: 4, 7: 5}          # the sampler with the other address mode


def _chart_scene(luts, twin=False, chains=True):
    """Camera-facing quads over a floor, one combination of {format} x {sampler 2, 3, 5, 7} x {5x3, 32x4 chain, 33x17 chain} each (every
    format x size pair once, the samplers cycling), vertex uv spanning [-1.5, 2.5], every other quad alpha-tested (MASK) so that the
    floor's shadow rays go through candidate_alpha_grad, and a thirteenth quad whose material mixes an 8-bit albedo with a float emissive
    texture (the batched fetch declines it). Float texels are kept in [0, 1.5] here: the picture has to stay finite."""
    rng = np.random.default_rng(17)
    b = scenes.SceneBuilder()
    floor = b.add_mesh(*scenes.generate_floor_quad())
    pos = [(0.5, -0.5, 0.0), (-0.5, -0.5, 0.0), (-0.5, 0.5, 0.0), (0.5, 0.5, 0.0)]
    quad = b.add_mesh(*scenes._faces_to_mesh([(pos, (0, 0, -1), (-1, 0, 0), 1.0, [(-1.5, 2.5), (2.5, 2.5), (2.5, -1.5), (-1.5, -1.5)])]))
    b.add_instance(floor, b.add_material(m_BaseColor=(0.8, 0.8, 0.8, 1)), scenes._mat(scale=(14, 1, 14), translate=(0, 0, 2)))

    def texture(w, h, mips, fmt):
        t = T.random_texture(rng, w, h, fmt, mips, positive=True)
        return t if chains or mips == 1 else S.Texture(t.level(0).copy(), w, h, fmt, 1)
    for q in range(13):
        fmt, (w, h, mips), smp = T.FORMATS[q % 4], CHART_SIZES[q % 3], CHART_SAMPLERS[(q + q // 4) % 4]
        smp = CHART_TWIN[smp] if twin else smp
        kw = dict(m_TextureFlags=S.TEXFLAG_ALBEDO, m_AlbedoTextureIndex=b.add_texture(texture(w, h, mips, fmt)), m_AlbedoSamplerIndex=smp,
                  m_AlphaMode=S.ALPHA_MODE_MASK if q % 2 else S.ALPHA_MODE_OPAQUE, m_AlphaCutoff=0.5)
        if q == 12:
            kw.update(m_TextureFlags=S.TEXFLAG_ALBEDO | S.TEXFLAG_EMISSIVE, m_EmissiveFactor=(0.5, 0.5, 0.5, 1), m_EmissiveSamplerIndex=smp,
                      m_EmissiveTextureIndex=b.add_texture(texture(5, 3, 1, S.TEXTURE_FORMAT_RGBA16_FLOAT)), m_AlphaMode=S.ALPHA_MODE_MASK)
        col, row = q % 5, q // 5
        b.add_instance(quad, b.add_material(**kw), scenes._mat(scale=(0.45, 0.45, 1), translate=(0.6 * (col - 2) + 0.15 * row, 0.3 + 0.05 * col, 0.8 * row)))
    b.add_light(S.LIGHT_POINT, position=(0.0, 1.3, 3.2), intensity=40.0)        # behind the quads: their shadows fall towards the camera
    return b.finalize(luts)


def _chart_view():
    return scenes.planar_view(64, 48, position=(0.0, 2.0, -2.6), pitch=0.55, aspect=64 / 48)


@pytest.mark.parametrize("flags", [S.FRAME_MEGAKERNEL, S.FRAME_DEFAULT], ids=["megakernel", "default"])
def test_sampler_chart_renders_like_the_oracle(luts, flags):
    """The render path over the same matrix: bit-exact against the oracle, every sampler's address mode matters (its clamp / wrap twin gives
    another image) and so do the mip chains (the gradient-sampled alpha test of the shadow rays)."""
    from test_parity_gpu import _run_both, _assert_parity
    from hobbyrenderer_amd.native import PathTracerContext
    view, pos = _chart_view()
    c = PathTracerContext(0)
    try:
        res = _run_both(c, _chart_scene(luts), view, pos, 64, 48, 2, 3, flags)
        _assert_parity(*res)
        assert res[2].shadowRays > 0 and np.isfinite(res[0]).all()
        twin = _run_both(c, _chart_scene(luts, twin=True), view, pos, 64, 48, 2, 3, flags)
        _assert_parity(*twin)
        assert not np.array_equal(res[0], twin[0]), "clamp and wrap twins of every sampler gave the same image"
        flat = _run_both(c, _chart_scene(luts, chains=False), view, pos, 64, 48, 2, 3, flags)
        _assert_parity(*flat)
        assert not np.array_equal(res[0], flat[0]), "the mip chains did not influence the image: the gradient-sampled alpha test was not exercised"
    finally:
        c.close()
