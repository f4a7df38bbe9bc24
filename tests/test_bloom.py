"""Bloom in front of the HDR post chain (hrpt_bloom / hrpt_bloom_device / hrpt_bloom_host; csrc/pt_bloom.h, pt_bloom.hip) against
tests/bloom_reference.py, the NumPy float32 restatement of src/shaders/Bloom.hlsl + BloomRenderer::Render. Every comparison is bit
equality of the uint32 views: the contract is + - * / floor min max in a fixed order, which NumPy, the host build and the gfx950
kernels round identically.

CPU: the packed format's known answers, hrpt_bloom_host == NumPy on the sizes that exercise every schedule (full six levels, odd sizes,
fewer levels, none), properties, argument errors, and the kernels' scratch budget from the code object.
GPU: the kernels == NumPy == the host executor, fused tail on and off, a caller-owned device image, the chain bloom -> post_process
against the post chain's oracle, and a resize."""
import ctypes as C
import os

import numpy as np
import pytest

import bloom_reference as ref
import kernel_metadata
from hobbyrenderer_amd import native, scenes, structs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULTS = (0.1, 0.005, 0.85)
OTHER = (0.5, 0.25, 1.5)
INVALID_ARGUMENT = -1                                                # HRPT_ERR_INVALID_ARGUMENT
SIZES = [(160, 90), (131, 77), (64, 64), (40, 24), (1, 5)]          # (width, height): full schedule, odd, smallest full, L < 6, L = 0


def hdr_image(width, height, seed=7, alpha_one=False):
    """Log-uniform radiance 1e-3 .. 1e4 with a few isolated pixels at 6e4 and one above 65504 (SafeHDR and the format's ceiling)."""
    rng = np.random.default_rng(seed + 1000 * width + height)
    img = np.empty((height, width, 4), np.float32)
    img[..., :3] = (10.0 ** rng.uniform(-3.0, 4.0, (height, width, 3))).astype(np.float32)
    img[..., 3] = 1.0 if alpha_one else rng.uniform(0.0, 2.0, (height, width)).astype(np.float32)
    n = width * height
    flat = img.reshape(n, 4)
    for k in range(min(5, n)):
        flat[(k * 7919 + 13) % n, :3] = 6e4
    flat[(n // 2 + 3) % n, :3] = (1.0e5, 7.0e4, 3.0e5)
    return img


def params(p):
    return S.BloomParams(*p)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def _probe1(x):
    """(11-bit word, 10-bit word, unpacked r, unpacked b) of the scalar x through the library."""
    packed, unpacked = native.bloom_pack_probe(np.array([[x, x, x]], np.float32))
    w = int(packed[0])
    assert (w & 0x7FF) == ((w >> 11) & 0x7FF)
    return w & 0x7FF, w >> 22, unpacked[0, 0], unpacked[0, 2]


def test_pack_known_answers():
    inf = float("inf")
    assert _probe1(0.0)[:2] == (0, 0)
    assert _probe1(1.0) == (0x3C0, 0x1E0, 1.0, 1.0)
    assert _probe1(65024.0) == (0x7BF, 0x3DF, 65024.0, 64512.0)           # the largest finite 11-bit value; the 10-bit one is 64512
    assert _probe1(64512.0)[1:] == (0x3DF, 64512.0, 64512.0)
    assert _probe1(1e9) == (0x7BF, 0x3DF, 65024.0, 64512.0)               # too large: the largest finite value, never inf
    assert _probe1(65504.0) == (0x7BF, 0x3DF, 65024.0, 64512.0)
    assert _probe1(inf) == (0x7C0, 0x3E0, inf, inf)
    assert _probe1(-1.0) == (0, 0, 0.0, 0.0) and _probe1(-inf)[:2] == (0, 0) and _probe1(-0.0)[:2] == (0, 0)
    # between 1 and the next 11-bit value 1 + 1/64 (10-bit: 1 + 1/32): rounds DOWN even when nearer to the upper one
    assert _probe1(1.0 + 0.99 / 64.0) == (0x3C0, 0x1E0, 1.0, 1.0)
    assert _probe1(1.0 + 1.5 / 64.0) == (0x3C1, 0x1E0, 1.0 + 1.0 / 64.0, 1.0)
    # denormals are kept: 2^-14 is the smallest normal, below it the mantissa counts units of 2^-20 (11 bit) / 2^-19 (10 bit)
    assert _probe1(2.0 ** -14) == (0x040, 0x020, 2.0 ** -14, 2.0 ** -14)
    assert _probe1(2.0 ** -15) == (0x020, 0x010, 2.0 ** -15, 2.0 ** -15)
    assert _probe1(3.0 * 2.0 ** -20) == (0x003, 0x001, 3.0 * 2.0 ** -20, 2.0 ** -19)
    assert _probe1(2.0 ** -20 * 0.99) == (0, 0, 0.0, 0.0)
    w11, w10, r, b = _probe1(float("nan"))
    assert (w11 >> 6) == 31 and (w11 & 63) and (w10 >> 5) == 31 and (w10 & 31) and np.isnan(r) and np.isnan(b)


def test_pack_equals_numpy_and_rounds_down():
    rng = np.random.default_rng(3)
    x = (10.0 ** rng.uniform(-9.0, 6.0, (100000, 3))).astype(np.float32)
    x[::17] *= -1.0
    packed, unpacked = native.bloom_pack_probe(x)
    assert np.array_equal(packed, ref.pack_r11g11b10(x))
    assert np.array_equal(bits(unpacked), bits(ref.unpack_r11g11b10(packed)))
    pos = x >= 0
    assert (unpacked[pos] <= x[pos]).all() and (unpacked[~pos] == 0).all()
    # every 11-bit and 10-bit pattern survives a round trip
    every = np.arange(2048, dtype=np.uint32)
    vals = np.stack([ref.unpack_channel(every, 6), ref.unpack_channel(every, 6), ref.unpack_channel(every % 1024, 5)], -1)
    finite = ~np.isnan(vals).any(-1)
    again, _ = native.bloom_pack_probe(vals)
    assert np.array_equal(again[finite], (every | (every << 11) | ((every % 1024) << 22))[finite])


@pytest.mark.parametrize("p", [DEFAULTS, OTHER], ids=["defaults", "knee0.5_int0.25_r1.5"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_equals_numpy(size, p):
    img = hdr_image(*size)
    got = native.bloom_host(img, params(p), nthreads=4)
    want = ref.bloom(img, *p)
    assert np.array_equal(bits(got), bits(want))
    if size == (1, 5):
        assert np.array_equal(bits(got), bits(img))                       # no level: unchanged
    else:
        assert (bits(got)[..., :3] != bits(img)[..., :3]).mean() > 0.99    # the comparison discriminates


def test_host_properties():
    img = hdr_image(160, 90)
    out = native.bloom_host(img, params(DEFAULTS), nthreads=1)
    assert np.array_equal(bits(out[..., 3]), bits(img[..., 3]))            # alpha untouched
    assert (out[..., :3] >= img[..., :3]).all()                            # additive, bloom >= 0
    assert np.isfinite(out).all()
    assert np.array_equal(bits(out), bits(native.bloom_host(img, params(DEFAULTS), nthreads=8)))
    for n in (0, -1, 1000):                                                # the clamp: one per hardware thread up to 16; at most 256
        assert np.array_equal(bits(out), bits(native.bloom_host(img, params(DEFAULTS), nthreads=n))), n
    zero = native.bloom_host(img, params((0.1, 0.0, 0.85)), nthreads=2)
    assert np.array_equal(bits(zero), bits(img))                           # intensity 0: every bit as it was
    inplace = img.copy()                                                   # hdrOut may be hdrIn
    assert native.lib.hrpt_bloom_host(inplace.ctypes.data, inplace.ctypes.data, 160, 90, C.byref(params(DEFAULTS)), 3) == 0
    assert np.array_equal(bits(inplace), bits(out))


def test_host_argument_errors():
    img = hdr_image(8, 8)
    out = np.empty_like(img)
    call = native.lib.hrpt_bloom_host
    err = lambda: native.lib.hrpt_last_error(None).decode()          # noqa: E731 -- the whole text, as the library has always worded it
    ok = params(DEFAULTS)
    assert call(img.ctypes.data, out.ctypes.data, 8, 8, C.byref(ok), 1) == 0
    assert call(None, out.ctypes.data, 8, 8, C.byref(ok), 1) == INVALID_ARGUMENT
    assert err() == "hrpt_bloom_host: null image"
    assert call(img.ctypes.data, None, 8, 8, C.byref(ok), 1) == INVALID_ARGUMENT
    assert err() == "hrpt_bloom_host: null image"
    assert call(img.ctypes.data, out.ctypes.data, 8, 8, None, 1) == INVALID_ARGUMENT
    assert err() == "hrpt_bloom_host: null params"
    assert call(img.ctypes.data, out.ctypes.data, 0, 8, C.byref(ok), 1) == INVALID_ARGUMENT
    assert call(img.ctypes.data, out.ctypes.data, 8, 70000, C.byref(ok), 1) == INVALID_ARGUMENT
    for ww, hh in ((0, 8), (8, 0), (0, 0), (65536, 8), (8, 65536), (8, 70000)):
        assert call(img.ctypes.data, out.ctypes.data, ww, hh, C.byref(ok), 1) == INVALID_ARGUMENT and err() == "hrpt_bloom_host: size must be 1..65535", (ww, hh)
    for bad in [(-0.1, 0.005, 0.85), (0.1, -1.0, 0.85), (0.1, 0.005, -0.5), (float("nan"), 0.005, 0.85), (0.1, float("inf"), 0.85),
                (0.1, 0.005, float("nan"))]:
        assert call(img.ctypes.data, out.ctypes.data, 8, 8, C.byref(params(bad)), 1) == INVALID_ARGUMENT, bad
        assert b"hrpt_bloom_host" in native.lib.hrpt_last_error(None)
        assert err() == "hrpt_bloom_host: knee, intensity and upsampleRadius must be finite and >= 0", bad
    with pytest.raises(native.HrptError):
        native.bloom_host(img, params((0.1, -1.0, 0.85)))


def test_bloom_kernels_use_no_scratch():
    """Every kernel of pt_bloom.hip.o has private_segment_fixed_size 0: no spills, no private arrays (the fused tail runs 512 lanes of up
    to 256 VGPRs for exactly this reason)."""
    found = {n: k["scratch"] for n, k in kernel_metadata.kernels("pt_bloom.hip.o").items()}
    for kernel in ("bloom_prefilter", "bloom_downsample", "bloom_upsample", "bloom_composite", "bloom_tail"):
        assert any(kernel in name for name in found), (kernel, sorted(found))
    assert all(v == 0 for v in found.values()), found


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def _gpu_bloom(img, p, fused_tail=None, ctx=None):
    """Output of a context after write_accumulation (alpha 1) + resolve_output + bloom. fused_tail: HRPT_BLOOM_FUSED_TAIL for a fresh
    context (the knob is read by hrpt_create)."""
    own = ctx is None
    if own:
        old = os.environ.get("HRPT_BLOOM_FUSED_TAIL")
        if fused_tail is not None:
            os.environ["HRPT_BLOOM_FUSED_TAIL"] = str(fused_tail)
        try:
            ctx = native.PathTracerContext(0)
        finally:
            if fused_tail is not None:
                if old is None:
                    del os.environ["HRPT_BLOOM_FUSED_TAIL"]
                else:
                    os.environ["HRPT_BLOOM_FUSED_TAIL"] = old
    h, w = img.shape[:2]
    ctx.resize(w, h)
    ctx.write_accumulation(img)
    ctx.resolve_output()
    assert np.array_equal(bits(ctx.read_output()), bits(img))              # alpha 1: the resolve divides by 1
    ctx.bloom(params(p))
    out = ctx.read_output()
    if own:
        ctx.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("p", [DEFAULTS, OTHER], ids=["defaults", "knee0.5_int0.25_r1.5"])
@pytest.mark.parametrize("size", SIZES + [(1920, 1080)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_equals_numpy_and_host(size, p):
    img = hdr_image(*size, alpha_one=True)
    got = _gpu_bloom(img, p)
    assert np.array_equal(bits(got), bits(native.bloom_host(img, params(p))))
    assert np.array_equal(bits(got), bits(ref.bloom(img, *p)))


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1920, 1080), (160, 90), (131, 77), (600, 400), (40, 24)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_fused_tail_on_and_off_give_the_same_bits(size):
    """0: one kernel per pass; 1: the default tail; 2048: a shorter tail (starts one level later at 1080p); 32768: the longest tail the
    LDS holds (600 x 400: levels 1..5 in one workgroup, more than 64 KiB of LDS)."""
    img = hdr_image(*size, alpha_one=True)
    want = native.bloom_host(img, params(OTHER))
    for knob in (0, 1, 2048, 32768):
        assert np.array_equal(bits(_gpu_bloom(img, OTHER, fused_tail=knob)), bits(want)), knob


@pytest.mark.gpu
def test_gpu_bloom_device_on_a_torch_tensor():
    import torch
    img = hdr_image(320, 200, alpha_one=True)
    want = _gpu_bloom(img, OTHER)
    t = torch.from_numpy(img).to("cuda:0")
    ctx = native.PathTracerContext(0)
    stream = torch.cuda.current_stream()
    ctx.bloom_device(t.data_ptr(), 320, 200, params(OTHER), stream.cuda_stream)
    stream.synchronize()
    got = t.cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    with pytest.raises(native.HrptError):
        ctx.bloom_device(0, 320, 200, params(OTHER))
    with pytest.raises(native.HrptError):
        ctx.bloom_device(t.data_ptr(), 0, 200, params(OTHER))
    ctx.close()


@pytest.mark.gpu
def test_gpu_argument_errors():
    ctx = native.PathTracerContext(0)
    with pytest.raises(native.HrptError) as e:
        ctx.bloom(params(DEFAULTS))                                        # before resize
    assert e.value.code == INVALID_ARGUMENT
    ctx.resize(32, 32)
    assert native.lib.hrpt_bloom(ctx._h, None) == INVALID_ARGUMENT
    assert native.lib.hrpt_bloom(None, C.byref(params(DEFAULTS))) == INVALID_ARGUMENT
    for bad in [(-0.1, 0.005, 0.85), (0.1, float("nan"), 0.85), (0.1, 0.005, float("inf"))]:
        with pytest.raises(native.HrptError) as e:
            ctx.bloom(params(bad))
        assert e.value.code == INVALID_ARGUMENT
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("auto", [1, 0], ids=["auto", "manual"])
def test_gpu_chain_render_bloom_post_process(luts, auto):
    """A rendered frame, bloom, then the post chain: display, exposure and histogram equal the post chain's oracle applied to the
    NumPy-bloomed output."""
    from oracle.binding import post_process
    sc, view, pos, cfg = scenes.config_glass(luts, 160, 90, detail=0.3)
    ctx = native.PathTracerContext(0)
    ctx.upload_scene(sc); ctx.resize(160, 90)
    ctx.render(scenes.fill_constants(view, pos, sc, 0, 6), accum_count=4)
    out = ctx.read_output()
    bp = (0.1, 0.25, 0.85)
    ctx.bloom(params(bp))
    bloomed = ctx.read_output()
    want = ref.bloom(out, *bp)
    assert np.array_equal(bits(bloomed), bits(want))
    assert not np.array_equal(bits(bloomed), bits(out))
    pp = S.PostParams(auto, 0.37, 0.033, 5.0, -7.0, 23.0, 0.0, 0, 600.0)
    ctx.post_process(pp)
    disp = ctx.read_display()
    e_gpu, h_gpu = ctx.exposure()
    d_ref, e_ref, h_ref = post_process(want, pp, 1.0)
    assert np.float32(e_gpu) == np.float32(e_ref)
    if auto:
        assert np.array_equal(h_gpu, h_ref)
    assert np.array_equal(bits(disp), bits(d_ref))
    # the next render resolves Output from the accumulation again: bloom has not fed back
    ctx.render(scenes.fill_constants(view, pos, sc, 0, 6), accum_count=4)
    assert np.array_equal(bits(ctx.read_output()), bits(out))
    ctx.close()


@pytest.mark.gpu
def test_gpu_bloom_after_resize():
    ctx = native.PathTracerContext(0)
    for size in [(160, 90), (131, 77), (320, 200), (160, 90), (1, 5)]:
        img = hdr_image(*size, alpha_one=True)
        got = _gpu_bloom(img, DEFAULTS, ctx=ctx)
        assert np.array_equal(bits(got), bits(ref.bloom(img, *DEFAULTS))), size
    ctx.close()
