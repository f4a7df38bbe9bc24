"""The post-chain kernels (post_histogram, post_adaptation, post_tonemap through hrpt_post_process_device / hrpt_post_process) against both
references, on the cases of tests/post_cases.py: the CPU oracle bit for bit, and the float64 statement of tests/post_reference.py within
the bounds fixed on the CPU (tests/test_post_reference_cpu.py). The two are asserted separately, so a failure says which relation broke.
No scene: a context, torch tensors and the post-chain entry points."""
import numpy as np
import pytest

from hobbyrenderer_amd import native
import post_cases as PC
import post_reference as R
from test_post_reference_cpu import MODES, bits, bounds_of, check_against_statement, ebits, oracle_sequence, oracle_single

pytestmark = pytest.mark.gpu
f32 = np.float32


def device_pass(ctx, img, p):
    """One hrpt_post_process_device over a copy of `img` on the current torch stream. The display tensor is one pixel longer than the image
    and starts as NaN: returns (display of the image's shape, the extra pixel, exposure, histogram)."""
    import torch
    n = img.shape[0] * img.shape[1]
    hdr = torch.from_numpy(np.array(img, f32)).to("cuda:0")                 # a copy: the cases are read-only
    display = torch.full((n + 1, 4), float("nan"), device="cuda:0")
    stream = torch.cuda.current_stream()
    ctx.post_process_device(hdr.data_ptr(), display.data_ptr(), n, p, stream.cuda_stream)
    stream.synchronize()
    e, hist = ctx.exposure()
    out = display.cpu().numpy()
    return out[:n].reshape(img.shape), out[n], f32(e), hist


def assert_equals_oracle(run, disp, e, hist, what):
    assert ebits(e) == ebits(run["e"]), f"{what}: exposure {e!r} != oracle {run['e']!r}"
    assert np.array_equal(hist, run["hist"]), f"{what}: histogram differs from the oracle in bins {np.flatnonzero(hist != run['hist'])[:8]}"
    diff = np.flatnonzero((bits(disp) != bits(run["disp"])).reshape(-1, 4).any(-1))
    assert diff.size == 0, f"{what}: {diff.size} display pixels differ from the oracle as bits, first {diff[:8]}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(PC.SINGLE))
def test_device_single_frame(name, mode):
    run = oracle_single(name, mode)
    sure, maybe, exact = bounds_of(name)
    ctx = native.PathTracerContext(0)
    try:
        disp, extra, e, hist = device_pass(ctx, run["img"], run["params"])
    finally:
        ctx.close()
    what = f"device {name} {mode}"
    assert np.isnan(extra).all(), f"{what}: the pixel after the last one was written"
    if name == "stride":                                                     # named on their own: a lost tail or head
        for part, sl in (("last", slice(-773, None)), ("first", slice(0, 773))):
            assert np.array_equal(bits(disp[0, sl]), bits(run["disp"][0, sl])), f"{what}: the {part} 773 display pixels differ from the oracle"
    assert_equals_oracle(run, disp, e, hist, what)
    check_against_statement(run, disp, e, hist, sure, maybe, what)
    if name == "ladder":
        assert np.array_equal(hist, exact)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(PC.SEQUENCES))
def test_device_sequence(name, mode):
    runs = oracle_sequence(name, mode)
    ctx = native.PathTracerContext(0)
    try:
        if name == "manual":                                                 # a histogram to be zeroed
            _, _, _, hist = device_pass(ctx, PC.random(), PC.params(mode))
            assert hist.sum() == 61 * 37
        got = [device_pass(ctx, run["img"], run["params"]) for run in runs]
    finally:
        ctx.close()
    for i, (run, (disp, extra, e, hist)) in enumerate(zip(runs, got)):
        what = f"device {name}[{i}] {mode}"
        assert np.isnan(extra).all(), f"{what}: the pixel after the last one was written"
        assert_equals_oracle(run, disp, e, hist, what)
        sure, maybe, _ = R.histogram_bounds(run["img"])
        check_against_statement(run, disp, e, hist, sure, maybe, what)
        if name == "dt0":
            assert ebits(e) == ebits(1.0), f"{what}: dt = 0 moved the exposure"
        if name == "manual":
            assert not hist.any() and ebits(e) == ebits(0.37)


def test_context_path_equals_device_path():
    """hrpt_post_process over Output at 61 x 37 == hrpt_post_process_device over the same pixels, as bits. Output is filled without a
    render: the `random` case written as the accumulation image (alpha 1) and resolved."""
    import torch
    p = PC.params("sdr", dt=0.033)
    a = native.PathTracerContext(0)
    b = native.PathTracerContext(0)
    try:
        a.resize(61, 37)
        a.write_accumulation(np.array(PC.random()))
        a.resolve_output()
        out = a.read_output()
        assert np.array_equal(bits(out[..., :3]), bits(PC.random()[..., :3]))
        for _ in range(2):                                                   # twice: the second pass adapts from the first one's exposure
            a.post_process(p)
        disp_a, (e_a, h_a) = a.read_display(), a.exposure()
        hdr = torch.from_numpy(out).to("cuda:0")
        display = torch.full((37, 61, 4), float("nan"), device="cuda:0")
        stream = torch.cuda.current_stream()
        for _ in range(2):
            b.post_process_device(hdr.data_ptr(), display.data_ptr(), 61 * 37, p, stream.cuda_stream)
        stream.synchronize()
        e_b, h_b = b.exposure()
        assert np.array_equal(bits(disp_a), bits(display.cpu().numpy()))
        assert ebits(e_a) == ebits(e_b) and e_a != 1.0 and np.array_equal(h_a, h_b) and h_a.sum() == 61 * 37
    finally:
        a.close(); b.close()


def test_set_exposure_on_a_fresh_context():
    """hrpt_set_exposure before any post pass allocates the histogram: it must be zero, not whatever the allocation held. A fresh allocation
    may happen to be zero, so this could pass without the initialisation in post_buffers; the initialisation is required regardless."""
    ctx = native.PathTracerContext(0)
    try:
        ctx.set_exposure(0.5)
        e, hist = ctx.exposure()
        assert e == 0.5 and hist.shape == (256,) and not hist.any()
    finally:
        ctx.close()


def test_pixel_count_outside_the_range_is_refused_before_any_launch():
    import torch
    ctx = native.PathTracerContext(0)
    try:
        hdr = torch.ones((4, 4), device="cuda:0")
        display = torch.full((4, 4), float("nan"), device="cuda:0")
        p = PC.params("sdr")
        ctx.set_exposure(0.25)
        for count in (0, 2 ** 32, 2 ** 32 + 4, 2 ** 63):
            with pytest.raises(native.HrptError) as err:
                ctx.post_process_device(hdr.data_ptr(), display.data_ptr(), count, p)
            assert "pixelCount must be 1..2^32-1" in str(err.value)
        torch.cuda.synchronize()
        assert torch.isnan(display).all().item() and ctx.exposure()[0] == 0.25
    finally:
        ctx.close()
