"""wf_bounce0: bounce 0 of the config-2 class of scenes traced and shaded in one kernel (HRPT_WF_FUSED_BOUNCE0, default 1) against the
wf_extend<PRIMARY> + wf_shade_lt<PRIMARY> pair it replaces (knob 0). The same rays, the same shading body, fed from registers instead of the hit and
{direction, seed} records: Accumulation, Output and every ray / path / NEE counter must be bit-identical between the two, and equal to the oracle's.

Small frames on purpose: 40 x 24 is 15 whole 8 x 8 tiles, 37 x 19 leaves padding pixels in the last tile column and row (slots without a path);
with one bounce the fused kernel is also the last bounce (no survivors, no specular ring traffic), with four it feeds the ordinary kernels.
The knob is read at hrpt_create, so every render runs on a context of its own."""
import copy

import numpy as np
import pytest

from hobbyrenderer_amd import scenes, structs as S
from test_parity_gpu import _assert_parity
from test_shade_lds_tables_gpu import _frame, _oracle

pytestmark = pytest.mark.gpu

COUNTERS = ("closestRays", "shadowRays", "paths", "neeEntries", "neeSamples")


def _render(monkeypatch, knob, sc, view, pos, w, h, spp, bounces, tiles=(((0, 0, 0, 0), (1, 0)),)):
    """(accumulation, output, counters, stats) of the frame under HRPT_WF_FUSED_BOUNCE0=knob."""
    from hobbyrenderer_amd.native import PathTracerContext
    monkeypatch.setenv("HRPT_WF_FUSED_BOUNCE0", str(knob))
    c = PathTracerContext(0)
    try:
        c.upload_scene(sc)
        acc, out, _ = _frame(c, sc, view, pos, w=w, h=h, spp=spp, bounces=bounces, tiles=tiles)
        st = c.stats()
    finally:
        c.close()
    return acc, out, tuple(getattr(st, f) for f in COUNTERS), st


def _on_off(monkeypatch, sc, view, pos, w, h, spp, bounces, chosen=True, **kw):
    """The frame under knob 1 after it was found bit-identical, counters included, to the frame under knob 0. `chosen`: whether the plan takes
    the fused kernel for this scene -- then, and only then, bounce 0 moves no hit and no path record through the trace stage's queues."""
    on, off = (_render(monkeypatch, knob, sc, view, pos, w, h, spp, bounces, **kw) for knob in (1, 0))
    assert on[2] == off[2], (on[2], off[2])
    assert np.array_equal(on[0].view(np.uint32), off[0].view(np.uint32)) and np.array_equal(on[1].view(np.uint32), off[1].view(np.uint32))
    assert on[3].megakernelFallbacks == 0 and off[3].megakernelFallbacks == 0
    if chosen:
        assert on[3].traceQueueBytes == off[3].traceQueueBytes - 32 * on[3].paths, (on[3].traceQueueBytes, off[3].traceQueueBytes, on[3].paths)
        assert on[3].shadeQueueBytes < off[3].shadeQueueBytes
    else:
        assert (on[3].traceQueueBytes, on[3].shadeQueueBytes) == (off[3].traceQueueBytes, off[3].shadeQueueBytes)
    return on


@pytest.mark.parametrize("bounces", [1, 4], ids=["last-bounce", "four-bounces"])
@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("size", [(40, 24), (37, 19)], ids=["whole-tiles", "padded-tiles"])
def test_knob_on_off_and_oracle(luts, monkeypatch, size, spp, bounces):
    w, h = size
    sc, view, pos, _ = scenes.config_cornell(luts, w, h)
    acc, out, _, st = _on_off(monkeypatch, sc, view, pos, w, h, spp, bounces)
    assert st.paths == w * h * spp and st.neeEntries > 0
    _assert_parity(acc, out, st, *_oracle(sc, view, pos, w=w, h=h, spp=spp, bounces=bounces))


@pytest.mark.parametrize("size", [(40, 24), (37, 19)], ids=["whole-tiles", "padded-tiles"])
def test_unaligned_rectangle_and_interleaved_columns(luts, monkeypatch, size):
    w, h = size
    sc, view, pos, _ = scenes.config_cornell(luts, w, h)
    rect = (5, 3, w - 6, h - 2)                   # neither corner on the 8-pixel grid
    acc, _, _, _ = _on_off(monkeypatch, sc, view, pos, w, h, 3, 4, tiles=((rect, (1, 0)),))
    oacc, _, _ = _oracle(sc, view, pos, w=w, h=h, spp=3, bounces=4, tile=rect)
    x0, y0, x1, y1 = rect
    assert np.array_equal(acc[y0:y1, x0:x1].view(np.uint32), oacc[y0:y1, x0:x1].view(np.uint32))
    # the odd 8-pixel columns alone (stripes = (2, 1)), then both sets: the whole rectangle, as the oracle renders it in one piece
    odd, _, _, _ = _on_off(monkeypatch, sc, view, pos, w, h, 3, 4, tiles=((rect, (2, 1)),))
    cols = np.array([x for x in range(x0, x1) if ((x - x0) // 8) % 2 == 1])
    assert np.array_equal(odd[y0:y1, cols].view(np.uint32), oacc[y0:y1, cols].view(np.uint32))
    both, _, _, _ = _on_off(monkeypatch, sc, view, pos, w, h, 3, 4, tiles=((rect, (2, 0)), (rect, (2, 1))))
    assert np.array_equal(both[y0:y1, x0:x1].view(np.uint32), oacc[y0:y1, x0:x1].view(np.uint32))


def test_scene_with_a_mask_material_keeps_the_pair(luts, monkeypatch):
    """One alpha-tested material makes its instances ForceNonOpaque: the closest-hit kernel needs the candidate rules the fused kernel compiles
    out, so the plan does not choose it and the knob changes nothing, queue bytes included."""
    w, h = 40, 24
    sc, view, pos, _ = scenes.config_cornell(luts, w, h)
    sc = copy.copy(sc)
    mats = sc.materials.copy()
    mats["m_AlphaMode"][1] = S.ALPHA_MODE_MASK
    sc.materials = mats
    acc, out, _, st = _on_off(monkeypatch, sc, view, pos, w, h, 3, 4, chosen=False)
    _assert_parity(acc, out, st, *_oracle(sc, view, pos, w=w, h=h, spp=3, bounces=4))
