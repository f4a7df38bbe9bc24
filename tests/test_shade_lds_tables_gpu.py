"""wf_shade_lt: the SIMPLE shade variants with the triangle, instance and material tables in LDS (HRPT_WF_SHADE_LDS_TABLES, default 1) against
the same kernels over the tables in global memory (knob 0). The same records are read, only from another place: Accumulation, Output and the
ray counters must be bit-identical between the two, and equal to the oracle's.

The knob is read at hrpt_create, so every render here runs on a context of its own, created under the knob's value."""
import copy

import numpy as np
import pytest

from hobbyrenderer_amd import scenes
from test_parity_gpu import _assert_parity

pytestmark = pytest.mark.gpu

W, H, SPP, BOUNCES = 96, 54, 3, 4


def _context(monkeypatch, knob, **env):
    from hobbyrenderer_amd.native import PathTracerContext
    monkeypatch.setenv("HRPT_WF_SHADE_LDS_TABLES", str(knob))
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    return PathTracerContext(0)


def _frame(c, sc, view, pos, w=W, h=H, spp=SPP, bounces=BOUNCES, tiles=(((0, 0, 0, 0), (1, 0)),)):
    c.resize(w, h)
    c.reset_stats()
    for tile, stripes in tiles:
        c.render(scenes.fill_constants(view, pos, sc, 0, bounces), accum_count=spp, tile=tile, stripes=stripes)
    st = c.stats()
    return c.read_accumulation(), c.read_output(), (st.closestRays, st.shadowRays, st.paths)


def _oracle(sc, view, pos, w=W, h=H, spp=SPP, bounces=BOUNCES, tile=None):
    from oracle.binding import Oracle, OrStats
    o = Oracle(sc)
    ost = OrStats()
    kw = {} if tile is None else {"tile": tile}
    oacc, oout = o.render_accumulated(lambda i: scenes.fill_constants(view, pos, sc, i, bounces), w, h, spp, stats=ost, **kw)
    o.close()
    return oacc, oout, ost


def _same(a, b):
    assert a[2] == b[2], (a[2], b[2])
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _both_knobs(monkeypatch, sc, view, pos, after_upload=None, now=None, env=None, **frame):
    """The frame of `sc` under knob 1, after it was found bit-identical to the one under knob 0. after_upload(context) runs between the
    upload and the render, `now` is the scene the render then shows (its constants)."""
    frames = []
    for knob in (1, 0):
        c = _context(monkeypatch, knob, **(env or {}))
        try:
            c.upload_scene(sc)
            if after_upload:
                after_upload(c)
            frames.append(_frame(c, now if now is not None else sc, view, pos, **frame))
        finally:
            c.close()
    _same(*frames)
    return frames[0]


@pytest.mark.parametrize("fused", [1, 0], ids=["fused-primary", "raygen"])
def test_config2_scene_knob_on_off_and_oracle(luts, monkeypatch, fused):
    sc, view, pos, _ = scenes.config_cornell(luts, W, H)
    acc, out, _ = _both_knobs(monkeypatch, sc, view, pos, env={"HRPT_WF_FUSED_PRIMARY": fused})
    c = _context(monkeypatch, 1, HRPT_WF_FUSED_PRIMARY=fused)
    try:
        c.upload_scene(sc); c.resize(W, H); c.reset_stats()
        c.render(scenes.fill_constants(view, pos, sc, 0, BOUNCES), accum_count=SPP)
        _assert_parity(c.read_accumulation(), c.read_output(), c.stats(), *_oracle(sc, view, pos))
    finally:
        c.close()


def test_tile_and_interleaved_columns(luts, monkeypatch):
    sc, view, pos, _ = scenes.config_cornell(luts, W, H)
    band = (0, 16, W, 40)
    acc, _, _ = _both_knobs(monkeypatch, sc, view, pos, tiles=((band, (1, 0)),))
    oacc, _, _ = _oracle(sc, view, pos, tile=band)
    assert np.array_equal(acc[16:40].view(np.uint32), oacc[16:40].view(np.uint32))
    # an unaligned rectangle rendered as two sets of interleaved 8-pixel columns: the whole rectangle, as the oracle renders it in one piece
    rect = (5, 3, 91, 50)
    acc, _, _ = _both_knobs(monkeypatch, sc, view, pos, tiles=((rect, (2, 0)), (rect, (2, 1))))
    oacc, _, _ = _oracle(sc, view, pos, tile=rect)
    assert np.array_equal(acc[3:50, 5:91].view(np.uint32), oacc[3:50, 5:91].view(np.uint32))


def test_material_update_shows(luts, monkeypatch):
    """The LDS copy is made at every launch: new material constants must show in the next render without a new upload."""
    sc, view, pos, _ = scenes.config_cornell(luts, W, H)
    now = copy.copy(sc)
    mats = sc.materials.copy()
    mats["m_BaseColor"][0] = (0.2, 0.3, 0.9, 1.0)                      # the white walls turn blue ...
    mats["m_RoughnessMetallic"][1] = (0.3, 0.8)                      # ... the red one turns into rough metal
    mats["m_EmissiveFactor"][3] = (3.0, 9.0, 14.0, 1.0)                # ... and the lamp changes colour
    now.materials = mats
    before, _, _ = _both_knobs(monkeypatch, sc, view, pos)
    acc, out, _ = _both_knobs(monkeypatch, sc, view, pos, after_upload=lambda c: c.update_materials(mats), now=now)
    assert not np.array_equal(acc, before)
    oacc, oout, _ = _oracle(now, view, pos)
    assert np.array_equal(acc.view(np.uint32), oacc.view(np.uint32)) and np.array_equal(out.view(np.uint32), oout.view(np.uint32))


def test_instance_update_shows(luts, monkeypatch):
    from test_update_instances_gpu import _moved
    sc, view, pos, _ = scenes.config_cornell(luts, W, H)
    n = len(sc.instances)
    now = _moved(sc, n - 3, 2, 1)                                       # the two boxes turn and move: new adjugate rows in GpuInstShade
    before, _, _ = _both_knobs(monkeypatch, sc, view, pos)
    acc, out, _ = _both_knobs(monkeypatch, sc, view, pos, after_upload=lambda c: c.update_instances(now.instances[n - 3:n - 1], n - 3), now=now)
    assert not np.array_equal(acc, before)
    oacc, oout, _ = _oracle(now, view, pos)
    assert np.array_equal(acc.view(np.uint32), oacc.view(np.uint32)) and np.array_equal(out.view(np.uint32), oout.view(np.uint32))


def _quad_field(luts, quads):
    """SIMPLE scene of `quads` one-quad instances (2 triangles each) over 3 materials: its tables take quads * (2 * 80 + 48) + 3 * 180 bytes."""
    b = scenes.SceneBuilder()
    quad = b.add_mesh(*scenes.generate_floor_quad())
    mats = [b.add_material(m_BaseColor=c) for c in ((0.7, 0.7, 0.7, 1), (0.7, 0.2, 0.1, 1), (0.1, 0.3, 0.7, 1))]
    rng = np.random.default_rng(11)
    for i in range(quads):
        x, z = (i % 9) - 4.0, (i // 9) - 1.0
        tilt = rng.uniform(-0.4, 0.4)
        rot = [[np.cos(tilt), np.sin(tilt), 0], [-np.sin(tilt), np.cos(tilt), 0], [0, 0, 1]]
        b.add_instance(quad, mats[i % 3], scenes._mat((0.9, 1, 0.9), rot, (x * 0.5, -0.6 + 0.05 * (i % 4), z * 0.5)))
    return b.finalize(luts)


@pytest.mark.parametrize("quads", [76, 77], ids=["just-under-the-budget", "just-over-the-budget"])
def test_simple_scene_at_the_lds_budget(luts, monkeypatch, quads):
    """pt_wavefront_plan.h: tables + 23 552 B of ring <= 40 KiB - 1 KiB, i.e. at most 16 384 B of tables. 76 quads take 76 * 208 + 540 = 16 348 B
    (LDS), 77 take 16 556 B (global): both sides of the decision give the same bits as knob 0 and as the oracle."""
    assert 76 * 208 + 540 <= 16384 < 77 * 208 + 540
    sc = _quad_field(luts, quads)
    view, pos = scenes.planar_view(W, H, position=(0.0, 2.5, -3.0), pitch=0.9)            # looks down on the field
    acc, out, rays = _both_knobs(monkeypatch, sc, view, pos)
    assert rays[1] > 1000                                                            # shadow rays: surfaces were hit and shaded
    oacc, oout, _ = _oracle(sc, view, pos)
    assert np.array_equal(acc.view(np.uint32), oacc.view(np.uint32)) and np.array_equal(out.view(np.uint32), oout.view(np.uint32))
