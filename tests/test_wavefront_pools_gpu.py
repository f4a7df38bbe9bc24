"""The wavefront pipeline's device buffers across calls of different sizes (csrc/pt_wavefront.hip: the render's queue pool, the G-buffer's
own pool, the overflow columns). One context, sized once at 64 x 64, makes the calls of SEQUENCE in order: the G-buffer before any render
(its own pool), a 16 x 8 tile render (a render pool smaller than the G-buffer needs), the G-buffer again, a full-frame render (the render
pool grows), the G-buffer again (now inside the render pool), ray queries, the small tile again. Every image and hit array equals, bit for
bit, what a fresh context of the same size returns for that call alone; HrptStats::queuePoolBytes describes the render pool only: 0 before
the first render, never shrinking afterwards, untouched by G-buffer and ray-query calls. Cornell-class scene, one light, two bounces; no
resize between calls (hrpt_resize re-allocates the images a pending result lives in). Deep trees (the overflow columns) are covered by the
deep-tree case of tests/test_parity_gpu.py."""
import numpy as np
import pytest

from hobbyrenderer_amd import native, scenes, structs as S
import ray_cases

pytestmark = pytest.mark.gpu
W, H = 64, 64
TILE = (0, 0, 16, 8)
RAYS = 1000


def _inputs(luts):
    sc, view, pos, _ = scenes.config_cornell(luts, W, H)
    assert len(sc.lights) == 1
    cb = scenes.fill_constants(view, pos, sc, 0, 2)
    cbg = cb.copy()
    cbg["m_Jitter"] = (0.0, 0.0)
    rng = np.random.default_rng(7)
    origins = rng.uniform((-0.8, 0.2, -0.8), (0.8, 1.8, 0.8), (RAYS, 3))       # inside the box
    closest = ray_cases._rays(origins, ray_cases._unit(rng, RAYS))
    shadow = ray_cases._rays(origins, ray_cases._unit(rng, RAYS), 1e-3, rng.uniform(0.2, 3.0, RAYS))
    return sc, cb, cbg, closest, shadow


def _crop(image, tile):
    x0, y0, x1, y1 = tile
    return image[y0:y1, x0:x1]


def _call(ctx, name, sc_inputs):
    """Makes the call `name` on ctx; the bytes it produced (tile renders: over the tile only)."""
    _, cb, cbg, closest, shadow = sc_inputs
    if name == "gbuffer":
        ctx.render_gbuffer(cbg, planes=S.GB_ALL_PLANES)
        return b"".join(np.ascontiguousarray(ctx.read_gbuffer(p)).tobytes() for p in range(S.GB_PLANES))
    if name == "tile render":
        ctx.render(cb, accum_count=2, tile=TILE)
        return np.ascontiguousarray(_crop(ctx.read_accumulation(), TILE)).tobytes() + np.ascontiguousarray(_crop(ctx.read_output(), TILE)).tobytes()
    if name == "full render":
        ctx.render(cb)
        return ctx.read_accumulation().tobytes() + ctx.read_output().tobytes()
    assert name == "trace rays"
    return ctx.trace_rays(closest).tobytes() + ctx.trace_rays(shadow, shadow=True).tobytes()


SEQUENCE = ("gbuffer", "tile render", "gbuffer", "full render", "gbuffer", "trace rays", "tile render")
LEAVES_RENDER_POOL_ALONE = ("gbuffer", "trace rays")


def _context(sc):
    ctx = native.PathTracerContext(0)
    ctx.upload_scene(sc)
    ctx.resize(W, H)
    return ctx


@pytest.fixture(scope="module")
def inputs(luts):
    return _inputs(luts)


@pytest.fixture(scope="module")
def fresh(inputs):
    """name -> the bytes of that call made alone on a fresh context of the same size."""
    out = {}
    for name in sorted(set(SEQUENCE)):
        ctx = _context(inputs[0])
        try:
            out[name] = _call(ctx, name, inputs)
        finally:
            ctx.close()
    return out


def test_calls_of_different_sizes_on_one_context_give_fresh_bits(inputs, fresh):
    ctx = _context(inputs[0])
    try:
        got, pool = [], []
        for name in SEQUENCE:
            got.append(_call(ctx, name, inputs))
            pool.append(int(ctx.stats().queuePoolBytes))
    finally:
        ctx.close()
    differing = [f"{i + 1} {name}" for i, name in enumerate(SEQUENCE) if got[i] != fresh[name]]
    assert not differing, differing
    print("queuePoolBytes after each call:", pool)
    assert pool[0] == 0                                      # the G-buffer before any render worked in its own pool
    assert all(b > 0 for b in pool[1:]) and all(b >= a for a, b in zip(pool, pool[1:]))
    for i, name in enumerate(SEQUENCE):
        if i and name in LEAVES_RENDER_POOL_ALONE:
            assert pool[i] == pool[i - 1], (i + 1, name)
    assert pool[3] > pool[2]                                 # the full frame needed more than the tile: the render pool grew
    # the calls did something: the images are not empty and some rays hit
    assert all(any(fresh[name]) for name in fresh)
