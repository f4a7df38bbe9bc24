"""The device against the float64 reference of hit attributes, normal maps and sampled-alpha masks (tests/surface_reference.py, DESIGN.md
section 31), with the bars, DELTA and the 5 % cap that tests/test_surface_reference_cpu.py settled against the CPU oracle; nothing is
adjusted here.

* hrpt_render_gbuffer of cases F, G and H at 48 x 27 per camera on the wavefront and the megakernel paths, H over the two-level structure,
  F also with quantised nodes of format 1: ids and flags exactly and the five float planes to TAU_ATTR (TAU_ATTR_FAR on the island) on
  every pixel whose decision margin reaches DELTA.
* hrpt_trace_radiance on the camera and probe rays of F, G and H through both kernels, hrpt_render of F and G at two accumulation indices,
  and G under both shadow schedules for scenes with non-opaque geometry, per path against the replay to TAU_SURFACE.
* The exact probes (alpha == cutoff commits, the next cutoff above does not) through hrpt_trace_rays' closest-hit and shadow queries."""
import numpy as np
import pytest

from hobbyrenderer_amd import structs as S
import path_cases as PC
import path_reference as R
import surface_cases as SC
import surface_reference as SR

pytestmark = pytest.mark.gpu
PLANES = ["albedo", "normal", "geo_normal", "emissive", "depth"]
KERNELS = [("wavefront", S.FRAME_WAVEFRONT), ("megakernel", S.FRAME_MEGAKERNEL)]
_CACHE = {}


def _context(scene, structure=None):
    from hobbyrenderer_amd.native import PathTracerContext
    ctx = PathTracerContext(0)
    try:
        if structure is not None:
            ctx.set_acceleration_structure(structure)
        ctx.upload_scene(scene)
    except Exception:
        ctx.close()
        raise
    return ctx


# ---------------------------------------------------------------- the first hit
def _check_first_hit(case, flags, what):
    ref = SC.first_hit_reference(case)
    ctx = _context(case.scene, case.structure)
    try:
        if case.structure is not None:
            assert ctx.build_info().structure == case.structure
        ctx.resize(SC.GW, SC.GH)
        got = []
        for _, cb, w, h, *_ in ref:
            ctx.render_gbuffer(cb, flags=flags)
            got.append([ctx.read_gbuffer(k) for k in range(S.GB_PLANES)])
    finally:
        ctx.close()
    for k, ((label, cb, w, h, planes, margin, info), g) in enumerate(zip(ref, got)):
        inc = margin >= R.DELTA
        bar = SR.TAU_ATTR_FAR if k in case.far_views else SR.TAU_ATTR
        same = (g[S.GB_IDS].reshape(-1, 4).astype(np.int64) == planes[S.GB_IDS]).all(1)
        err = {PLANES[p]: SR.plane_error(g[p], planes[p]) for p in range(5)}
        print(f"{what}, {label}: {int((~inc).sum())} of {len(inc)} pixels left out, ids differ on {int((~same).sum())}, worst included error "
              + ", ".join(f"{p} {np.where(inc, e, 0.0).max():.3e}" for p, e in err.items()) + f", bar {bar:.3e}")
        assert (~inc).mean() <= R.MAX_EXCLUDED_SHARE
        assert (same | ~inc).all(), f"{what}, {label}: ids, hit or front-face flags differ at pixel {int(np.argmax(~same & inc))}"
        for p, e in err.items():
            assert np.where(inc, e, 0.0).max() <= bar, f"{what}, {label}, {p}: pixel {int(np.argmax(np.where(inc, e, 0.0)))}"


@pytest.mark.parametrize("label,flags", KERNELS)
@pytest.mark.parametrize("name", SC.NAMES)
def test_gbuffer_equals_the_reference(luts, name, label, flags):
    _check_first_hit(SC.case(name, luts), flags, f"case {name}, {label}")


def test_gbuffer_over_quantised_nodes_equals_the_reference(luts, monkeypatch):
    monkeypatch.setenv("HRPT_BVH_NODE_FORMAT", "1")
    _check_first_hit(SC.case("F", luts), S.FRAME_WAVEFRONT, "case F, HRPT_BVH_NODE_FORMAT=1")


# ---------------------------------------------------------------- paths
def _batch_reference(luts, name):
    if name not in _CACHE:
        case = SC.case(name, luts)
        rays, cb = case.batch(), case.constants()
        _CACHE[name] = (case, rays, cb, R.trace_paths(R.PathScene(case.scene), cb, rays))
    return _CACHE[name]


def _camera_reference(luts, name):
    """[(cb, replay)] of the first camera at both indices."""
    key = ("camera", name)
    if key not in _CACHE:
        case = SC.case(name, luts)
        ps = R.PathScene(case.scene)
        _CACHE[key] = [(cb, R.trace_paths(ps, cb, PC.rays_of(cb, w, h))) for _, cb, w, h in case.views()[:2]]
    return _CACHE[key]


def _compare(got, paths, what):
    got = np.asarray(got)
    assert np.isfinite(got).all() and (got[:, 3] == 1.0).all(), what
    err = R.path_error(got, paths)
    inc = paths.included()
    share = 1.0 - inc.mean()
    worst = int(np.argmax(np.where(inc, err, -1.0)))
    print(f"{what}: {len(err)} paths, {100 * share:.2f} % left out, worst included error {err[worst]:.3e} (path {worst}), "
          f"beyond 1e-2 among the left out: {int((~inc & (err > 1e-2)).sum())}")
    assert share <= R.MAX_EXCLUDED_SHARE, what
    assert err[worst] <= R.TAU_SURFACE, (f"{what}: path {worst} {got[worst, :3]} against {paths.radiance[worst]}, margin {paths.margin[worst]:.3e}, "
                                         f"{int((inc & (err > R.TAU_SURFACE)).sum())} paths beyond tau, took {[b for b in paths.took if paths.took[b][worst]]}")


@pytest.mark.parametrize("thread_per_ray", [False, True], ids=["wavefront", "thread-per-ray"])
@pytest.mark.parametrize("name", SC.NAMES)
def test_trace_radiance_equals_the_replay(luts, name, thread_per_ray):
    case, rays, cb, paths = _batch_reference(luts, name)
    ctx = _context(case.scene, case.structure)
    try:
        got = ctx.trace_radiance(rays, cb, thread_per_ray=thread_per_ray)
    finally:
        ctx.close()
    _compare(got, paths, f"case {name}, hrpt_trace_radiance")


def _render_and_compare(luts, name, what):
    case = SC.case(name, luts)
    ctx = _context(case.scene, case.structure)
    try:
        ctx.resize(PC.W, PC.H)
        for cb, paths in _camera_reference(luts, name):
            ctx.clear_accumulation()
            ctx.render(cb)
            _compare(ctx.read_accumulation().reshape(-1, 4), paths, f"{what}, hrpt_render of index {int(cb['m_AccumulationIndex'])}")
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["F", "G"])
def test_render_equals_the_replay(luts, name):
    _render_and_compare(luts, name, f"case {name}")


@pytest.mark.parametrize("schedule", [1, 2])
def test_both_shadow_schedules_equal_the_replay(luts, monkeypatch, schedule):
    """Scenes with non-opaque geometry take wf_shadow's own buffered query (1) or ray generation + any-hit pass + resolve (2)."""
    monkeypatch.setenv("HRPT_WF_SHADOW_PATH", str(schedule))
    _render_and_compare(luts, "G", f"case G, HRPT_WF_SHADOW_PATH={schedule}")


# ---------------------------------------------------------------- exact probes
@pytest.mark.parametrize("thread_per_ray", [False, True], ids=["persistent", "thread-per-ray"])
def test_exact_probes(luts, thread_per_ray):
    scene = SC.probe_scene(luts)
    rays, commits = SC.probe_rays()
    srays, _ = SC.probe_shadow_rays()
    masked = np.nonzero(scene.materials["m_AlphaMode"][scene.instances["m_MaterialIndex"]] == S.ALPHA_MODE_MASK)[0]
    ctx = _context(scene)
    try:
        closest = ctx.trace_rays(rays, thread_per_ray=thread_per_ray)
        shadow = ctx.trace_rays(srays, shadow=True, thread_per_ray=thread_per_ray)
    finally:
        ctx.close()
    assert (closest["hit"] != 0).all()                                     # the quad or the floor below it
    assert np.array_equal(np.isin(closest["instance"], masked), commits)
    assert np.array_equal(shadow["t"], np.where(commits, 0.0, 1.0).astype(np.float32))
