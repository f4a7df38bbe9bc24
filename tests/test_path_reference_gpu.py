"""The path tracer's kernels against the float64 replay of tests/path_reference.py, per path.

Per case of tests/path_cases.py: hrpt_trace_radiance on the 1 304 camera and probe rays plus 1 061 rays no camera makes, in one call,
through the wavefront pipeline and through the thread-per-ray kernel; hrpt_render of the camera at both indices on a cleared
accumulation (the fused primary / wf_bounce0 forms where the plan picks them); case A over the two-level structure; case C with
HRPT_WF_FUSED_BOUNCE0=0. A path whose decision margin is below DELTA is left out (at most 5 % of a batch); every other path must agree
with the replay to TAU in max_c |L32 - L64| / max(|L64|_inf, 1e-3 * Lmax). DELTA and TAU were measured against the CPU oracle
(tests/test_path_reference_cpu.py) and are imported, never adjusted here. The free rays have had no CPU rehearsal: a disagreement there
is a finding about the product or the reference, to be settled by reading."""
import numpy as np
import pytest

from hobbyrenderer_amd import structs as S
import path_cases as PC
import path_reference as R

pytestmark = pytest.mark.gpu
_CACHE = {}


def _reference(luts, name):
    """(case, rays, cb, replay of the rays) per case, once per session: the batch, then the free rays."""
    if name not in _CACHE:
        case = PC.case(name, luts)
        rays = np.concatenate([case.batch(), case.free_rays()])
        assert len(rays) == 1304 + 1061
        cb = case.constants()
        _CACHE[name] = (case, rays, cb, R.trace_paths(R.PathScene(case.scene), cb, rays))
    return _CACHE[name]


def _camera_reference(luts, name):
    """[(cb, replay of the camera's rays)] at both indices."""
    key = ("camera", name)
    if key not in _CACHE:
        case = PC.case(name, luts)
        ps = R.PathScene(case.scene)
        _CACHE[key] = [(cb, R.trace_paths(ps, cb, PC.rays_of(cb, w, h))) for _, cb, w, h in case.views()[:len(PC.INDICES)]]
    return _CACHE[key]


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
    assert err[worst] <= R.TAU, (f"{what}: path {worst} {got[worst, :3]} against {paths.radiance[worst]}, margin {paths.margin[worst]:.3e}, "
                                 f"{int((inc & (err > R.TAU)).sum())} paths beyond tau, took {[b for b in R.BRANCHES if paths.took[b][worst]]}")


@pytest.mark.parametrize("thread_per_ray", [False, True], ids=["wavefront", "thread-per-ray"])
@pytest.mark.parametrize("name", PC.NAMES)
def test_trace_radiance_equals_the_replay(luts, name, thread_per_ray):
    case, rays, cb, paths = _reference(luts, name)
    ctx = _context(case.scene)
    try:
        got = ctx.trace_radiance(rays, cb, thread_per_ray=thread_per_ray)
    finally:
        ctx.close()
    _compare(got, paths, f"case {name}, hrpt_trace_radiance")


@pytest.mark.parametrize("name", PC.NAMES)
def test_render_equals_the_replay(luts, name):
    case = PC.case(name, luts)
    ctx = _context(case.scene)
    try:
        ctx.resize(PC.W, PC.H)
        for cb, paths in _camera_reference(luts, name):
            ctx.clear_accumulation()
            ctx.render(cb)
            _compare(ctx.read_accumulation().reshape(-1, 4), paths, f"case {name}, hrpt_render of index {int(cb['m_AccumulationIndex'])}")
    finally:
        ctx.close()


def test_two_level_structure_equals_the_replay(luts):
    case, rays, cb, paths = _reference(luts, "A")
    ctx = _context(case.scene, S.ACCEL_TWO_LEVEL)
    try:
        assert ctx.build_info().structure == S.ACCEL_TWO_LEVEL
        got = ctx.trace_radiance(rays, cb)
    finally:
        ctx.close()
    _compare(got, paths, "case A over the two-level structure")


def test_unfused_bounce0_equals_the_replay(luts, monkeypatch):
    monkeypatch.setenv("HRPT_WF_FUSED_BOUNCE0", "0")
    case = PC.case("C", luts)
    ctx = _context(case.scene)
    try:
        ctx.resize(PC.W, PC.H)
        for cb, paths in _camera_reference(luts, "C"):
            ctx.clear_accumulation()
            ctx.render(cb)
            _compare(ctx.read_accumulation().reshape(-1, 4), paths, f"case C, HRPT_WF_FUSED_BOUNCE0=0, index {int(cb['m_AccumulationIndex'])}")
    finally:
        ctx.close()
