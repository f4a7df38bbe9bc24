"""The irradiance probe volume on the GPU. hrpt_probes_update equals, as bytes, the composition of the public calls
hrpt_probes_rays_host -> hrpt_trace_radiance -> hrpt_trace_rays -> hrpt_probes_blend_host on a second context; the blend kernel equals the
host executor on the CPU cases; the query equals the host executor with host arrays and with device tensors, and at the G-buffer the NumPy
statement fed the read-back planes; a closed, uniformly emissive box gives the known answer; nothing of it leaves a trace in what renders
see; errors leave the atlases as they were.

Every comparison of two implementations is of bits and covers every texel, point or pixel."""
import copy
import math

import numpy as np
import pytest

from hobbyrenderer_amd import native, scenes, structs as S
from scene_helpers import random_soup
import probes_cases as PC
import probes_reference as R
from test_temporal_cpu import u32

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
_CACHE = {}
# (origin, spacing, counts, rays per probe): 3 x 2 x 2 with 100 rays, one probe with 32
VOLUMES = {"cornell-3x2x2": ((-0.6, 0.5, -2.5), (0.6, 1.0, 2.0), (3, 2, 2), 100), "cornell-1": ((0.1, 1.0, -1.2), (1.0, 1.0, 1.0), (1, 1, 1), 32),
           "soup-3x2x2": ((-1.0, -0.5, -1.0), (1.0, 1.0, 2.0), (3, 2, 2), 100), "soup-1": ((0.05, 0.1, -0.05), (1.0, 1.0, 1.0), (1, 1, 1), 32)}


def _scene(luts, name):
    if name not in _CACHE:
        if name == "cornell":
            sc = scenes.cornell_scene(luts, extra_lights=True)        # a point and a spot light
        else:
            sc = random_soup(luts, 500, 21, 0.5, 0.3, True)           # BLEND (stochastic alpha, glass), MASK, textures, a point light
        _CACHE[name] = sc
    return _CACHE[name]


def _volume(key, hysteresis=0.9):
    origin, spacing, counts, rays = VOLUMES[key]
    return native.probe_volume(origin, spacing, counts, rays, hysteresis=hysteresis, max_ray_distance=4.0, distance_exponent=50.0, normal_bias=0.05, view_bias=0.02)


def _context(sc, structure=None):
    ctx = native.PathTracerContext(0)
    try:
        if structure is not None:
            ctx.set_acceleration_structure(structure)
        ctx.upload_scene(sc)
    except Exception:
        ctx.close()
        raise
    return ctx


def _constants(sc, bounces=3):
    view, pos = scenes.planar_view(16, 9)
    return scenes.fill_constants(view, pos, sc, 0, bounces)        # of these the sun, the light count and the bounce count are read


def same_bytes(got, want, what):
    a, b = u32(got), u32(want)
    if not np.array_equal(a, b):
        i = tuple(np.argwhere(a != b)[0])
        raise AssertionError(f"{what}: {int((a != b).sum())} of {a.size} words differ, first at {i}: {got[i]} != {want[i]}")


def _compose(other, vol, cb, seed, irr, dist, has_history):
    """One update through the public calls on the context `other`."""
    rays, dirs = native.probes_rays_host(vol, seed)
    radiance = other.trace_radiance(rays, cb)
    hits = other.trace_rays(rays)
    return native.probes_blend_host(vol, dirs, radiance, hits, irr, dist, has_history)


def _moved(sc, k):
    out = copy.copy(sc)
    inst = sc.instances.copy()
    w = inst["m_World"][k].reshape(4, 4).astype(np.float64)
    shift = np.eye(4); shift[3, :3] = (0.15, 0.1, -0.2)
    inst["m_World"][k] = (w @ shift).astype(np.float32).reshape(inst["m_World"][k].shape)
    inst["m_PrevWorld"][k] = sc.instances["m_World"][k]
    out.instances = inst
    return out


# ---------------------------------------------------------------- 1. update == composition of the public calls
@pytest.mark.parametrize("name,key,structure", [("cornell", "cornell-3x2x2", None), ("soup", "soup-3x2x2", None), ("cornell", "cornell-3x2x2", S.ACCEL_TWO_LEVEL),
                                                ("soup", "soup-1", S.ACCEL_TWO_LEVEL), ("cornell", "cornell-1", None)],
                         ids=["cornell-3x2x2", "soup-3x2x2", "cornell-3x2x2-two-level", "soup-1-two-level", "cornell-1"])
def test_update_equals_the_composition_of_the_public_calls(luts, name, key, structure):
    sc, vol = _scene(luts, name), _volume(key)
    cb = _constants(sc)
    ctx, other = _context(sc, structure), _context(sc, structure)
    pv = native.ProbeVolume(ctx, vol)
    try:
        assert structure is None or ctx.build_info().structure == S.ACCEL_TWO_LEVEL
        irr, dist = pv.read()
        assert not irr.any() and not dist.any()                                   # created zeroed
        steps = [(5, False, False), (6, False, False), (7, False, False), (8, True, False), (9, False, True), (10, False, False)]
        for step, (seed, reset, move) in enumerate(steps):
            if move:                                                              # hrpt_update_instances between two updates
                sc = _moved(sc, len(sc.instances) - 1)
                for c in (ctx, other):
                    c.update_instances(sc.instances[-1:], len(sc.instances) - 1)
            pv.update(cb, seed, reset=reset)
            irr, dist = _compose(other, vol, cb, seed, irr, dist, has_history=step > 0 and not reset)
            got = pv.read()
            same_bytes(got[0], irr, f"step {step}: irradiance")
            same_bytes(got[1], dist, f"step {step}: distance")
            assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and (got[0][..., :3] > 0).any() and (got[0][:, 1:-1, 1:-1, 3] == 1).all()
            assert (got[1][..., 0] > 0).all() and (got[1][..., 0] <= vol["maxRayDistance"]).all()
    finally:
        pv.close(); ctx.close(); other.close()


# ---------------------------------------------------------------- 2. the blend kernel == the host executor
@pytest.fixture(scope="module")
def ctx0():
    ctx = native.PathTracerContext(0)
    yield ctx
    ctx.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to("cuda:0")


@pytest.mark.parametrize("case", PC.BLEND_CASES, ids=PC.blend_id)
def test_blend_kernel_equals_the_host_executor(ctx0, case):
    import torch
    c = PC.blend_case(case)
    want = native.probes_blend_host(c["vol"], c["dirs"], c["radiance"], c["hits"], c["irradiance"], c["distance"], c["history"])
    ref = PC.blend_reference(case)
    d = [_dev(c[k]) for k in ("dirs", "radiance", "hits", "irradiance", "distance")]
    stream = torch.cuda.current_stream()
    ctx0.probes_blend_device(c["vol"], *[t.data_ptr() for t in d], c["history"], stream.cuda_stream)
    stream.synchronize()
    irr = d[3].cpu().numpy().view(np.float32).reshape(want[0].shape)
    dist = d[4].cpu().numpy().view(np.float32).reshape(want[1].shape)
    same_bytes(irr, want[0], "irradiance vs host"); same_bytes(dist, want[1], "distance vs host")
    same_bytes(irr, ref[0], "irradiance vs statement"); same_bytes(dist, ref[1], "distance vs statement")


# ---------------------------------------------------------------- 3. query
@pytest.mark.parametrize("grid", PC.GRIDS, ids=PC.grid_id)
def test_query_equals_the_host_executor_and_write_round_trips(ctx0, grid):
    import torch
    q = PC.query_case(grid)
    pv = native.ProbeVolume(ctx0, q["vol"])
    try:
        pv.write(q["irradiance"], q["distance"])
        irr, dist = pv.read()
        same_bytes(irr, q["irradiance"], "written irradiance"); same_bytes(dist, q["distance"], "written distance")
        pv.write(distance=q["distance"][::-1])                                     # one atlas alone
        same_bytes(pv.read()[0], q["irradiance"], "irradiance after writing distances"); same_bytes(pv.read()[1], q["distance"][::-1], "distance alone")
        pv.write(distance=q["distance"])
        want = native.probes_query_host(q["vol"], q["irradiance"], q["distance"], q["points"])
        same_bytes(pv.query(q["points"]), want, "host arrays")
        same_bytes(want, q["reference"], "host executor vs statement")
        d_pts = _dev(q["points"])
        d_out = torch.full((len(q["points"]), 4), -7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        pv.query_device(d_pts.data_ptr(), d_out.data_ptr(), len(q["points"]))
        ctx0.synchronize()
        same_bytes(d_out.cpu().numpy(), want, "device tensors")
        a, b = pv.device()
        assert a and b and a != b
        assert pv.query(q["points"][:0]).shape == (0, 4)
    finally:
        pv.close()


def _full_view(view, pos):
    full = np.array(view, S.PlanarViewConstants)
    full["m_CameraDirectionOrPosition"] = (pos[0], pos[1], pos[2], 1.0)
    return full


def test_shade_gbuffer_equals_the_statement_on_the_read_back_planes(luts):
    w, h = 61, 37
    sc = _scene(luts, "soup")
    view, pos = scenes.planar_view(w, h, position=(0.0, 0.3, -5.0))
    full = _full_view(view, pos)
    cb = scenes.fill_constants(view, pos, sc, 0, 3)
    cb["m_Jitter"] = (0.0, 0.0)
    ctx = _context(sc)
    pv = native.ProbeVolume(ctx, _volume("soup-3x2x2"))
    try:
        ctx.resize(w, h)
        assert ctx.probe_irradiance_device() is None
        with pytest.raises(native.HrptError, match="HRPT_GB_NORMAL"):
            pv.shade_gbuffer(full, 1.0)
        ctx.render_gbuffer(cb, planes=1 << S.GB_NORMAL)
        with pytest.raises(native.HrptError, match="HRPT_GB_DEPTH"):
            pv.shade_gbuffer(full, 1.0)
        ctx.render_gbuffer(cb, planes=(1 << S.GB_NORMAL) | (1 << S.GB_DEPTH))
        for seed in (1, 2):
            pv.update(cb, seed)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(native.HrptError, match="intensity"):
                pv.shade_gbuffer(full, bad)
        with pytest.raises(native.HrptError, match="m_ViewportSize"):
            pv.shade_gbuffer(_full_view(scenes.planar_view(w + 1, h)[0], pos), 1.0)
        with pytest.raises(native.HrptError):
            ctx.read_probe_irradiance()
        pv.shade_gbuffer(full, 0.75)
        got = ctx.read_probe_irradiance()
        normal, depth = ctx.read_gbuffer(S.GB_NORMAL), ctx.read_gbuffer(S.GB_DEPTH)
        irr, dist = pv.read()
        hit = depth[..., 0] != np.float32(1e10)
        assert 100 < hit.sum() < hit.size - 100                                   # hits and misses in frame
        same_bytes(got, R.shade_gbuffer(pv.volume[0], irr, dist, normal, depth, full, 0.75), "probe irradiance plane")
        assert (got[hit][:, 3] == 1).all() and not got[~hit].any() and (got[hit][:, :3] > 0).any() and np.isfinite(got).all()
        assert ctx.probe_irradiance_device()
        ctx.resize(w, h)                                                          # a resize drops the plane
        assert ctx.probe_irradiance_device() is None
        with pytest.raises(native.HrptError):
            ctx.read_probe_irradiance()
    finally:
        pv.close(); ctx.close()


# ---------------------------------------------------------------- 4. normalisation against a known answer
def test_closed_emissive_box_gives_the_known_answer(luts):
    """A closed box of half-size a, every wall emitting Le, one probe at the centre, one bounce and no lights: every ray returns exactly
    Le. A cosine-weighted mean of equal values is that value up to the summation bound 4 (N + 8) 2^-24; the mean distance to the walls lies
    between a (the face centres) and a sqrt(3) (the corners); the query at the centre returns pi Le."""
    a, n = 1.0, 100
    Le = np.array([2.0, 1.0, 0.5], np.float32)
    b = scenes.SceneBuilder()
    quad = b.add_mesh(*scenes.generate_floor_quad())
    wall = b.add_material(m_BaseColor=(0.5, 0.5, 0.5, 1), m_EmissiveFactor=(float(Le[0]), float(Le[1]), float(Le[2]), 1))
    for axis, offset in (("+y", (0, -a, 0)), ("-y", (0, a, 0)), ("+x", (-a, 0, 0)), ("-x", (a, 0, 0)), ("-z", (0, 0, a)), ("+z", (0, 0, -a))):
        b.add_instance(quad, wall, scenes._mat((2 * a, 1, 2 * a), scenes._ROT_TO[axis], offset))
    sc = b.finalize(luts)
    cb = _constants(sc, bounces=1)
    cb["m_LightCount"] = 0
    vol = native.probe_volume((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1), n, hysteresis=0.9, max_ray_distance=10.0, distance_exponent=50.0)
    ctx = _context(sc)
    pv = native.ProbeVolume(ctx, vol)
    try:
        rays, _ = native.probes_rays_host(vol, 3)
        radiance = ctx.trace_radiance(rays, cb)
        assert np.array_equal(radiance, np.tile(np.append(Le, np.float32(1.0)), (n, 1)))           # exactly Le along every ray
        hits = ctx.trace_rays(rays)
        assert (hits["hit"] == 1).all() and (hits["t"] >= a * (1 - 1e-5)).all() and (hits["t"] <= a * math.sqrt(3.0) * (1 + 1e-5)).all()
        pv.update(cb, 3)
        irr, dist = pv.read()
        bound = 4 * (n + 8) * EPS
        print("irradiance texels: largest relative deviation from Le", float(np.abs(irr[0, 1:-1, 1:-1, :3] / Le - 1).max()), "bound", bound)
        assert np.abs(irr[0, 1:-1, 1:-1, :3].astype(np.float64) / Le - 1.0).max() <= bound
        mean = dist[0, 1:-1, 1:-1, 0]
        print("distance texels: mean in", float(mean.min()), float(mean.max()))
        assert (mean >= a).all() and (mean <= np.float32(a * math.sqrt(3.0))).all()
        pts = native.probe_points([(0.0, 0.0, 0.0)] * 3, [(0, 1, 0), (1, 0, 0), (0.6, 0.0, -0.8)], [(0, 0, 1)] * 3)
        got = pv.query(pts)
        print("query at the centre: largest relative deviation from pi Le", float(np.abs(got[:, :3] / (np.pi * Le.astype(np.float64)) - 1).max()))
        assert np.abs(got[:, :3] / (np.pi * Le.astype(np.float64)) - 1.0).max() <= bound and (got[:, 3] == 1).all()
    finally:
        pv.close(); ctx.close()


# ---------------------------------------------------------------- 5. isolation
def test_renders_do_not_notice_the_volume(luts):
    w, h = 64, 36
    sc, view, pos, cfg = scenes.config_cornell(luts, w, h, extra_lights=True)
    constants = lambda i: scenes.fill_constants(view, pos, sc, i, cfg["max_bounces"])       # noqa: E731

    def state(c):
        return (c.read_accumulation(), c.read_output(), c.read_gbuffer(S.GB_DEPTH), c.exposure(), c.stats(), c.build_info())

    ctx, plain = _context(sc), _context(sc)
    pv = native.ProbeVolume(ctx, _volume("cornell-3x2x2"))
    try:
        for c in (ctx, plain):
            c.resize(w, h)
            c.render(constants(0), accum_count=2)
            c.render_gbuffer(constants(0), planes=(1 << S.GB_DEPTH) | (1 << S.GB_NORMAL))
            c.post_process(S.PostParams(1, 1.0, 0.016, 5.0, -7.0, 23.0, 0.0, 0, 80.0))      # an adapted exposure and a histogram to leave alone
        before = state(ctx)
        pv.update(constants(3), 1)
        pv.update(constants(3), 2)
        got = pv.query(PC.points(pv.volume[0], 256, hostile=False))
        pv.shade_gbuffer(_full_view(view, pos), 1.0)
        assert (got[:, :3] > 0).any() and (ctx.read_probe_irradiance()[..., :3] > 0).any()
        after = state(ctx)
        for k in range(3):
            assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k
        assert before[3][0] == after[3][0] and np.array_equal(before[3][1], after[3][1])
        for k, struct in ((4, S.Stats), (5, S.BuildInfo)):
            for field, _ in struct._fields_:
                assert getattr(before[k], field) == getattr(after[k], field), field
        for c in (ctx, plain):
            c.render(constants(2), accum_count=2)
        same_bytes(ctx.read_accumulation(), plain.read_accumulation(), "the next render")
        a, b = ctx.stats(), plain.stats()
        for field in ("closestRays", "shadowRays", "paths", "megakernelFallbacks", "queuePoolBytes"):
            assert getattr(a, field) == getattr(b, field), field
    finally:
        pv.close(); ctx.close(); plain.close()


# ---------------------------------------------------------------- 6. errors leave the atlases as they were
def test_errors_leave_the_atlases_as_they_were(luts):
    lib = native.lib
    sc = _scene(luts, "cornell")
    cb = np.ascontiguousarray(_constants(sc))
    vol = _volume("cornell-3x2x2")
    ctx = native.PathTracerContext(0)
    try:
        h = native.C.c_void_p()
        bad = vol.copy(); bad["raysPerProbe"] = 0
        assert lib.hrpt_probes_create(ctx._h, bad.ctypes.data, native.C.byref(h)) == -1 and not h.value and b"raysPerProbe 1..1024" in lib.hrpt_last_error(ctx._h)
        assert lib.hrpt_probes_create(ctx._h, None, native.C.byref(h)) == -1 and lib.hrpt_probes_create(ctx._h, vol.ctypes.data, None) == -1
        pv = native.ProbeVolume(ctx, vol)
        try:
            assert lib.hrpt_probes_update(pv._h, cb.ctypes.data, 1, 0) == -4                      # no scene: HRPT_ERR_NO_SCENE
            ctx.upload_scene(sc)
            pv.update(cb, 1)
            before = pv.read()
            too_deep, too_many = cb.copy(), cb.copy()
            too_deep["m_MaxBounces"] = 65; too_many["m_LightCount"] = len(sc.lights) + 1
            for constants, flags in ((too_deep, 0), (too_many, 0), (None, 0), (cb, 2), (cb, 0x100), (cb, 0x80000000)):
                assert lib.hrpt_probes_update(pv._h, None if constants is None else constants.ctypes.data, 2, flags) == -1, flags
            pts, out = PC.points(vol, 64, hostile=False), np.full((64, 4), -3.0, np.float32)
            assert lib.hrpt_probes_query(pv._h, pts.ctypes.data, out.ctypes.data, 64, 1) == -1                    # unknown flag
            assert lib.hrpt_probes_query(pv._h, None, out.ctypes.data, 64, 0) == -1 and lib.hrpt_probes_query(pv._h, pts.ctypes.data, None, 64, 0) == -1
            assert lib.hrpt_probes_query(pv._h, None, None, 0, 0) == 0 and (out == -3.0).all()
            irr, dist = before
            assert lib.hrpt_probes_write(pv._h, irr.ctypes.data, irr.nbytes - 4, dist.ctypes.data, dist.nbytes) == -1
            assert lib.hrpt_probes_write(pv._h, irr.ctypes.data, irr.nbytes, dist.ctypes.data, dist.nbytes + 4) == -1
            assert lib.hrpt_probes_read(pv._h, irr.ctypes.data, 16, None, 0) == -1
            with pytest.raises(native.HrptError, match="hrpt_resize not called"):
                pv.shade_gbuffer(_full_view(*scenes.planar_view(16, 9)), 1.0)
            after = pv.read()
            same_bytes(after[0], before[0], "irradiance after refused calls"); same_bytes(after[1], before[1], "distance after refused calls")
            # ... and the refused updates did not count as history or consume anything: the next update is the second one
            other = _context(sc)
            try:
                pv.update(cb, 2)
                want = _compose(other, vol, cb, 2, before[0], before[1], True)
            finally:
                other.close()
            got = pv.read()
            same_bytes(got[0], want[0], "irradiance of the next update"); same_bytes(got[1], want[1], "distance of the next update")
        finally:
            pv.close()
    finally:
        ctx.close()
