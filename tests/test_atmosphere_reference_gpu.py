"""The atmosphere pinned to tests/atmosphere_reference.py (GPU part): the cases, float64 references and tolerances of
tests/test_atmosphere_reference.py, with every producer pass run by the HIP kernel (hrpt_atmosphere_pass on device 0, the whole table in
one launch) and the run-time lookups by hrpt_selftest_atmosphere, which calls atm::sky_radiance, atm::sun_radiance and
atm::transmittance_to_top of csrc/pt_atmosphere.h as they are, one thread per probe, over the uploaded scene's RGBA16F tables. That the
host executor and the kernel return the same bits is tests/test_atmosphere.py's subject; here each side is compared with float64."""
import numpy as np
import pytest

import test_atmosphere_reference as A
from hobbyrenderer_amd import scenes, structs as S

pytestmark = pytest.mark.gpu
F64 = np.float64


@pytest.fixture(scope="module")
def ctx(luts):
    from hobbyrenderer_amd.native import PathTracerContext
    c = PathTracerContext(0)
    c.upload_scene(scenes.config_cube(luts, 16)[0])
    yield c
    c.close()


def test_probe_argument_errors(luts):
    from hobbyrenderer_amd.native import PathTracerContext, lib
    c = PathTracerContext(0)
    try:
        p, r = np.zeros(2, S.AtmosphereProbe), np.zeros(2, S.AtmosphereProbeResult)
        assert lib.hrpt_selftest_atmosphere(c._h, p.ctypes.data, r.ctypes.data, 2) == -4            # no scene
        assert lib.hrpt_selftest_atmosphere(None, p.ctypes.data, r.ctypes.data, 2) == -1
        c.upload_scene(scenes.config_cube(luts, 16)[0])
        assert lib.hrpt_selftest_atmosphere(c._h, None, r.ctypes.data, 2) == -1
        assert lib.hrpt_selftest_atmosphere(c._h, p.ctypes.data, None, 2) == -1
        assert lib.hrpt_selftest_atmosphere(c._h, None, None, 0) == 0                               # nothing to do
        assert lib.hrpt_selftest_atmosphere(c._h, p.ctypes.data, r.ctypes.data, (1 << 24) + 1) == -1   # too many for one call
        assert len(c.selftest_atmosphere(np.zeros(0, S.AtmosphereProbe))) == 0
    finally:
        c.close()


@pytest.mark.parametrize("family", list(A.FAMILIES))
def test_producer_pass_on_the_gpu_equals_the_float64_reference(family):
    A.check(family + " (HIP kernel)", A.product(family, 0), A.reference(family))


def test_device_lookups_equal_the_float64_reference(ctx, luts):
    p = A.probes()
    res = ctx.selftest_atmosphere(p)
    A.check_probes(luts, {"sky": res["sky"], "sun": res["sun"], "transmittance": res["transmittance"], "r_mu": np.stack([res["r"], res["mu"]], 1)})


def test_device_lookups_equal_the_oracle_bit_for_bit(ctx, luts):
    """What lets the CPU part stand for the device: the oracle's sky and sun radiance are the device's, every bit."""
    from oracle.binding import Oracle
    p = A.probes()
    res = ctx.selftest_atmosphere(p)
    o = Oracle(scenes.config_cube(luts, 16)[0])
    try:
        sky = np.stack([o.sky_radiance(q["cameraPos"], q["viewRay"], q["sunDir"], float(q["sunIntensity"]), bool(q["addSunDisk"])) for q in p])
        sun = np.stack([o.sun_radiance(q["cameraPos"], q["sunDir"], float(q["sunIntensity"])) for q in p])
    finally:
        o.close()
    assert np.array_equal(res["sky"].view(np.uint32), sky.view(np.uint32))
    assert np.array_equal(res["sun"].view(np.uint32), sun.view(np.uint32))


def test_device_transmittance_follows_the_shader_mapping_not_the_physics(ctx, luts):
    """The device side of test_run_time_transmittance_follows_the_shader_mapping_not_the_physics: from the ground
    towards the zenith the lookup returns the reference's shader-mapped value, which is not the physical transmittance."""
    looked_up, physical = A.transmittance_mismatch(luts)
    p = np.zeros(1, S.AtmosphereProbe)
    p["viewRay"], p["sunDir"], p["sunIntensity"] = (0, 1, 0), (0, 1, 0), 1.0
    got = ctx.selftest_atmosphere(p)["transmittance"][0].astype(F64)
    tol = A.probe_reference(luts)["transmittance"]["tol"].max(0)
    assert (np.abs(got - looked_up[0]) <= tol).all()
    assert (np.abs(got - physical[0]) > tol).all()
