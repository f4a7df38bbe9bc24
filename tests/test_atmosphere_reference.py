"""The atmosphere pinned to tests/atmosphere_reference.py, an independent float64 statement of the published model (CPU part).

Producer: every pass of hobbyrenderer_amd/csrc/atmosphere_precompute.cpp runs through hrpt_atmosphere_pass on host threads, from the real
transmittance table and smooth, positive, analytic stand-ins for the other tables, and is compared texel by texel with the reference:
passes 0, 1 and 4 over their whole tables; passes 2, 3 and 5 on whole rows of 256 texels in x (all 8 nu slices, all 32 mu_s values) at
r = bottom (z = 0: rho = 0, the d == 0 guards fire) and r = top (z = 31), each at y = 0, 63, 64 and 127 (the two ends of the half that
hits the ground and of the half that does not: horizon, nadir, zenith, horizon), and on two seeded interior rows; three horizon rows give
way to near neighbours for one pass each because the reference's own float32 run is too far from its float64 run there (see ROWS).
Run time: about 2000 probes of the sky radiance and the sun radiance through the oracle (which the device code equals bit for bit,
tests/test_atmosphere_reference_gpu.py) against the reference's lookups in the default tables rounded to binary16: cameras on the ground,
2 m below it, at 30 km, 10 m under the top boundary and outside at 100 km; views from nadir to zenith with half a degree either side of
the horizons; the sun from the zenith to 20 degrees below the horizon; nu = +1 and -1; half and one and a half sun radii from the sun's
centre with and without the disk; intensities 1 and 3.5.
tests/test_atmosphere_reference_gpu.py runs the same cases through the HIP kernel and the device probe.

Tolerances come from the reference alone (atmosphere_reference.tolerance): four times the largest difference between its float32 and its
float64 run over the family, plus 4 ulp. A family whose tolerance exceeds 1e-3 of the channel's largest value, or that loses more than
1 % of its cases to branch flips between the two runs, fails test_tolerances_come_from_the_reference_and_stay_under_the_cap."""
import functools

import numpy as np
import pytest

import atmosphere_reference as R
from hobbyrenderer_amd import native, structs as S

F32, F64 = np.float32, np.float64
NS, NI, NT = 32 * 128 * 256, 16 * 64, 64 * 256
_interior = np.random.default_rng(2017)
_INTERIOR_ROWS = [(int(_interior.integers(1, 63)), int(_interior.integers(1, 31))), (int(_interior.integers(65, 127)), int(_interior.integers(1, 31)))]
# (y, z) of the tested rows. In y the table runs from the horizon seen from above the ground (0) to the nadir (63), then from the zenith (64)
# to the horizon (127); z = 0 is r = bottom, z = 31 r = top. Three of the horizon rows are replaced for one pass each: the float32 run of
# the reference differs there from its float64 run by more than the cap allows (grazing rays 875 to 1750 km long, whose end points the
# (r, mu) parameterisation resolves badly in binary32), measured 4 x conditioning / largest value: single scattering (127, 0) 1.5e-3;
# multiple scattering (0, 31) 4.0e-3 and (127, 31) 1.1e-3, with its neighbours up to (123, 31) between 0.8e-3 and 1.9e-3.
_EDGE_ROWS = [(y, z) for z in (0, 31) for y in (0, 63, 64, 127)]
_REPLACED = {2: {(127, 0): (126, 0)}, 5: {(0, 31): (1, 31), (127, 31): (119, 31)}}


class Rows:
    def __init__(self, pass_id):
        self.rows = [_REPLACED.get(pass_id, {}).get(r, r) for r in _EDGE_ROWS] + _INTERIOR_ROWS
        self.first = [(z * 128 + y) * 256 for y, z in self.rows]
        self.x = np.tile(np.arange(256), len(self.rows))
        self.y = np.repeat([y for y, _ in self.rows], 256)
        self.z = np.repeat([z for _, z in self.rows], 256)
        self.index = (self.z * 128 + self.y) * 256 + self.x


ROWS = {pass_id: Rows(pass_id) for pass_id in (2, 3, 5)}
IRR_Y, IRR_X = np.divmod(np.arange(NI), 64)
TR_Y, TR_X = np.divmod(np.arange(NT), 256)
# family -> (pass, order); the channels of a family are listed in _product
FAMILIES = {"transmittance": (0, 0), "direct_irradiance": (1, 0), "single_scattering": (2, 0), "density_order2": (3, 2), "density_order3": (3, 3),
            "indirect_order1": (4, 1), "indirect_order2": (4, 2), "multiple_order2": (5, 2), "multiple_order3": (5, 3)}


def _smooth_scattering_table(scale, phase, channels=3):
    """scale * (1 + 0.4 sin(.) cos(.) + 0.3 sin(.) cos(.)) over (nu, mu_s, mu, r) in [0, 1]^4: positive, a fraction of a period per axis."""
    x = np.arange(256)
    nu, ms, mu, rr = (x // 32) / 7.0, (x % 32) / 31.0, np.arange(128)[:, None] / 127.0, np.arange(32)[:, None, None] / 31.0
    out = np.empty((32, 128, 256, channels), F32)
    for c in range(channels):
        p = phase + 0.9 * c
        out[..., c] = scale * (1.0 + 0.4 * np.sin(2.3 * nu + 1.1 * ms + p) * np.cos(2.9 * mu + 0.5 * p) + 0.3 * np.sin(3.1 * ms + 0.7 * p) * np.cos(2.1 * rr + p))
    return out.reshape(NS, channels)


@functools.lru_cache(None)
def inputs():
    """The input tables of every pass: the real transmittance table (pass 0 of the host executor, itself checked below) and analytic ones."""
    xi, yi = np.arange(64) / 63.0, np.arange(16)[:, None] / 15.0
    d_irr = np.stack([0.5 * (1.0 + 0.5 * np.sin(2.7 * xi + 0.4 + c) * np.cos(1.9 * yi + 0.3 * c)) for c in range(3)], -1).astype(F32).reshape(NI, 3)
    t = {"T": np.ones((NT, 4), F32), "dIrr": d_irr, "dR": _smooth_scattering_table(0.02, 0.3), "dM": _smooth_scattering_table(0.01, 1.7),
         "dDens": _smooth_scattering_table(1e-3, 2.9), "dMulti": _smooth_scattering_table(5e-3, 4.1), "scat": _smooth_scattering_table(0.05, 5.3, 4)}
    t["T"] = native.atmosphere_pass(native.ATM_PASS_TRANSMITTANCE, 0, 0, NT, t, device=-1)["out"]
    for a in t.values():
        a.setflags(write=False)
    return t


def _reference(family, dtype, branches):
    t = inputs()
    pass_id, order = FAMILIES[family]
    rows = ROWS.get(pass_id)
    if pass_id == 0:
        return R.transmittance_pass(TR_X, TR_Y, dtype)
    if pass_id == 1:
        return R.direct_irradiance_pass(t["T"], IRR_X, IRR_Y, dtype, branches)
    if pass_id == 2:
        ray, mie = R.single_scattering_pass(t["T"], rows.x, rows.y, rows.z, dtype)
        return np.concatenate([ray, mie[:, :1], ray, mie], 1)
    if pass_id == 3:
        return R.scattering_density_pass(t["T"], t["dIrr"], t["dR"], t["dM"], t["dMulti"], rows.x, rows.y, rows.z, order, dtype, branches)
    if pass_id == 4:
        return R.indirect_irradiance_pass(t["dR"], t["dM"], t["dMulti"], IRR_X, IRR_Y, order, dtype)
    delta, total = R.multiple_scattering_pass(t["T"], t["dDens"], rows.x, rows.y, rows.z, dtype, scattering_rgb=t["scat"][rows.index, :3])
    return np.concatenate([delta, total], 1)


_REFERENCES = {}


def reference(family):
    """{"ref": float64 values [n, channels], "tol": [n, channels], "cond": per channel, "keep": cases without a branch flip}; computed once."""
    key = "multiple" if family.startswith("multiple") else family          # the multiple-scattering pass does not depend on the order
    if key not in _REFERENCES:
        b32, b64 = [], []
        with np.errstate(all="ignore"):
            ref64, ref32 = _reference(family, F64, b64), _reference(family, F32, b32)
        keep = ~R.branch_flips(b32, b64) if b64 else np.ones(len(ref64), bool)
        tol, cond = R.tolerance(ref32[keep], ref64[keep])
        full = np.zeros_like(ref64)
        full[keep] = tol
        _REFERENCES[key] = {"ref": ref64, "tol": full, "cond": cond, "keep": keep}
    return _REFERENCES[key]


def product(family, device):
    """The family's values from hrpt_atmosphere_pass: host threads run the tested rows one call each, a GPU the whole table in one call."""
    t = inputs()
    pass_id, order = FAMILIES[family]
    if pass_id in (0, 1, 4):
        out = native.atmosphere_pass(pass_id, order, 0, NT if pass_id == 0 else NI, t, device=device)["out"]
        if pass_id == 0:
            assert (out[:, 3] == 1.0).all()
        return out[:, :3]
    rows = ROWS[pass_id]
    spans = [(0, NS)] if device >= 0 else [(first, 256) for first in rows.first]
    parts = []
    for first, count in spans:
        res = native.atmosphere_pass(pass_id, order, first, count, t, device=device)
        sel = rows.index if device >= 0 else np.arange(first, first + 256)
        if pass_id == 2:
            parts.append(np.concatenate([res["scat"][sel], res["dR"][sel], res["dM"][sel]], 1))
        elif pass_id == 3:
            parts.append(res["out"][sel])
        else:
            assert np.array_equal(res["scat"][sel, 3], t["scat"][sel, 3])               # the single-Mie channel is not touched
            parts.append(np.concatenate([res["out"][sel], res["scat"][sel, :3]], 1))
        if device < 0:                                                                  # nothing outside the texels asked for is written
            rest = np.ones(NS, bool)
            rest[first:first + count] = False
            assert np.array_equal(res["scat"][rest], t["scat"][rest])
            if pass_id == 2:
                assert not res["out"].any() and np.array_equal(res["dR"][rest], t["dR"][rest]) and np.array_equal(res["dM"][rest], t["dM"][rest])
            else:
                assert not res["out"][rest].any()
    return np.concatenate(parts)


def check(name, got, ref):
    """got within the family's tolerance of the float64 reference wherever both reference runs took the same branches."""
    got = np.asarray(got, F64)
    err = np.abs(got - ref["ref"])
    keep = ref["keep"]
    worst = (err[keep] / ref["tol"][keep]).max(0)
    print(f"{name}: max |product - float64| per channel {err[keep].max(0)}, as a share of the tolerance {worst}, conditioning {ref['cond']}")
    assert np.isfinite(got[keep]).all(), name
    bad = np.argwhere(keep[:, None] & (err > ref["tol"]))
    assert len(bad) == 0, f"{name}: {len(bad)} values off, first (case, channel) {bad[0]}: got {got[tuple(bad[0])]}, reference {ref['ref'][tuple(bad[0])]}, tolerance {ref['tol'][tuple(bad[0])]}"


@pytest.mark.parametrize("family", list(FAMILIES))
def test_producer_pass_equals_the_float64_reference(family):
    check(family, product(family, -1), reference(family))


# ---------------------------------------------------------------------------------------------------------------- run-time probes
CAMERA_HEIGHTS = (0.0, -2.0, 30000.0, 59990.0, 100000.0)          # metres above the ground: on it, just below, inside, just inside, outside
SUN_ELEVATIONS = (90.0, 60.0, 45.0, 10.0, 2.0, -1.0, -5.0, -12.5, -20.0)
VIEW_AZIMUTHS = (0.0, 70.0, 180.0)                                # against the sun's azimuth
HORIZON_OFFSET = 0.5                                              # degrees either side of the geometric horizons


def _direction(elevation, azimuth):
    e, a = np.radians(elevation), np.radians(azimuth)
    return np.stack(np.broadcast_arrays(np.cos(e) * np.sin(a), np.sin(e), np.cos(e) * np.cos(a)), -1)


def _view_elevations(height):
    """Nadir to zenith, with HORIZON_OFFSET either side of the ground's horizon and (from outside) of the top boundary's."""
    r = R.BOTTOM + max(height, 0.0) / 1000.0
    horizon = -np.degrees(np.arccos(R.BOTTOM / r))
    e = [-90.0, -60.0, -25.0, horizon - 3.0, horizon - HORIZON_OFFSET, horizon + HORIZON_OFFSET, horizon + 3.0, 12.0, 30.0, 55.0, 80.0, 90.0]
    if r > R.TOP:
        top = -np.degrees(np.arccos(R.TOP / r))
        e += [top - HORIZON_OFFSET, top + HORIZON_OFFSET]
    else:
        e += [-8.0, 4.0]
    # from below the ground only upwards: downwards d_min = r - bottom < 0 = d_max there, and u_mu is a quotient of two rounding errors
    return [x for x in e if x > 0.0] if height < 0.0 else e


@functools.lru_cache(None)
def probes():
    rows = []
    for h in CAMERA_HEIGHTS:
        for se in SUN_ELEVATIONS:
            sun = _direction(se, 0.0)
            for ve in _view_elevations(h):
                for az in VIEW_AZIMUTHS:
                    rows.append((h, _direction(ve, az), sun))
            for view in (sun, -sun):                                                   # nu = +1 and -1, without and with the disk
                if h >= 0.0 or view[1] > 0.0:
                    rows += [(h, view, sun), (h, view, sun)]
            if se > 0.0:                                                               # half and one and a half sun radii from the centre
                for radii in (0.5, 1.5):
                    view = _direction(se + np.degrees(radii * R.SUN_ANGULAR_RADIUS), 0.0)
                    rows += [(h, view, sun), (h, view, sun)]
    p = np.zeros(len(rows), S.AtmosphereProbe)
    p["cameraPos"][:, 1] = [r[0] for r in rows]
    p["viewRay"], p["sunDir"] = [r[1] for r in rows], [r[2] for r in rows]
    k = np.arange(len(rows))
    p["addSunDisk"] = k % 2                                                            # the disk pairs above differ in this flag alone
    p["sunIntensity"] = np.where((k // 2) % 2 == 0, 1.0, 3.5)
    p.setflags(write=False)
    return p


def _probe_reference(luts, dtype):
    p = probes()
    t16, s16 = R.to_half(luts[0]), R.to_half(luts[1])
    b = []
    sky = R.rt_sky_radiance(t16, s16, p["cameraPos"], p["viewRay"], p["sunDir"], p["sunIntensity"], p["addSunDisk"], dtype, b)
    sun = R.rt_sun_radiance(t16, p["cameraPos"], p["sunDir"], p["sunIntensity"], dtype)
    pa = R.atmosphere_position(p["cameraPos"], dtype)
    r = np.sqrt((pa * pa).sum(1, dtype=dtype))
    mu = (pa * p["viewRay"].astype(dtype)).sum(1, dtype=dtype) / r
    return {"sky": sky, "sun": sun, "transmittance": R.rt_transmittance_to_top(t16, r, mu, dtype), "r_mu": np.stack([r, mu], 1)}, b


def probe_reference(luts):
    """Families sky (outside the sun's disk), sky_disk (inside it, flag set), sun, transmittance and r_mu (the radius and cosine the
    transmittance is looked up with): each {"ref", "tol", "cond", "keep", "rows", "field"}."""
    if "probes" not in _REFERENCES:
        with np.errstate(all="ignore"):
            (r64, b64), (r32, b32) = _probe_reference(luts, F64), _probe_reference(luts, F32)
        flips = R.branch_flips(b32, b64)
        in_disk = b64[0][:, 3]
        fam = {}
        for name, field, rows in (("sky", "sky", ~in_disk), ("sky_disk", "sky", in_disk), ("sun", "sun", np.ones(len(flips), bool)),
                                  ("transmittance", "transmittance", np.ones(len(flips), bool)), ("r_mu", "r_mu", np.ones(len(flips), bool))):
            keep = ~flips[rows] if field == "sky" else np.ones(int(rows.sum()), bool)
            tol, cond = R.tolerance(r32[field][rows][keep], r64[field][rows][keep])
            full = np.zeros_like(r64[field][rows])
            full[keep] = tol
            fam[name] = {"ref": r64[field][rows], "tol": full, "cond": cond, "keep": keep, "rows": rows, "field": field}
        _REFERENCES["probes"] = fam
    return _REFERENCES["probes"]


def check_probes(luts, got):
    """got: {"sky", "sun"[, "transmittance", "r_mu"]} float32 [n, channels] of every probe."""
    for name, fam in probe_reference(luts).items():
        if fam["field"] in got:
            check("probe " + name, got[fam["field"]][fam["rows"]], fam)


@pytest.fixture(scope="module")
def oracle(luts):
    from hobbyrenderer_amd import scenes
    from oracle.binding import Oracle
    o = Oracle(scenes.config_cube(luts, 16)[0])
    yield o
    o.close()


def test_probes_cover_what_they_claim(luts):
    p = probes()
    fam = probe_reference(luts)
    assert 1800 <= len(p) <= 2600
    assert fam["sky_disk"]["rows"].sum() >= 40 and (p["addSunDisk"][~fam["sky_disk"]["rows"]] == 1).sum() > 500
    nu = (p["viewRay"].astype(F64) * p["sunDir"]).sum(1)
    assert (nu > 1 - 1e-6).sum() >= 40 and (nu < -1 + 1e-6).sum() >= 40
    assert (fam["sun"]["ref"].max(1) == 0).sum() > 100 and (fam["sky"]["ref"].max(1) == 0).sum() > 20       # sun below the horizon; no atmosphere on the ray


def test_run_time_lookups_equal_the_float64_reference(luts, oracle):
    p = probes()
    sky = np.stack([oracle.sky_radiance(q["cameraPos"], q["viewRay"], q["sunDir"], float(q["sunIntensity"]), bool(q["addSunDisk"])) for q in p])
    sun = np.stack([oracle.sun_radiance(q["cameraPos"], q["sunDir"], float(q["sunIntensity"])) for q in p])
    check_probes(luts, {"sky": sky, "sun": sun})


def test_tolerances_come_from_the_reference_and_stay_under_the_cap(luts):
    """Per family and channel: 4 x the float32 conditioning of the reference is at most 1e-3 of the channel's largest reference value, and at
    most 1 % of the cases are left out because the float32 and float64 runs took different branches. Prints the table of the docstrings."""
    fams = {name: reference(name) for name in FAMILIES if name != "multiple_order3"}
    fams.update({"probe " + k: v for k, v in probe_reference(luts).items()})
    for name, f in fams.items():
        largest = np.abs(f["ref"][f["keep"]]).max(0)
        left_out = 1.0 - f["keep"].mean()
        print(f"{name:22s} cond " + " ".join(f"{c:.2e}" for c in f["cond"]) + "  [largest " + " ".join(f"{c:.3e}" for c in largest) + f"]  left out {100 * left_out:.2f} %")
        assert left_out <= 0.01, name
        assert (4.0 * f["cond"] <= 1e-3 * largest).all(), name


# ---------------------------------------------------------------------------------------------------------------- the parameterisation mismatch
MISMATCH_ELEVATIONS = (90.0, 45.0, 10.0)


def transmittance_mismatch(luts):
    """(run-time lookup with the shader's mapping, physical transmittance) rgb at ground level for MISMATCH_ELEVATIONS, by the reference."""
    mu = np.sin(np.radians(MISMATCH_ELEVATIONS))
    mu[0] = 1.0
    r = np.full(len(mu), R.BOTTOM)
    return R.rt_transmittance_to_top(R.to_half(luts[0]), r, mu), R.physical_transmittance(r, mu)


def test_run_time_transmittance_follows_the_shader_mapping_not_the_physics(luts, oracle):
    """The shader maps mu to the table with x_mu = d / (rho + H); the producer fills the table with Bruneton's (d - d_min) / (d_max - d_min).
    Both are kept as they are ("the transmittance parameterisation"): the shader's mapping is the parity contract, the
    standard one is what the reference's own files most likely hold. So from the ground the run-time transmittance towards the zenith is
    that of a ray about twice as long: it equals the reference's shader-mapped lookup and is NOT the physical transmittance. The relative
    difference (printed; quoted in DESIGN.md) shrinks towards the horizon, where the two mappings agree."""
    looked_up, physical = transmittance_mismatch(luts)
    solar = np.asarray(R.SOLAR_IRRADIANCE)
    got = oracle.sun_radiance((0, 0, 0), (0, 1, 0), 1.0).astype(F64)                  # solar irradiance x transmittance(r = bottom, mu = 1)
    tol = probe_reference(luts)["sun"]["tol"].max(0)
    assert (np.abs(got - solar * looked_up[0]) <= tol).all()
    assert (np.abs(got - solar * physical[0]) > tol).all()
    rel = np.abs(looked_up - physical) / physical
    for e, a, b, c in zip(MISMATCH_ELEVATIONS, looked_up, physical, rel):
        print(f"sun elevation {e:4.0f} deg: run-time {a}, physical {b}, relative difference {c}")
    assert (rel[0] > rel[1]).all() and (rel[1] > rel[2]).all()
