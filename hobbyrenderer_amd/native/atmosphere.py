"""The atmosphere tables (csrc/atmosphere_precompute.cpp): the cached precompute and single producer passes."""
import ctypes as C
import os

import numpy as np

from .. import structs as S
from ._lib import _PKG, HrptError, _check_rc, declare, lib

declare("hrpt_precompute_atmosphere", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])
declare("hrpt_precompute_atmosphere_ex", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int])
declare("hrpt_atmosphere_pass", [C.c_int, C.c_int, C.c_uint32, C.c_uint32] + [C.c_void_p] * 8 + [C.c_int, C.c_int])

ATMOSPHERE_ORDERS = 4        # scattering orders of the default tables (Bruneton's demo value; the reference's own count is unknown)


def _atmosphere_cache_path(orders):
    """Cache file of the tables for this producer source: hobbyrenderer_amd/.cache/ (git-ignored; it travels to the GPU box like the built
    libraries do). The key covers the producer and the arithmetic header, so an edit of either invalidates it."""
    import hashlib
    h = hashlib.sha1()
    for rel in (("csrc", "atmosphere_precompute.cpp"), ("..", "include", "hobbyrt", "detmath.h")):
        with open(os.path.join(_PKG, *rel), "rb") as f:
            h.update(f.read())
    return os.path.join(_PKG, ".cache", f"atmosphere_o{orders}_{h.hexdigest()[:12]}.npz")


def precompute_atmosphere(nthreads=0, orders=ATMOSPHERE_ORDERS, device=-2, cache=True):
    """Stand-ins for bin/bruneton/*.dat (src/CommonResources.cpp:519-569): float32 RGBA tables (transmittance 64 x 256, scattering
    32 x 128 x 256, irradiance 16 x 64) with `orders` scattering orders (csrc/atmosphere_precompute.cpp). device: -1 host threads, >= 0 that
    GPU, -2 the current GPU when there is one. The result does not depend on the executor (bit-identical; tests/test_atmosphere.py), so it
    is cached on disk: four orders take ~40 s on 8 host threads and ~0.1 s on the GPU."""
    path = _atmosphere_cache_path(orders) if cache else None
    if path and os.path.exists(path):
        try:
            with np.load(path) as z:
                t, s, i = z["transmittance"], z["scattering"], z["irradiance"]
            if t.shape == S.LUT_TRANSMITTANCE_SHAPE and s.shape == S.LUT_SCATTERING_SHAPE and i.shape == S.LUT_IRRADIANCE_SHAPE:
                return t, s, i
        except (OSError, ValueError, KeyError):
            pass
    t = np.zeros(S.LUT_TRANSMITTANCE_SHAPE, np.float32)
    s = np.zeros(S.LUT_SCATTERING_SHAPE, np.float32)
    i = np.zeros(S.LUT_IRRADIANCE_SHAPE, np.float32)
    rc = lib.hrpt_precompute_atmosphere_ex(t.ctypes.data, s.ctypes.data, i.ctypes.data, orders, nthreads, device)
    if rc != 0:
        raise HrptError(rc, "hrpt_precompute_atmosphere_ex")
    if path:
        try:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            tmp = f"{path}.{os.getpid()}.tmp.npz"
            np.savez(tmp, transmittance=t, scattering=s, irradiance=i)
            os.replace(tmp, path)
        except OSError:
            pass
    return t, s, i


ATM_PASS_TRANSMITTANCE, ATM_PASS_DIRECT_IRRADIANCE, ATM_PASS_SINGLE, ATM_PASS_DENSITY, ATM_PASS_INDIRECT, ATM_PASS_MULTIPLE = range(6)
_ATM_NS, _ATM_NI, _ATM_NT = 32 * 128 * 256, 16 * 64, 64 * 256


def atmosphere_pass(pass_id, order, first, count, tables, device=-1, nthreads=0):
    """hrpt_atmosphere_pass: texels [first, first + count) of one producer pass (ATM_PASS_*) from the full-size float32 tables in `tables`
    (keys T [64 * 256, 4], dIrr [16 * 64, 3], dR / dM / dDens / dMulti [32 * 128 * 256, 3], scat [32 * 128 * 256, 4]; none is modified), by
    host threads (device < 0) or on that GPU. Returns a dict of the tables the pass writes, zero outside the texels asked for unless the
    table was an input: "out" (pass 0: [64 * 256, 4]; passes 1, 4: [16 * 64, 3]; passes 3, 5: [32 * 128 * 256, 3]), "scat" (passes 2 and
    5: a copy of tables["scat"] with the texels written / accumulated), "dR" and "dM" (pass 2)."""
    shapes = {"T": (_ATM_NT, 4), "dIrr": (_ATM_NI, 3), "dR": (_ATM_NS, 3), "dM": (_ATM_NS, 3), "dDens": (_ATM_NS, 3), "dMulti": (_ATM_NS, 3), "scat": (_ATM_NS, 4)}
    written = ("scat", "dR", "dM") if pass_id == ATM_PASS_SINGLE else (("scat",) if pass_id == ATM_PASS_MULTIPLE else ())
    t = {k: (np.array(tables[k], np.float32) if k in written else np.ascontiguousarray(tables[k], np.float32)).reshape(shape) for k, shape in shapes.items()}
    out = np.zeros((_ATM_NT, 4) if pass_id == ATM_PASS_TRANSMITTANCE else ((_ATM_NI, 3) if pass_id in (ATM_PASS_DIRECT_IRRADIANCE, ATM_PASS_INDIRECT) else (_ATM_NS, 3)), np.float32)
    _check_rc(lib.hrpt_atmosphere_pass(int(pass_id), int(order), int(first), int(count), t["T"].ctypes.data, t["dIrr"].ctypes.data, t["dR"].ctypes.data, t["dM"].ctypes.data,
                                       t["dDens"].ctypes.data, t["dMulti"].ctypes.data, t["scat"].ctypes.data, out.ctypes.data, int(nthreads), int(device)))
    res = {"out": out, "scat": t["scat"]}
    if pass_id == ATM_PASS_SINGLE:
        res["dR"], res["dM"] = t["dR"], t["dM"]
    return res
