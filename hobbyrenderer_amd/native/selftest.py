"""Test hooks (csrc/pt_capi_selftest.cpp): device decoders and samplers against probes, and the acceleration structure read back."""
import ctypes as C

import numpy as np

from .. import structs as S
from ._lib import _check_rc, declare, lib, records

declare("hrpt_selftest_f16_decode", [C.c_void_p, C.c_void_p])
declare("hrpt_selftest_unorm8", [C.c_void_p, C.c_void_p])
declare("hrpt_selftest_sample_textures", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64])
declare("hrpt_selftest_atmosphere", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64])
declare("hrpt_selftest_bvh", [C.c_void_p, C.POINTER(C.c_uint64)])
declare("hrpt_selftest_read_bvh", [C.c_void_p, C.POINTER(S.BvhDump)])
declare("hrpt_selftest_host_build", [C.POINTER(S.SceneDesc), C.c_uint32, C.c_uint32, C.POINTER(S.BvhDump)])

_BVH_DUMP_ARRAYS = (("nodes", S.GpuNode, "nodeCount"), ("nodes4", S.GpuNode4, "node4Count"), ("nodesQ", S.GpuNodeQ, "node4Count"),
                    ("triangles", S.GpuTri, "triangleCount"), ("attributes", S.GpuTriAttr, "triangleCount"),
                    ("tangents", S.GpuTriTangent, "triangleCount"), ("instances", S.GpuInstance, "instanceCount"))


def _read_bvh_dump(call):
    """Size query, then fill (HrptBvhDump): returns a dict of the header fields and one structured numpy array per record array
    (None where the structure has none)."""
    d = S.BvhDump()
    call(d)
    present = {"nodesQ": d.hasNodesQ, "tangents": d.hasTangents}
    arrays = {}
    for name, dtype, count in _BVH_DUMP_ARRAYS:
        if present.get(name, 1):
            arrays[name] = np.zeros(getattr(d, count), dtype)
            setattr(d, name, arrays[name].ctypes.data if arrays[name].size else None)
        else:
            arrays[name] = None
    counts = [getattr(d, c) for _, _, c in _BVH_DUMP_ARRAYS]
    call(d)
    assert counts == [getattr(d, c) for _, _, c in _BVH_DUMP_ARRAYS], "the structure changed between the size query and the fill"
    out = {f: getattr(d, f) for f, _ in S.BvhDump._fields_ if f not in arrays}
    out.update(arrays)
    return out


def host_build_bvh(scene, structure=S.ACCEL_FLAT, separate_collapse=False):
    """hrpt_selftest_host_build: the host builder's structure for a SceneArrays, without a context or a device (see _read_bvh_dump)."""
    desc, keep = scene.desc()

    def call(d):
        _check_rc(lib.hrpt_selftest_host_build(C.byref(desc), int(structure), S.HOST_BUILD_SEPARATE_COLLAPSE if separate_collapse else 0, C.byref(d)))
    out = _read_bvh_dump(call)
    del keep
    return out


def _run_probes(ctx, fn, probes, name):
    probes = records(probes, name)
    results = np.zeros(len(probes), getattr(S, name + "Result"))
    ctx._check(fn(ctx._h, probes.ctypes.data if len(probes) else None, results.ctypes.data if len(probes) else None, len(probes)))
    return results


class SelftestCalls:
    def selftest_f16_decode(self):
        out = np.empty(65536, np.float32)
        self._check(lib.hrpt_selftest_f16_decode(self._h, out.ctypes.data))
        return out

    def selftest_unorm8(self):
        out = np.empty(512, np.float32)
        self._check(lib.hrpt_selftest_unorm8(self._h, out.ctypes.data))
        return out[:256], out[256:]

    def selftest_sample_textures(self, probes):
        """hrpt_selftest_sample_textures: probes = structured array of S.TextureProbe over the uploaded scene's materials; returns a
        structured array of S.TextureProbeResult (the shader's one-by-one, batched and gradient sampling of every probe)."""
        return _run_probes(self, lib.hrpt_selftest_sample_textures, probes, "TextureProbe")

    def selftest_atmosphere(self, probes):
        """hrpt_selftest_atmosphere: probes = structured array of S.AtmosphereProbe; returns a structured array of S.AtmosphereProbeResult
        (the device's sky radiance, sun radiance and transmittance lookup of every probe over the uploaded scene's tables)."""
        return _run_probes(self, lib.hrpt_selftest_atmosphere, probes, "AtmosphereProbe")

    def selftest_bvh(self):
        """Number of child boxes of the acceleration structure that do not contain their subtree (0 = sound)."""
        v = C.c_uint64()
        self._check(lib.hrpt_selftest_bvh(self._h, C.byref(v)))
        return int(v.value)

    def read_bvh(self):
        """hrpt_selftest_read_bvh: the structure the kernels currently walk, as host arrays (see _read_bvh_dump)."""
        return _read_bvh_dump(lambda d: self._check(lib.hrpt_selftest_read_bvh(self._h, C.byref(d))))
