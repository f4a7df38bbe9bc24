"""Irradiance probe volumes (csrc/pt_capi_probes.cpp)."""
import ctypes as C

import numpy as np

from .. import structs as S
from ._lib import HrptError, _check_rc, _ptr, address, declare, lib, records

declare("hrpt_probes_create", [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)])
declare("hrpt_probes_destroy", [C.c_void_p], restype=None)
declare("hrpt_probes_update", [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32])
declare("hrpt_probes_query", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32])
declare("hrpt_probes_shade_gbuffer", [C.c_void_p, C.c_void_p, C.c_float])
declare("hrpt_read_probe_irradiance", [C.c_void_p, C.c_void_p, C.c_size_t])
declare("hrpt_get_probe_irradiance_device", [C.c_void_p, C.POINTER(C.c_void_p)])
declare("hrpt_probes_read", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t])
declare("hrpt_probes_write", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t])
declare("hrpt_probes_get_device", [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)])
declare("hrpt_probes_rays_host", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p])
declare("hrpt_probes_blend_host", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int])
declare("hrpt_probes_blend_device", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p])
declare("hrpt_probes_query_host", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int])


def probe_volume(origin, spacing, counts, rays_per_probe, hysteresis=0.97, max_ray_distance=1e4, distance_exponent=50.0, normal_bias=0.0, view_bias=0.0):
    """An S.ProbeVolume record (HrptProbeVolume). Probe (x, y, z) sits at origin + (x, y, z) * spacing."""
    v = np.zeros((), S.ProbeVolume)
    v["origin"], v["spacing"], v["counts"], v["raysPerProbe"] = origin, spacing, counts, rays_per_probe
    v["hysteresis"], v["maxRayDistance"], v["distanceExponent"], v["normalBias"], v["viewBias"] = hysteresis, max_ray_distance, distance_exponent, normal_bias, view_bias
    return v


def _volume_record(volume):
    v = records(volume, "ProbeVolume")
    return v, int(np.prod(v["counts"], dtype=np.uint64)), int(v["raysPerProbe"].reshape(-1)[0])


def probe_points(position, normal, view):
    """S.ProbePoint records from [n, 3] positions, unit normals and unit directions to the viewer."""
    position = np.asarray(position, np.float32)
    pts = np.zeros(len(position), S.ProbePoint)
    pts["position"], pts["normal"], pts["view"] = position, normal, view
    return pts


def probes_rays_host(volume, frame_seed):
    """hrpt_probes_rays_host: the ray records (S.Ray [P * N]) and the N shared directions (float32 [N, 4]) of one update. Needs no GPU."""
    v, P, N = _volume_record(volume)
    if not (0 < P <= 1 << 20 and 0 < N <= 1024):      # the library refuses it too; this keeps the arrays below from being sized by a bad record
        raise HrptError(-1, "probes_rays_host: counts or raysPerProbe out of range")
    rays, dirs = np.zeros(P * N, S.Ray), np.zeros((N, 4), np.float32)
    _check_rc(lib.hrpt_probes_rays_host(v.ctypes.data, int(frame_seed) & 0xFFFFFFFF, rays.ctypes.data, dirs.ctypes.data))
    return rays, dirs


def probes_blend_host(volume, directions, radiance, hits, irradiance, distance, has_history, nthreads=0):
    """hrpt_probes_blend_host: the blend (csrc/pt_probes.h) on host threads; needs no GPU and is bit-identical to the kernel. directions:
    float32 [N, 4]; radiance: float32 [P * N, 4] and hits: S.RayHit [P * N] as trace_radiance / trace_rays returned them; irradiance
    [P, 8, 8, 4] and distance [P, 16, 16, 2]: the atlases before. Returns the atlases after (new arrays)."""
    v, P, N = _volume_record(volume)
    directions, radiance = np.ascontiguousarray(directions, np.float32), np.ascontiguousarray(radiance, np.float32)
    hits = records(hits, "RayHit")
    irr, dist = np.array(irradiance, np.float32, order="C"), np.array(distance, np.float32, order="C")
    if directions.shape != (N, 4) or radiance.shape != (P * N, 4) or hits.shape != (P * N,) or irr.shape != (P,) + S.PROBE_IRRADIANCE_SHAPE or dist.shape != (P,) + S.PROBE_DISTANCE_SHAPE:
        raise ValueError("probes_blend_host: array shapes do not match the volume")
    _check_rc(lib.hrpt_probes_blend_host(v.ctypes.data, directions.ctypes.data, radiance.ctypes.data, hits.ctypes.data, irr.ctypes.data, dist.ctypes.data,
                                         1 if has_history else 0, int(nthreads)))
    return irr, dist


def probes_query_host(volume, irradiance, distance, points, nthreads=0):
    """hrpt_probes_query_host: float32 [n, 4] = (irradiance rgb, inside) at the S.ProbePoint records `points`. Needs no GPU."""
    v, P, _ = _volume_record(volume)
    irr, dist = np.ascontiguousarray(irradiance, np.float32), np.ascontiguousarray(distance, np.float32)
    if irr.shape != (P,) + S.PROBE_IRRADIANCE_SHAPE or dist.shape != (P,) + S.PROBE_DISTANCE_SHAPE:
        raise ValueError("probes_query_host: atlas shapes do not match the volume")
    points = records(points, "ProbePoint")
    out = np.zeros((len(points), 4), np.float32)
    _check_rc(lib.hrpt_probes_query_host(v.ctypes.data, irr.ctypes.data, dist.ctypes.data, points.ctypes.data, out.ctypes.data, len(points), int(nthreads)))
    return out


class ProbeVolume:
    """HrptProbes: an irradiance probe volume on one PathTracerContext (hrpt_probes_*). Close it before its context."""

    def __init__(self, context, volume):
        self._ctx = context
        self.volume, self.probe_count, self.rays_per_probe = _volume_record(volume)
        self._h = C.c_void_p()
        context._check(lib.hrpt_probes_create(context._h, self.volume.ctypes.data, C.byref(self._h)))

    def close(self):
        if self._h:
            lib.hrpt_probes_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, constants, frame_seed, reset=False):
        """hrpt_probes_update: rays for frame_seed, trace_radiance + trace_rays, blend. Asynchronous on the context stream."""
        cb = records(constants, "PathTracerConstants")
        self._ctx._check(lib.hrpt_probes_update(self._h, cb.ctypes.data, int(frame_seed) & 0xFFFFFFFF, S.PROBES_RESET if reset else 0))

    def query(self, points):
        """hrpt_probes_query over host records (S.ProbePoint): float32 [n, 4] = (irradiance rgb, inside). Synchronises."""
        points = records(points, "ProbePoint")
        out = np.zeros((len(points), 4), np.float32)
        self._ctx._check(lib.hrpt_probes_query(self._h, points.ctypes.data, out.ctypes.data, len(points), 0))
        return out

    def query_device(self, points_ptr, out_ptr, count):
        """hrpt_probes_query over device arrays (integer addresses of `count` S.ProbePoint records and float4 slots). Asynchronous."""
        self._ctx._check(lib.hrpt_probes_query(self._h, address(points_ptr), address(out_ptr), int(count), S.PROBES_DEVICE_POINTERS))

    def shade_gbuffer(self, view, intensity=1.0):
        """hrpt_probes_shade_gbuffer: the query at every first hit (planes S.GB_NORMAL and S.GB_DEPTH) into the context's probe irradiance plane."""
        v = records(view, "PlanarViewConstants")      # named: the record must outlive the call
        self._ctx._check(lib.hrpt_probes_shade_gbuffer(self._h, v.ctypes.data, float(intensity)))

    def read(self):
        """(irradiance [P, 8, 8, 4], distance [P, 16, 16, 2]); synchronises."""
        irr = np.empty((self.probe_count,) + S.PROBE_IRRADIANCE_SHAPE, np.float32)
        dist = np.empty((self.probe_count,) + S.PROBE_DISTANCE_SHAPE, np.float32)
        self._ctx._check(lib.hrpt_probes_read(self._h, irr.ctypes.data, irr.nbytes, dist.ctypes.data, dist.nbytes))
        return irr, dist

    def write(self, irradiance=None, distance=None):
        """hrpt_probes_write: installs atlases (None = leave that one); they are the history of the next update."""
        irr = None if irradiance is None else np.ascontiguousarray(irradiance, np.float32)
        dist = None if distance is None else np.ascontiguousarray(distance, np.float32)
        self._ctx._check(lib.hrpt_probes_write(self._h, _ptr(irr), 0 if irr is None else irr.nbytes, _ptr(dist), 0 if dist is None else dist.nbytes))

    def device(self):
        """Device pointers (irradiance, distance) of the atlases."""
        a, b = C.c_void_p(), C.c_void_p()
        self._ctx._check(lib.hrpt_probes_get_device(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value


class ProbeCalls:
    def probes_blend_device(self, volume, directions_ptr, radiance_ptr, hits_ptr, irradiance_ptr, distance_ptr, has_history, hip_stream=0):
        """hrpt_probes_blend_device: the blend kernel over caller-owned device arrays, asynchronous on `hip_stream`."""
        v, _, _ = _volume_record(volume)
        self._check(lib.hrpt_probes_blend_device(self._h, v.ctypes.data, *[address(p) for p in (directions_ptr, radiance_ptr, hits_ptr, irradiance_ptr, distance_ptr)],
                                                 1 if has_history else 0, address(hip_stream)))

    def read_probe_irradiance(self):
        """The plane ProbeVolume.shade_gbuffer wrote: float32 [H, W, 4] (synchronises)."""
        return self._read_image(lib.hrpt_read_probe_irradiance)

    def probe_irradiance_device(self):
        """Device pointer of that plane (None before the first shade_gbuffer and after a resize)."""
        return self._device_ptr(lib.hrpt_get_probe_irradiance_device)
