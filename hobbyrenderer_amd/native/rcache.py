"""The world-space hash-grid radiance cache (csrc/pt_capi_rcache.cpp)."""
import ctypes as C

import numpy as np

from .. import structs as S
from ._lib import _check_rc, _ptr, address, declare, lib, or_default, records

declare("hrpt_rcache_create", [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)])
declare("hrpt_rcache_destroy", [C.c_void_p], restype=None)
declare("hrpt_rcache_update", [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32])
declare("hrpt_rcache_indirect", [C.c_void_p, C.c_void_p, C.POINTER(S.RcacheParams)])
declare("hrpt_read_rcache_served", [C.c_void_p, C.c_void_p, C.c_size_t])
declare("hrpt_rcache_clear", [C.c_void_p])
declare("hrpt_rcache_read", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p])
declare("hrpt_rcache_write", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64])
declare("hrpt_rcache_get_device", [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)])
declare("hrpt_rcache_surfaces_device", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p])
declare("hrpt_rcache_insert_host", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int])
declare("hrpt_rcache_insert_device", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p])
declare("hrpt_rcache_resolve_host", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int])
declare("hrpt_rcache_resolve_device", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p])
declare("hrpt_rcache_query_host", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int])
declare("hrpt_rcache_query_device", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p])


def rcache_desc(capacity_log2=22, scene_scale=50.0, level_bias=0.0, radiance_scale=1e3, max_samples=60, stale_frames_max=64, sparse_block=5,
                roughness_threshold=0.1):
    """An S.RcacheDesc record (HrptRcacheDesc); the defaults are the reference's constants."""
    d = np.zeros((), S.RcacheDesc)
    d["capacityLog2"], d["sceneScale"], d["levelBias"], d["radianceScale"] = capacity_log2, scene_scale, level_bias, radiance_scale
    d["maxSamples"], d["staleFramesMax"], d["sparseBlock"], d["roughnessThreshold"] = max_samples, stale_frames_max, sparse_block, roughness_threshold
    return d


def _entries(d):
    return 1 << min(int(d["capacityLog2"].reshape(-1)[0]), 26)      # the library refuses more; this keeps an array from being sized by a bad record


def rcache_table(desc):
    """An empty table for `desc`: (keys uint64 [n], accumulation S.RcacheAccum [n], resolved S.RcacheEntry [n]), n = 2^capacityLog2."""
    n = _entries(records(desc, "RcacheDesc"))
    return np.zeros(n, np.uint64), np.zeros(n, S.RcacheAccum), np.zeros(n, S.RcacheEntry)


def _table(desc, keys, accum, resolved, name):
    d = records(desc, "RcacheDesc")
    n = _entries(d)
    keys = None if keys is None else np.ascontiguousarray(keys, np.uint64)
    accum = None if accum is None else records(accum, "RcacheAccum")
    resolved = None if resolved is None else records(resolved, "RcacheEntry")
    if any(a is not None and a.shape != (n,) for a in (keys, accum, resolved)):
        raise ValueError(f"{name}: the table arrays must have 2^capacityLog2 entries")
    return d, keys, accum, resolved


def _camera(camera_pos):
    cam = np.ascontiguousarray(camera_pos, np.float32)
    if cam.shape != (3,):
        raise ValueError("the camera position is three floats")
    return cam


def rcache_insert_host(desc, camera_pos, keys, accum, samples, drops=0, nthreads=0):
    """hrpt_rcache_insert_host: S.RcacheSample records into a table (csrc/pt_rcache.h) on host threads; needs no GPU. Returns (keys,
    accumulation, drops) after (new arrays)."""
    d, keys, accum, _ = _table(desc, np.array(keys, np.uint64), np.array(accum, S.RcacheAccum), None, "rcache_insert_host")
    samples, cam, dr = records(samples, "RcacheSample"), _camera(camera_pos), np.array([drops], np.uint64)
    _check_rc(lib.hrpt_rcache_insert_host(d.ctypes.data, cam.ctypes.data, keys.ctypes.data, accum.ctypes.data, dr.ctypes.data, _ptr(samples) if len(samples) else None,
                                          len(samples), int(nthreads)))
    return keys, accum, int(dr[0])


def rcache_resolve_host(desc, keys, accum, resolved, flags=0, nthreads=0):
    """hrpt_rcache_resolve_host: one frame's resolve (running mean, ageing, eviction, compaction). Returns the three arrays after (new arrays)."""
    d, keys, accum, resolved = _table(desc, np.array(keys, np.uint64), np.array(accum, S.RcacheAccum), np.array(resolved, S.RcacheEntry), "rcache_resolve_host")
    _check_rc(lib.hrpt_rcache_resolve_host(d.ctypes.data, keys.ctypes.data, accum.ctypes.data, resolved.ctypes.data, int(flags), int(nthreads)))
    return keys, accum, resolved


def rcache_query_host(desc, camera_pos, keys, resolved, points, nthreads=0):
    """hrpt_rcache_query_host: (float32 [n, 4] = (radiance rgb, found), float32 [n] voxel sizes) at the S.RcachePoint records `points`."""
    d, keys, _, resolved = _table(desc, keys, None, resolved, "rcache_query_host")
    points, cam = records(points, "RcachePoint"), _camera(camera_pos)
    out, voxel = np.zeros((len(points), 4), np.float32), np.zeros(len(points), np.float32)
    _check_rc(lib.hrpt_rcache_query_host(d.ctypes.data, cam.ctypes.data, keys.ctypes.data, resolved.ctypes.data, _ptr(points) if len(points) else None,
                                         out.ctypes.data, voxel.ctypes.data, len(points), int(nthreads)))
    return out, voxel


class RadianceCache:
    """HrptRcache: a radiance cache on one PathTracerContext (hrpt_rcache_*). Close it before its context."""

    def __init__(self, context, desc=None):
        self._ctx = context
        self.desc = records(or_default(desc, rcache_desc), "RcacheDesc")
        self.entries = _entries(self.desc)
        self._h = C.c_void_p()
        context._check(lib.hrpt_rcache_create(context._h, self.desc.ctypes.data, C.byref(self._h)))

    def close(self):
        if self._h:
            lib.hrpt_rcache_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, constants, frame_index, flags=0):
        """hrpt_rcache_update: one sparse set of path-traced samples into the table, then the resolve. Asynchronous on the context stream."""
        cb = records(constants, "PathTracerConstants")
        self._ctx._check(lib.hrpt_rcache_update(self._h, cb.ctypes.data, int(frame_index) & 0xFFFFFFFF, int(flags)))

    def indirect(self, constants, params=None):
        """hrpt_rcache_indirect: the context's indirect diffuse plane from the cache, a traced path where it does not serve."""
        cb = records(constants, "PathTracerConstants")
        self._ctx._check(lib.hrpt_rcache_indirect(self._h, cb.ctypes.data, C.byref(or_default(params, S.RcacheParams))))

    def clear(self):
        self._ctx._check(lib.hrpt_rcache_clear(self._h))

    def read(self):
        """(keys uint64 [n], accumulation S.RcacheAccum [n], resolved S.RcacheEntry [n], drops); synchronises."""
        keys, accum, resolved = np.empty(self.entries, np.uint64), np.empty(self.entries, S.RcacheAccum), np.empty(self.entries, S.RcacheEntry)
        drops = np.zeros(1, np.uint64)
        self._ctx._check(lib.hrpt_rcache_read(self._h, keys.ctypes.data, accum.ctypes.data, resolved.ctypes.data, self.entries, drops.ctypes.data))
        return keys, accum, resolved, int(drops[0])

    def write(self, keys, accum, resolved):
        """hrpt_rcache_write: installs a table; one that breaks the bucket invariant is refused."""
        _, keys, accum, resolved = _table(self.desc, keys, accum, resolved, "RadianceCache.write")
        self._ctx._check(lib.hrpt_rcache_write(self._h, keys.ctypes.data, accum.ctypes.data, resolved.ctypes.data, self.entries))

    def device(self):
        """Device pointers (keys, accumulation, resolved, drops) of the table."""
        p = [C.c_void_p() for _ in range(4)]
        self._ctx._check(lib.hrpt_rcache_get_device(self._h, *[C.byref(x) for x in p]))
        return tuple(x.value for x in p)


class RcacheCalls:
    def rcache_surfaces_device(self, rays_ptr, surfaces_ptr, count, hip_stream=0):
        """hrpt_rcache_surfaces_device: S.RcacheSurface records where `count` device S.Ray records land. Asynchronous on `hip_stream`."""
        self._check(lib.hrpt_rcache_surfaces_device(self._h, address(rays_ptr), address(surfaces_ptr), int(count), address(hip_stream)))

    def rcache_insert_device(self, desc, camera_pos, keys_ptr, accum_ptr, drops_ptr, samples_ptr, count, flags=0, hip_stream=0):
        """hrpt_rcache_insert_device over caller-owned device arrays; flags: S.RCACHE_NO_WAVE_COMBINE."""
        d, cam = records(desc, "RcacheDesc"), _camera(camera_pos)
        self._check(lib.hrpt_rcache_insert_device(self._h, d.ctypes.data, cam.ctypes.data, address(keys_ptr), address(accum_ptr), address(drops_ptr), address(samples_ptr),
                                                  int(count), int(flags), address(hip_stream)))

    def rcache_resolve_device(self, desc, keys_ptr, accum_ptr, resolved_ptr, flags=0, hip_stream=0):
        d = records(desc, "RcacheDesc")
        self._check(lib.hrpt_rcache_resolve_device(self._h, d.ctypes.data, address(keys_ptr), address(accum_ptr), address(resolved_ptr), int(flags), address(hip_stream)))

    def rcache_query_device(self, desc, camera_pos, keys_ptr, resolved_ptr, points_ptr, out_ptr, voxel_ptr, count, hip_stream=0):
        d, cam = records(desc, "RcacheDesc"), _camera(camera_pos)
        self._check(lib.hrpt_rcache_query_device(self._h, d.ctypes.data, cam.ctypes.data, address(keys_ptr), address(resolved_ptr), address(points_ptr), address(out_ptr),
                                                 address(voxel_ptr), int(count), address(hip_stream)))

    def read_rcache_served(self):
        """The served plane hrpt_rcache_indirect wrote: float32 [H, W, 4], (cached rgb, 1) where the cache served the pixel (synchronises)."""
        return self._read_image(lib.hrpt_read_rcache_served)
