"""First-hit images and ray batches (csrc/pt_capi_render.cpp): G-buffer, motion vectors, hrpt_trace_rays, hrpt_trace_radiance."""
import ctypes as C

import numpy as np

from .. import structs as S
from ._lib import _frame_params, address, declare, lib, records

declare("hrpt_render_gbuffer", [C.c_void_p, C.c_void_p, C.c_uint32])
declare("hrpt_read_gbuffer", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t])
declare("hrpt_get_gbuffer_device", [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)])
declare("hrpt_render_motion_vectors", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32])
declare("hrpt_read_motion_vectors", [C.c_void_p, C.c_void_p, C.c_size_t])
declare("hrpt_get_motion_vectors_device", [C.c_void_p, C.POINTER(C.c_void_p)])
declare("hrpt_trace_rays", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32])
declare("hrpt_trace_radiance", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32])


class QueryCalls:
    def render_gbuffer(self, constants, planes=S.GB_ALL_PLANES, tile=(0, 0, 0, 0), flags=S.FRAME_DEFAULT, stripes=(1, 0)):
        """hrpt_render_gbuffer: what the primary rays of one accumulation index saw (path vertex 0), into the planes of the bit mask `planes`
        (1 << S.GB_ALBEDO ...). constants.m_Jitter is used as given; tile / flags / stripes as in render. Asynchronous."""
        p = _frame_params(constants, 1, tile, flags, stripes)
        self._check(lib.hrpt_render_gbuffer(self._h, p.ctypes.data, int(planes)))

    def read_gbuffer(self, plane):
        """One G-buffer plane: float32 [H, W, 4], or uint32 [H, W, 4] for S.GB_IDS (synchronises)."""
        return self._read_image(lib.hrpt_read_gbuffer, np.uint32 if plane == S.GB_IDS else np.float32, (int(plane),))

    def gbuffer_device(self, plane):
        """Device pointer of one G-buffer plane (None when it was never requested)."""
        return self._device_ptr(lib.hrpt_get_gbuffer_device, (int(plane),))

    def render_motion_vectors(self, constants, prev_view, planes=0, tile=(0, 0, 0, 0), flags=S.FRAME_DEFAULT, stripes=(1, 0)):
        """hrpt_render_motion_vectors: screen-space motion of the first hit (previous minus current window position in pixels, change of view
        depth, valid flag) for constants["m_View"] against last frame's `prev_view` (S.PlanarViewConstants) and the instances' m_PrevWorld.
        `planes`: G-buffer planes to write in the same pass (0 = motion only). tile / flags / stripes as in render_gbuffer. Asynchronous."""
        p = _frame_params(constants, 1, tile, flags, stripes)
        pv = records(prev_view, "PlanarViewConstants")
        self._check(lib.hrpt_render_motion_vectors(self._h, p.ctypes.data, pv.ctypes.data, int(planes)))

    def read_motion_vectors(self):
        """The motion plane: float32 [H, W, 4] (synchronises)."""
        return self._read_image(lib.hrpt_read_motion_vectors)

    def motion_vectors_device(self):
        """Device pointer of the motion plane (None before the first render_motion_vectors)."""
        return self._device_ptr(lib.hrpt_get_motion_vectors_device)

    def trace_rays(self, rays, shadow=False, thread_per_ray=False):
        """rays: structured array of S.Ray; returns a structured array of S.RayHit (see hrpt_trace_rays). thread_per_ray: the
        one-thread-per-ray cross-check kernel instead of the persistent refilling traversal kernel."""
        rays = records(rays, "Ray")
        hits = np.zeros(len(rays), S.RayHit)
        flags = (S.RAYS_SHADOW if shadow else S.RAYS_CLOSEST) | (S.RAYS_THREAD_PER_RAY if thread_per_ray else 0)
        self._check(lib.hrpt_trace_rays(self._h, rays.ctypes.data, hits.ctypes.data, len(rays), flags))
        return hits

    def trace_rays_device(self, rays_ptr, hits_ptr, count, flags=0):
        """hrpt_trace_rays over device arrays (integer addresses of `count` S.Ray and S.RayHit records). Asynchronous on the context stream."""
        self._check(lib.hrpt_trace_rays(self._h, address(rays_ptr), address(hits_ptr), int(count), int(flags) | S.RAYS_DEVICE_POINTERS))

    def trace_radiance(self, rays, constants, accumulate=False, thread_per_ray=False, out=None, secondary=False):
        """hrpt_trace_radiance: the path-traced radiance along each of `rays` (structured array of S.Ray: origin, unit direction, tmin and RNG
        state; tmax is ignored), float32 [n, 4] = (L.rgb, 1). Of `constants` (S.PathTracerConstants) the sun, m_LightCount and m_MaxBounces
        are read. accumulate: add (L, 1) to `out` (float32 [n, 4], required then) instead; out: the array to write, returned.
        thread_per_ray: the one-thread-per-ray cross-check kernel instead of the wavefront pipeline. secondary (S.RADIANCE_SECONDARY): the rays
        are path segment 1 -- they leave a first hit that is lit elsewhere -- so the bounce loop starts at index 1. Synchronises."""
        rays = records(rays, "Ray")
        if out is None:
            if accumulate:
                raise ValueError("trace_radiance: accumulate needs the array to add to (out)")
            out = np.zeros((len(rays), 4), np.float32)
        if out.dtype != np.float32 or out.shape != (len(rays), 4) or not out.flags.c_contiguous:
            raise ValueError("trace_radiance: out must be a contiguous float32 [len(rays), 4] array")
        cb = records(constants, "PathTracerConstants")
        flags = (S.RADIANCE_ACCUMULATE if accumulate else 0) | (S.RADIANCE_THREAD_PER_RAY if thread_per_ray else 0) | (S.RADIANCE_SECONDARY if secondary else 0)
        self._check(lib.hrpt_trace_radiance(self._h, rays.ctypes.data, out.ctypes.data, len(rays), cb.ctypes.data, flags))
        return out

    def trace_radiance_device(self, rays_ptr, out_ptr, count, constants, flags=0):
        """hrpt_trace_radiance over device arrays (integer addresses of `count` S.Ray records and `count` float4 slots, e.g. a torch tensor's
        data_ptr()): no copies, asynchronous on the context stream. flags: S.RADIANCE_ACCUMULATE / S.RADIANCE_THREAD_PER_RAY / S.RADIANCE_SECONDARY."""
        cb = records(constants, "PathTracerConstants")
        self._check(lib.hrpt_trace_radiance(self._h, address(rays_ptr), address(out_ptr), int(count), cb.ctypes.data, int(flags) | S.RADIANCE_DEVICE_POINTERS))
