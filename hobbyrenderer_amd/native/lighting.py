"""Lighting at the first hits: deferred direct light (csrc/pt_capi_deferred.cpp), traced indirect light
(csrc/pt_capi_indirect.cpp) and resampled direct light (csrc/pt_capi_restir.cpp)."""
import ctypes as C

import numpy as np

from .. import structs as S
from ._lib import _check_rc, _ptr, _same_shape_images, address, declare, lib, or_default, records

declare("hrpt_deferred_lighting", [C.c_void_p, C.c_void_p, C.POINTER(S.DeferredParams)])
declare("hrpt_deferred_lighting_device", [C.c_void_p, C.POINTER(S.DeferredImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.DeferredParams), C.c_void_p])
declare("hrpt_deferred_rays_host", [C.POINTER(S.DeferredImages), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p])
declare("hrpt_deferred_shade_host", [C.POINTER(S.DeferredImages), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(S.DeferredParams), C.c_int])
declare("hrpt_indirect_lighting", [C.c_void_p, C.c_void_p, C.POINTER(S.IndirectParams)])
declare("hrpt_indirect_compose", [C.c_void_p, C.POINTER(S.IndirectParams)])
declare("hrpt_read_indirect", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t])
declare("hrpt_get_indirect_device", [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)])
declare("hrpt_indirect_lighting_device", [C.c_void_p, C.POINTER(S.IndirectImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.IndirectParams), C.c_void_p])
declare("hrpt_indirect_compose_device", [C.c_void_p, C.POINTER(S.IndirectImages), C.c_uint32, C.c_uint32, C.POINTER(S.IndirectParams), C.c_void_p])
declare("hrpt_indirect_rays_device", [C.c_void_p, C.POINTER(S.IndirectImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.IndirectParams), C.c_void_p, C.c_void_p])
declare("hrpt_indirect_resolve_device", [C.c_void_p, C.POINTER(S.IndirectImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.IndirectParams), C.c_void_p, C.c_void_p])
declare("hrpt_indirect_rays_host", [C.POINTER(S.IndirectImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.IndirectParams), C.c_void_p, C.c_int])
declare("hrpt_indirect_resolve_host", [C.POINTER(S.IndirectImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.IndirectParams), C.c_void_p, C.c_int])
declare("hrpt_indirect_compose_host", [C.POINTER(S.IndirectImages), C.c_uint32, C.c_uint32, C.POINTER(S.IndirectParams), C.c_int])
_RESTIR_HEAD = [C.POINTER(S.RestirImages), C.c_uint32, C.c_uint32, C.c_void_p]
declare("hrpt_restir_lighting", [C.c_void_p, C.c_void_p, C.POINTER(S.RestirParams)])
declare("hrpt_read_restir_reservoirs", [C.c_void_p, C.c_void_p, C.c_size_t])
declare("hrpt_get_restir_device", [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)])
declare("hrpt_restir_lighting_device", [C.c_void_p] + _RESTIR_HEAD + [C.POINTER(S.RestirParams), C.c_void_p])
declare("hrpt_restir_initial_device", [C.c_void_p] + _RESTIR_HEAD + [C.POINTER(S.RestirParams), C.c_void_p, C.c_void_p])
declare("hrpt_restir_temporal_device", [C.c_void_p] + _RESTIR_HEAD + [C.POINTER(S.RestirParams), C.c_void_p, C.c_void_p, C.c_void_p])
declare("hrpt_restir_spatial_device", [C.c_void_p] + _RESTIR_HEAD + [C.POINTER(S.RestirParams), C.c_void_p, C.c_void_p, C.c_void_p])
declare("hrpt_restir_shade_device", [C.c_void_p] + _RESTIR_HEAD + [C.POINTER(S.RestirParams), C.c_void_p, C.c_void_p, C.c_void_p])
declare("hrpt_restir_initial_host", _RESTIR_HEAD + [C.c_void_p, C.POINTER(S.RestirParams), C.c_void_p, C.c_void_p, C.c_int])
declare("hrpt_restir_temporal_host", _RESTIR_HEAD + [C.c_void_p, C.POINTER(S.RestirParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])
declare("hrpt_restir_spatial_host", _RESTIR_HEAD + [C.c_void_p, C.POINTER(S.RestirParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])
declare("hrpt_restir_shade_host", _RESTIR_HEAD + [C.c_void_p, C.POINTER(S.RestirParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])


def _indirect_lobes(params):
    return int(bool(params.flags & S.INDIRECT_DIFFUSE)) + int(bool(params.flags & S.INDIRECT_SPECULAR))


def indirect_rays_host(albedo, normal, geo_normal, depth, constants, params=None, nthreads=0):
    """hrpt_indirect_rays_host: the ray records (S.Ray [lobes, H, W], diffuse first) of every pixel of the four float32 [H, W, 4] planes
    rendered with `constants` (csrc/pt_indirect.h). An untraced record has a NaN origin and zeros elsewhere. Needs no
    GPU; bit-identical to the kernel."""
    imgs, _, shape = _same_shape_images("indirect_rays_host", (albedo, normal, geo_normal, depth))
    params = or_default(params, S.IndirectParams)
    cb = records(constants, "PathTracerConstants")
    out = np.zeros((max(_indirect_lobes(params), 1), shape[0], shape[1]), S.Ray)
    im = S.IndirectImages(*[a.ctypes.data for a in imgs], None, None, None)
    _check_rc(lib.hrpt_indirect_rays_host(C.byref(im), shape[1], shape[0], cb.ctypes.data, C.byref(params), out.ctypes.data, int(nthreads)))
    return out


def indirect_resolve_host(albedo, normal, geo_normal, depth, constants, radiance, params=None, nthreads=0):
    """hrpt_indirect_resolve_host: (diffuse, specular) float32 [H, W, 4] from the radiance of the records (float32 [lobes, H, W, 4], the layout
    of indirect_rays_host); the plane of a lobe that is not flagged comes back as zeros."""
    imgs, _, shape = _same_shape_images("indirect_resolve_host", (albedo, normal, geo_normal, depth))
    params = or_default(params, S.IndirectParams)
    rad = np.ascontiguousarray(radiance, np.float32)
    if rad.shape != (max(_indirect_lobes(params), 1),) + shape:
        raise ValueError("indirect_resolve_host: radiance must be [lobes, H, W, 4]")
    cb = records(constants, "PathTracerConstants")
    dif, spec = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    im = S.IndirectImages(*[a.ctypes.data for a in imgs], dif.ctypes.data, spec.ctypes.data, None)
    _check_rc(lib.hrpt_indirect_resolve_host(C.byref(im), shape[1], shape[0], cb.ctypes.data, C.byref(params), rad.ctypes.data, int(nthreads)))
    return dif, spec


def indirect_compose_host(color, albedo, geo_normal, depth, diffuse, specular, params=None, nthreads=0):
    """hrpt_indirect_compose_host: color + (diffuse * albedo * (1 - metallic) + specular) * intensity at hits, float32 [H, W, 4] (a new array)."""
    imgs, _, shape = _same_shape_images("indirect_compose_host", (color, albedo, geo_normal, depth, diffuse))
    (spec,), _, sshape = _same_shape_images("indirect_compose_host", (specular,))
    if sshape != shape:
        raise ValueError("indirect_compose_host: specular must have the images' shape")
    out = imgs[0].copy()
    im = S.IndirectImages(imgs[1].ctypes.data, None, imgs[2].ctypes.data, imgs[3].ctypes.data, imgs[4].ctypes.data, spec.ctypes.data, out.ctypes.data)
    _check_rc(lib.hrpt_indirect_compose_host(C.byref(im), shape[1], shape[0], C.byref(or_default(params, S.IndirectParams)), int(nthreads)))
    return out


def deferred_rays_host(depth, normal, constants, lights, first_light=0, light_count=None):
    """hrpt_deferred_rays_host: the shadow-ray records (S.Ray [light_count, H, W]) of lights[first_light : first_light + light_count] at every
    pixel of the float32 [H, W, 4] planes S.GB_DEPTH / S.GB_NORMAL rendered with `constants` (csrc/pt_deferred.h). A lit
    pair: origin X, direction L, tmax = the distance to the light; an unlit pair or a miss: origin NaN, the rest 0. Needs no GPU."""
    (depth, normal), _, shape = _same_shape_images("deferred_rays_host", (depth, normal))
    lights = records(lights, "GPULight").reshape(-1)
    light_count = len(lights) - first_light if light_count is None else int(light_count)
    if first_light < 0 or light_count < 0 or first_light + light_count > len(lights):
        raise ValueError("deferred_rays_host: light range outside the list")
    rays = np.zeros((light_count, shape[0], shape[1]), S.Ray)
    im = S.DeferredImages(None, normal.ctypes.data, None, None, depth.ctypes.data, None, None)
    cb = records(constants, "PathTracerConstants")
    _check_rc(lib.hrpt_deferred_rays_host(C.byref(im), shape[1], shape[0], cb.ctypes.data, lights.ctypes.data if len(lights) else None, int(first_light), light_count,
                                          rays.ctypes.data if light_count else None))
    return rays


def deferred_shade_host(albedo, normal, geo_normal, emissive, depth, constants, lights, visibility=None, sun_radiance=None, sky=None, indirect=None,
                        params=None, nthreads=0):
    """hrpt_deferred_shade_host: the lit image, float32 [H, W, 4], of all `lights` over the five float32 [H, W, 4] planes; needs no GPU and is
    bit-identical to PathTracerContext.deferred_lighting / deferred_lighting_device given the same visibilities and atmosphere terms.
    visibility: float32 [len(lights), H, W] (None = 1); sun_radiance: [H, W, 4], the radiance of a directional light at each first hit (None =
    colour x intensity); sky: [H, W, 4] stored at misses (None = zeros); indirect: [H, W, 4], read with S.DEFERRED_INDIRECT in params.flags."""
    imgs, (sun, sk, ind), shape = _same_shape_images("deferred_shade_host", (albedo, normal, geo_normal, emissive, depth), sun_radiance=sun_radiance, sky=sky, indirect=indirect)
    lights = records(lights, "GPULight").reshape(-1)
    vis = None if visibility is None else np.ascontiguousarray(visibility, np.float32)
    if vis is not None and vis.shape != (len(lights), shape[0], shape[1]):
        raise ValueError("deferred_shade_host: visibility must be [lights, H, W]")
    out = np.empty(shape, np.float32)
    im = S.DeferredImages(*[a.ctypes.data for a in imgs], _ptr(ind), out.ctypes.data)
    cb = records(constants, "PathTracerConstants")
    _check_rc(lib.hrpt_deferred_shade_host(C.byref(im), shape[1], shape[0], cb.ctypes.data, lights.ctypes.data if len(lights) else None, len(lights), _ptr(vis), _ptr(sun),
                                           _ptr(sk), C.byref(or_default(params, S.DeferredParams)), int(nthreads)))
    return out


# ---- resampled direct lighting on the host (csrc/pt_restir.h) ---------------------------------------------------
def _restir_host(name, planes, constants, lights, params, sun_radiance=None, sky=None, motion=None):
    """What the four host wrappers share: (the five planes, (sun, sky, motion), shape, constants, lights, a light pointer, params)."""
    imgs, opt, shape = _same_shape_images(name, planes, sun_radiance=sun_radiance, sky=sky, motion=motion)
    cb = records(constants, "PathTracerConstants")
    lights = records(lights, "GPULight").reshape(-1)
    if int(cb.reshape(-1)[0]["m_LightCount"]) > len(lights):
        raise ValueError(f"{name}: m_LightCount exceeds the light list")
    return imgs, opt, shape, cb, lights, (lights.ctypes.data if len(lights) else None), or_default(params, S.RestirParams)


def _restir_records(name, a, shape, dtype=S.RestirReservoir):
    a = np.ascontiguousarray(a, dtype)
    if a.shape != shape[:2]:
        raise ValueError(f"{name}: [H, W] records of the images' size expected")
    return a


def restir_initial_host(planes, constants, lights, params=None, sun_radiance=None, nthreads=0):
    """hrpt_restir_initial_host over the five float32 [H, W, 4] planes (albedo, normal, geo_normal, emissive, depth): (reservoirs
    S.RestirReservoir [H, W], rays S.Ray [H, W] or None without S.RESTIR_INITIAL_VISIBILITY). Needs no GPU; bit-identical to the kernel."""
    imgs, (sun, _, _), shape, cb, lights, lp, params = _restir_host("restir_initial_host", planes, constants, lights, params, sun_radiance)
    res = np.zeros(shape[:2], S.RestirReservoir)
    rays = np.zeros(shape[:2], S.Ray) if params.flags & S.RESTIR_INITIAL_VISIBILITY else None
    im = S.RestirImages(*[a.ctypes.data for a in imgs], None, None, None, res.ctypes.data, None, None)
    _check_rc(lib.hrpt_restir_initial_host(C.byref(im), shape[1], shape[0], cb.ctypes.data, lp, C.byref(params), _ptr(sun), _ptr(rays), int(nthreads)))
    return res, rays


def restir_temporal_host(planes, constants, lights, initial, params=None, sun_radiance=None, motion=None, history=None, initial_visibility=None, nthreads=0):
    """hrpt_restir_temporal_host: the reservoirs after the temporal pass. history: (reservoirs [H, W], keys float32 [H, W, 4]) of the previous
    frame's spatial pass, or None; motion: the motion plane (required with S.RESTIR_TEMPORAL); initial_visibility: float32 [H, W] or None."""
    imgs, (sun, _, mot), shape, cb, lights, lp, params = _restir_host("restir_temporal_host", planes, constants, lights, params, sun_radiance, motion=motion)
    initial = _restir_records("restir_temporal_host", initial, shape)
    vis = None if initial_visibility is None else _restir_records("restir_temporal_host", initial_visibility, shape, np.float32)
    hres = hkey = None
    if history is not None:
        hres = _restir_records("restir_temporal_host", history[0], shape)
        (hkey,), _, kshape = _same_shape_images("restir_temporal_host", (history[1],))
        if kshape != shape:
            raise ValueError("restir_temporal_host: the history keys must have the images' shape")
    out = np.zeros(shape[:2], S.RestirReservoir)
    im = S.RestirImages(*[a.ctypes.data for a in imgs], _ptr(mot), _ptr(hres), _ptr(hkey), out.ctypes.data, None, None)
    _check_rc(lib.hrpt_restir_temporal_host(C.byref(im), shape[1], shape[0], cb.ctypes.data, lp, C.byref(params), _ptr(sun), initial.ctypes.data, _ptr(vis), int(nthreads)))
    return out


def restir_spatial_host(planes, constants, lights, temporal, params=None, sun_radiance=None, nthreads=0):
    """hrpt_restir_spatial_host: (final reservoirs [H, W], keys float32 [H, W, 4], the chosen lights' shadow rays S.Ray [H, W])."""
    imgs, (sun, _, _), shape, cb, lights, lp, params = _restir_host("restir_spatial_host", planes, constants, lights, params, sun_radiance)
    temporal = _restir_records("restir_spatial_host", temporal, shape)
    out, keys, rays = np.zeros(shape[:2], S.RestirReservoir), np.zeros(shape, np.float32), np.zeros(shape[:2], S.Ray)
    im = S.RestirImages(*[a.ctypes.data for a in imgs], None, None, None, out.ctypes.data, keys.ctypes.data, None)
    _check_rc(lib.hrpt_restir_spatial_host(C.byref(im), shape[1], shape[0], cb.ctypes.data, lp, C.byref(params), _ptr(sun), temporal.ctypes.data, rays.ctypes.data, int(nthreads)))
    return out, keys, rays


def restir_shade_host(planes, constants, lights, final, params=None, sun_radiance=None, sky=None, visibility=None, nthreads=0):
    """hrpt_restir_shade_host: the lit image, float32 [H, W, 4], of the final reservoirs; visibility: float32 [H, W] of their shadow rays (None = 1)."""
    imgs, (sun, sk, _), shape, cb, lights, lp, params = _restir_host("restir_shade_host", planes, constants, lights, params, sun_radiance, sky)
    final = _restir_records("restir_shade_host", final, shape)
    vis = None if visibility is None else _restir_records("restir_shade_host", visibility, shape, np.float32)
    out = np.empty(shape, np.float32)
    im = S.RestirImages(*[a.ctypes.data for a in imgs], None, None, None, None, None, out.ctypes.data)
    _check_rc(lib.hrpt_restir_shade_host(C.byref(im), shape[1], shape[0], cb.ctypes.data, lp, C.byref(params), _ptr(sun), _ptr(sk), final.ctypes.data, _ptr(vis), int(nthreads)))
    return out


class LightingCalls:
    def restir_lighting(self, constants, params=None):
        """hrpt_restir_lighting: resampled direct light (one shadow ray per pixel whatever m_LightCount is) from the five planes of
        deferred_lighting and, with S.RESTIR_TEMPORAL, the motion plane, into Output; the reservoirs persist between calls
        (csrc/pt_restir.h). Default params: shadows, sky, both reuse passes, the documented counts. Asynchronous."""
        cb = records(constants, "PathTracerConstants")
        self._check(lib.hrpt_restir_lighting(self._h, cb.ctypes.data, C.byref(or_default(params, S.RestirParams))))

    def read_restir_reservoirs(self):
        """The final reservoirs of the last restir_lighting: S.RestirReservoir [H, W] (synchronises)."""
        out = np.empty((self.height, self.width), S.RestirReservoir)
        self._check(lib.hrpt_read_restir_reservoirs(self._h, out.ctypes.data, out.nbytes))
        return out

    def restir_device(self):
        """(reservoirs, keys) device pointers of that history (None before the first restir_lighting and after a resize)."""
        res, keys = C.c_void_p(), C.c_void_p()
        self._check(lib.hrpt_get_restir_device(self._h, C.byref(res), C.byref(keys)))
        return res.value, keys.value

    def restir_lighting_device(self, images, width, height, constants, params=None, hip_stream=0):
        """The same over caller-owned device arrays (S.RestirImages of device addresses), with this context's scene and lights, on `hip_stream`."""
        cb = records(constants, "PathTracerConstants")
        self._check(lib.hrpt_restir_lighting_device(self._h, C.byref(images), int(width), int(height), cb.ctypes.data, C.byref(or_default(params, S.RestirParams)), address(hip_stream)))

    def restir_initial_device(self, images, width, height, constants, params=None, rays_ptr=0, hip_stream=0):
        """hrpt_restir_initial_device: the initial pass alone into images.reservoirOut (and rays_ptr with S.RESTIR_INITIAL_VISIBILITY)."""
        cb = records(constants, "PathTracerConstants")
        self._check(lib.hrpt_restir_initial_device(self._h, C.byref(images), int(width), int(height), cb.ctypes.data, C.byref(or_default(params, S.RestirParams)), address(rays_ptr),
                                                   address(hip_stream)))

    def restir_temporal_device(self, images, width, height, constants, initial_ptr, params=None, initial_hits_ptr=0, hip_stream=0):
        """hrpt_restir_temporal_device: the temporal pass alone, from the device reservoirs at initial_ptr into images.reservoirOut."""
        cb = records(constants, "PathTracerConstants")
        self._check(lib.hrpt_restir_temporal_device(self._h, C.byref(images), int(width), int(height), cb.ctypes.data, C.byref(or_default(params, S.RestirParams)), address(initial_ptr),
                                                    address(initial_hits_ptr), address(hip_stream)))

    def restir_spatial_device(self, images, width, height, constants, temporal_ptr, params=None, rays_ptr=0, hip_stream=0):
        """hrpt_restir_spatial_device: the spatial pass alone, from temporal_ptr into images.reservoirOut / keyOut (and rays_ptr unless 0)."""
        cb = records(constants, "PathTracerConstants")
        self._check(lib.hrpt_restir_spatial_device(self._h, C.byref(images), int(width), int(height), cb.ctypes.data, C.byref(or_default(params, S.RestirParams)), address(temporal_ptr),
                                                   address(rays_ptr), address(hip_stream)))

    def restir_shade_device(self, images, width, height, constants, final_ptr, params=None, hits_ptr=0, hip_stream=0):
        """hrpt_restir_shade_device: the shade pass alone, from final_ptr and the hit records at hits_ptr (0 = visibility 1) into images.colorOut."""
        cb = records(constants, "PathTracerConstants")
        self._check(lib.hrpt_restir_shade_device(self._h, C.byref(images), int(width), int(height), cb.ctypes.data, C.byref(or_default(params, S.RestirParams)), address(final_ptr),
                                                 address(hits_ptr), address(hip_stream)))

    def deferred_lighting(self, constants, params=None):
        """hrpt_deferred_lighting: direct light with traced shadows, sky and optional probe indirect at the first hits, from the planes
        S.GB_ALBEDO, S.GB_NORMAL, S.GB_GEO_NORMAL, S.GB_EMISSIVE and S.GB_DEPTH of a render_gbuffer / render_motion_vectors with the same
        `constants`, into Output (csrc/pt_deferred.h). Accumulation is not touched. Default params: shadows and sky.
        Asynchronous."""
        cb = records(constants, "PathTracerConstants")
        self._check(lib.hrpt_deferred_lighting(self._h, cb.ctypes.data, C.byref(or_default(params, S.DeferredParams, S.DEFERRED_SHADOWS | S.DEFERRED_SKY))))

    def deferred_lighting_device(self, images, width, height, constants, params=None, hip_stream=0):
        """The same over caller-owned device images (S.DeferredImages of device addresses), with this context's scene and lights, every step
        on `hip_stream` (integer handle)."""
        cb = records(constants, "PathTracerConstants")
        params = or_default(params, S.DeferredParams, S.DEFERRED_SHADOWS | S.DEFERRED_SKY)
        self._check(lib.hrpt_deferred_lighting_device(self._h, C.byref(images), int(width), int(height), cb.ctypes.data, C.byref(params), address(hip_stream)))

    def indirect_lighting(self, constants, params=None):
        """hrpt_indirect_lighting: one traced diffuse and one traced specular ray per first hit, from the planes S.GB_ALBEDO, GB_NORMAL,
        GB_GEO_NORMAL and GB_DEPTH that render_gbuffer wrote with the same `constants`, into two library-owned planes (read_indirect). Output
        and Accumulation are not touched (csrc/pt_indirect.h). Default params: both lobes, seed 0. Asynchronous."""
        cb = records(constants, "PathTracerConstants")
        self._check(lib.hrpt_indirect_lighting(self._h, cb.ctypes.data, C.byref(or_default(params, S.IndirectParams))))

    def indirect_compose(self, params=None):
        """hrpt_indirect_compose: Output += (diffuse * albedo * (1 - metallic) + specular) * params.intensity at hits."""
        self._check(lib.hrpt_indirect_compose(self._h, C.byref(or_default(params, S.IndirectParams))))

    def read_indirect(self, which):
        """One of the planes indirect_lighting wrote (0 = diffuse, 1 = specular): float32 [H, W, 4] (synchronises)."""
        return self._read_image(lib.hrpt_read_indirect, args=(int(which),))

    def indirect_device(self, which):
        """Device pointer of that plane (None before the first indirect_lighting and after a resize)."""
        return self._device_ptr(lib.hrpt_get_indirect_device, (int(which),))

    def indirect_lighting_device(self, images, width, height, constants, params=None, hip_stream=0):
        """The same over caller-owned device images (S.IndirectImages of device addresses), with this context's scene, on `hip_stream`."""
        cb = records(constants, "PathTracerConstants")
        self._check(lib.hrpt_indirect_lighting_device(self._h, C.byref(images), int(width), int(height), cb.ctypes.data, C.byref(or_default(params, S.IndirectParams)), address(hip_stream)))

    def indirect_rays_device(self, images, width, height, constants, rays_ptr, params=None, hip_stream=0):
        """hrpt_indirect_rays_device: the ray-record kernel alone, into a device array of width * height S.Ray per flagged lobe."""
        cb = records(constants, "PathTracerConstants")
        self._check(lib.hrpt_indirect_rays_device(self._h, C.byref(images), int(width), int(height), cb.ctypes.data, C.byref(or_default(params, S.IndirectParams)), address(rays_ptr),
                                                  address(hip_stream)))

    def indirect_resolve_device(self, images, width, height, constants, radiance_ptr, params=None, hip_stream=0):
        """hrpt_indirect_resolve_device: the resolve kernel alone, from a device array of one float4 per record into images.diffuse / specular."""
        cb = records(constants, "PathTracerConstants")
        self._check(lib.hrpt_indirect_resolve_device(self._h, C.byref(images), int(width), int(height), cb.ctypes.data, C.byref(or_default(params, S.IndirectParams)), address(radiance_ptr),
                                                     address(hip_stream)))

    def indirect_compose_device(self, images, width, height, params=None, hip_stream=0):
        """hrpt_indirect_compose_device: images.colorInOut += the composed images.diffuse / images.specular, on `hip_stream`."""
        self._check(lib.hrpt_indirect_compose_device(self._h, C.byref(images), int(width), int(height), C.byref(or_default(params, S.IndirectParams)), address(hip_stream)))
