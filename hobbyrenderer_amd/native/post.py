"""The HDR post stages (csrc/pt_capi_post.cpp): post_process and exposure, bloom, temporal accumulation, upscale, denoise,
demodulate / compose -- each as a context call, over caller-owned device images, and on host threads."""
import ctypes as C

import numpy as np

from .. import structs as S
from ._lib import _check_rc, _ptr, _same_shape_images, address, declare, lib, or_default, records

declare("hrpt_post_process", [C.c_void_p, C.POINTER(S.PostParams)])
declare("hrpt_post_process_device", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(S.PostParams), C.c_void_p])
declare("hrpt_get_exposure", [C.c_void_p, C.POINTER(C.c_float), C.c_void_p])
declare("hrpt_set_exposure", [C.c_void_p, C.c_float])
declare("hrpt_bloom", [C.c_void_p, C.POINTER(S.BloomParams)])
declare("hrpt_bloom_device", [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(S.BloomParams), C.c_void_p])
declare("hrpt_bloom_host", [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(S.BloomParams), C.c_int])
declare("hrpt_bloom_pack_probe", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p])
declare("hrpt_temporal_host", [C.POINTER(S.TemporalImages), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(S.TemporalParams), C.c_int])
declare("hrpt_temporal_device", [C.c_void_p, C.POINTER(S.TemporalImages), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(S.TemporalParams), C.c_void_p])
declare("hrpt_temporal_accumulate", [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(S.TemporalParams)])
declare("hrpt_read_temporal_history", [C.c_void_p, C.c_void_p, C.c_size_t])
declare("hrpt_get_temporal_history_device", [C.c_void_p, C.POINTER(C.c_void_p)])
declare("hrpt_upscale_host", [C.POINTER(S.UpscaleImages), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(S.UpscaleParams), C.c_int])
declare("hrpt_upscale_device", [C.c_void_p, C.POINTER(S.UpscaleImages), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                C.POINTER(S.UpscaleParams), C.c_void_p])
declare("hrpt_upscale", [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(S.UpscaleParams)])
declare("hrpt_read_upscaled", [C.c_void_p, C.c_void_p, C.c_size_t])
declare("hrpt_read_upscale_history", [C.c_void_p, C.c_void_p, C.c_size_t])
declare("hrpt_get_upscaled_device", [C.c_void_p, C.POINTER(C.c_void_p)])
declare("hrpt_denoise_host", [C.POINTER(S.DenoiseImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.DenoiseParams), C.c_int])
declare("hrpt_denoise_device", [C.c_void_p, C.POINTER(S.DenoiseImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.DenoiseParams), C.c_void_p])
declare("hrpt_denoise", [C.c_void_p, C.c_void_p, C.POINTER(S.DenoiseParams)])
declare("hrpt_set_denoise_noise", [C.c_void_p, C.c_void_p])
declare("hrpt_demodulate_host", [C.POINTER(S.DemodulateImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.ModulationParams), C.c_int])
declare("hrpt_compose_host", [C.POINTER(S.ComposeImages), C.c_uint32, C.c_uint32, C.c_int])
declare("hrpt_demodulate_device", [C.c_void_p, C.POINTER(S.DemodulateImages), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(S.ModulationParams), C.c_void_p])
declare("hrpt_compose_device", [C.c_void_p, C.POINTER(S.ComposeImages), C.c_uint32, C.c_uint32, C.c_void_p])
declare("hrpt_demodulate", [C.c_void_p, C.c_void_p, C.POINTER(S.ModulationParams)])
declare("hrpt_compose", [C.c_void_p])
declare("hrpt_read_modulation", [C.c_void_p, C.c_void_p, C.c_size_t])
declare("hrpt_get_modulation_device", [C.c_void_p, C.POINTER(C.c_void_p)])
declare("hrpt_modulation_probe", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p])


def bloom_host(img, params=None, nthreads=0):
    """hrpt_bloom_host: the bloom stage (csrc/pt_bloom.h) on host threads over a float32 [H, W, 4] image; returns the composited image.
    Needs no GPU; bit-identical to PathTracerContext.bloom."""
    img = np.ascontiguousarray(img, np.float32)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError("bloom_host: float32 [H, W, 4] image expected")
    out = np.empty_like(img)
    _check_rc(lib.hrpt_bloom_host(img.ctypes.data, out.ctypes.data, img.shape[1], img.shape[0], C.byref(or_default(params, S.BloomParams)), int(nthreads)))
    return out


def bloom_pack_probe(rgb):
    """Test hook: (packed R11G11B10_FLOAT words, the values read back from them) for float32 [..., 3] colours."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    packed = np.empty(rgb.shape[:-1], np.uint32)
    unpacked = np.empty_like(rgb)
    _check_rc(lib.hrpt_bloom_pack_probe(rgb.ctypes.data, packed.size, packed.ctypes.data, unpacked.ctypes.data))
    return packed, unpacked


def temporal_host(color, motion, depth, normal, history, view, prev_view, params=None, nthreads=0):
    """hrpt_temporal_host: the temporal stage (csrc/pt_temporal.h) on host threads over float32 [H, W, 4] images; needs no GPU and is
    bit-identical to PathTracerContext.temporal_accumulate / temporal_device. color: Output of a render; motion: read_motion_vectors();
    depth / normal: the planes S.GB_DEPTH / S.GB_NORMAL of the same frame; history: what the previous call returned, or None.
    view / prev_view: S.PlanarViewConstants of this and of last frame. view["m_ViewportSize"] must be (W, H), and
    view["m_CameraDirectionOrPosition"] must hold (camera position, 1): scenes.planar_view leaves it zero, the caller fills it.
    Returns (colour out, history out): rgb = blended radiance in both, alpha = color's alpha / the age."""
    imgs, (hist,), shape = _same_shape_images("temporal_host", (color, motion, depth, normal), history=history)
    out, hout = np.empty(shape, np.float32), np.empty(shape, np.float32)
    im = S.TemporalImages(*[a.ctypes.data for a in imgs], _ptr(hist), hout.ctypes.data, out.ctypes.data)
    v, pv = records(view, "PlanarViewConstants"), records(prev_view, "PlanarViewConstants")
    _check_rc(lib.hrpt_temporal_host(C.byref(im), shape[1], shape[0], v.ctypes.data, pv.ctypes.data, C.byref(or_default(params, S.TemporalParams)), int(nthreads)))
    return out, hout


def upscale_host(color, depth, motion, history, display_size, view, prev_view, params=None, nthreads=0):
    """hrpt_upscale_host: the upscale stage (csrc/pt_upscale.h) on host threads; needs no GPU and is bit-identical to
    PathTracerContext.upscale / upscale_device. color / depth / motion: float32 [h, w, 4] images of one render-size frame (Output, the plane
    S.GB_DEPTH, read_motion_vectors()); history: what the previous call returned, float32 [H, W, 4], or None; display_size = (W, H) with
    w <= W <= 4 w and h <= H <= 4 h. view / prev_view: the render-size S.PlanarViewConstants of this and of last frame. params.jitter is the
    sample offset the frame was rendered with. Returns (colour out, history out) at the display size: rgb = the resolved radiance in both,
    alpha = the nearest render texel's alpha / the accumulated sample weight."""
    imgs, _, shape = _same_shape_images("upscale_host", (color, depth, motion))
    W, H = int(display_size[0]), int(display_size[1])
    hist = None if history is None else np.ascontiguousarray(history, np.float32)
    if hist is not None and hist.shape != (H, W, 4):
        raise ValueError("upscale_host: history must be a float32 [H, W, 4] image of the display size")
    out, hout = np.empty((H, W, 4), np.float32), np.empty((H, W, 4), np.float32)
    im = S.UpscaleImages(*[a.ctypes.data for a in imgs], _ptr(hist), hout.ctypes.data, out.ctypes.data)
    v, pv = records(view, "PlanarViewConstants"), records(prev_view, "PlanarViewConstants")
    _check_rc(lib.hrpt_upscale_host(C.byref(im), shape[1], shape[0], W, H, v.ctypes.data, pv.ctypes.data, C.byref(or_default(params, S.UpscaleParams)), int(nthreads)))
    return out, hout


def denoise_host(input, depth, normal, geo_normal, view, params=None, noise=None, color=None, nthreads=0):
    """hrpt_denoise_host: ONE pass of the denoise stage (csrc/pt_denoise.h) on host threads over float32 [H, W, 4] images; needs no GPU and
    is bit-identical to PathTracerContext.denoise_device and to one pass of PathTracerContext.denoise. input: rgb = radiance, a = age (the
    history of the temporal stage); depth / normal / geo_normal: the planes S.GB_DEPTH / S.GB_NORMAL / S.GB_GEO_NORMAL of the same frame;
    noise: a float32 [64, 64, 2] tile, or None for the library's default tile (white noise); color: an image whose alpha the second
    result keeps. view: as for temporal_host. params.iterations must be 1; params.radius and params.frame are used as given.
    Returns output = (filtered rgb, age), or (output, colorOut) when color is given."""
    imgs, _, shape = _same_shape_images("denoise_host", (input, depth, normal, geo_normal))
    tile = None if noise is None else np.ascontiguousarray(noise, np.float32)
    if tile is not None and tile.shape != (64, 64, 2):
        raise ValueError("denoise_host: noise must be a float32 [64, 64, 2] tile")
    _, (col,), _ = _same_shape_images("denoise_host", imgs, color=color)      # checked after the tile, as before the helper existed
    out = np.empty(shape, np.float32)
    cout = None if col is None else np.empty(shape, np.float32)
    im = S.DenoiseImages(*[a.ctypes.data for a in imgs], _ptr(tile), out.ctypes.data, _ptr(col), _ptr(cout))
    v = records(view, "PlanarViewConstants")
    _check_rc(lib.hrpt_denoise_host(C.byref(im), shape[1], shape[0], v.ctypes.data, C.byref(or_default(params, S.DenoiseParams)), int(nthreads)))
    return out if cout is None else (out, cout)


def noise_tile_from_png(path):
    """A float32 [64, 64, 2] noise tile for denoise_host / PathTracerContext.set_denoise_noise from a 64 x 64 PNG, decoded through the
    library's own PNG decoder: tile[y][x] = (R / 255, G / 255), one correctly rounded binary32 division each. The reference's blue-noise
    tile is its data file external/LDR_RG01_0.png (tests/golden/blue_noise_rg_64.png is a copy)."""
    from .. import scene_io
    with open(path, "rb") as f:
        rgba = scene_io.decode_image(f.read())
    if rgba.shape != (64, 64, 4):
        raise ValueError(f"noise_tile_from_png: a 64 x 64 image expected, got {rgba.shape[1]} x {rgba.shape[0]}")
    return np.ascontiguousarray(rgba[..., :2].astype(np.float32) / np.float32(255.0))


def demodulate_host(color, albedo, normal, geo_normal, depth, view, params=None, emissive=None, nthreads=0):
    """hrpt_demodulate_host: the demodulate stage (csrc/pt_modulation.h) on host threads over float32 [H, W, 4]
    images; needs no GPU and is bit-identical to PathTracerContext.demodulate / demodulate_device. color: Output of a render; albedo /
    normal / geo_normal / depth / emissive: the planes S.GB_ALBEDO / S.GB_NORMAL / S.GB_GEO_NORMAL / S.GB_DEPTH / S.GB_EMISSIVE of the same
    frame (emissive None = 0). view: as for temporal_host. Returns (colour out, modulation): colour out = (max(rgb - E, 0) / Mf, alpha),
    modulation = (Mf, 1) at a hit and (1, 1, 1, 0) at a miss."""
    imgs, (em,), shape = _same_shape_images("demodulate_host", (color, albedo, normal, geo_normal, depth), emissive=emissive)
    out, mod = np.empty(shape, np.float32), np.empty(shape, np.float32)
    im = S.DemodulateImages(*[a.ctypes.data for a in imgs], _ptr(em), out.ctypes.data, mod.ctypes.data)
    v = records(view, "PlanarViewConstants")
    _check_rc(lib.hrpt_demodulate_host(C.byref(im), shape[1], shape[0], v.ctypes.data, C.byref(or_default(params, S.ModulationParams)), int(nthreads)))
    return out, mod


def compose_host(color, modulation, emissive=None, nthreads=0):
    """hrpt_compose_host: the compose stage on host threads: (rgb * Mf + E, alpha) with Mf from `modulation` (what demodulate_host
    returned); a texel whose modulation alpha is 0 (a miss) passes through. Bit-identical to PathTracerContext.compose / compose_device."""
    imgs, (em,), shape = _same_shape_images("compose_host", (color, modulation), emissive=emissive)
    out = np.empty(shape, np.float32)
    im = S.ComposeImages(imgs[0].ctypes.data, imgs[1].ctypes.data, _ptr(em), out.ctypes.data)
    _check_rc(lib.hrpt_compose_host(C.byref(im), shape[1], shape[0], int(nthreads)))
    return out


def modulation_probe(albedo, normal, view_dir, rough, metal, floor=0.04):
    """Test hook (hrpt_modulation_probe): the factor Mf of one hit, float32 [3], for an albedo, a unit normal and a unit vector towards the
    camera given directly instead of reconstructed from a depth."""
    a, n, v = [np.ascontiguousarray(x, np.float32).reshape(3) for x in (albedo, normal, view_dir)]
    out = np.empty(3, np.float32)
    _check_rc(lib.hrpt_modulation_probe(a.ctypes.data, n.ctypes.data, v.ctypes.data, float(rough), float(metal), float(floor), out.ctypes.data))
    return out


class PostCalls:
    def post_process(self, params):
        self._check(lib.hrpt_post_process(self._h, C.byref(params)))

    def post_process_device(self, hdr_ptr, display_ptr, pixel_count, params, hip_stream=0):
        """hrpt_post_process_device: the HDR post chain over caller-owned device images (pixel_count float4 each), on the context's
        histogram and exposure, asynchronously on `hip_stream` (integer handle). The way from upscaled_device() to the tonemapper."""
        self._check(lib.hrpt_post_process_device(self._h, address(hdr_ptr), address(display_ptr), int(pixel_count), C.byref(params), address(hip_stream)))

    def exposure(self):
        e = C.c_float(); h = np.zeros(256, np.uint32)
        self._check(lib.hrpt_get_exposure(self._h, C.byref(e), h.ctypes.data))
        return e.value, h

    def set_exposure(self, v):
        self._check(lib.hrpt_set_exposure(self._h, v))

    def bloom(self, params=None):
        """Bloom composited into Output in place (hrpt_bloom): call between render and post_process, once per frame."""
        self._check(lib.hrpt_bloom(self._h, C.byref(or_default(params, S.BloomParams))))

    def bloom_device(self, image_ptr, width, height, params=None, hip_stream=0):
        """The same over a caller-owned device image (width * height float4), asynchronously on `hip_stream` (integer handle)."""
        self._check(lib.hrpt_bloom_device(self._h, address(image_ptr), int(width), int(height), C.byref(or_default(params, S.BloomParams)), address(hip_stream)))

    def temporal_accumulate(self, view, prev_view, params=None):
        """hrpt_temporal_accumulate: reprojected accumulation of Output across frames, in place (csrc/pt_temporal.h).
        Frame order: clear_accumulation -> render -> render_motion_vectors(planes = 1 << S.GB_DEPTH | 1 << S.GB_NORMAL) -> temporal_accumulate
        -> bloom -> post_process. view / prev_view: S.PlanarViewConstants of this and of last frame; view["m_CameraDirectionOrPosition"]
        must hold (camera position, 1) -- scenes.planar_view leaves it zero, the caller fills it. The history lives in the context; the
        first call, the first call after resize and S.TEMPORAL_RESET run without it. Asynchronous."""
        v, pv = records(view, "PlanarViewConstants"), records(prev_view, "PlanarViewConstants")
        self._check(lib.hrpt_temporal_accumulate(self._h, v.ctypes.data, pv.ctypes.data, C.byref(or_default(params, S.TemporalParams))))

    def temporal_device(self, images, width, height, view, prev_view, params=None, hip_stream=0):
        """The same over caller-owned device images (S.TemporalImages of device addresses, width * height float4 each), asynchronously on
        `hip_stream` (integer handle). historyIn may be None (no history); historyOut must differ from it; colorOut may be color."""
        v, pv = records(view, "PlanarViewConstants"), records(prev_view, "PlanarViewConstants")
        self._check(lib.hrpt_temporal_device(self._h, C.byref(images), int(width), int(height), v.ctypes.data, pv.ctypes.data, C.byref(or_default(params, S.TemporalParams)),
                                             address(hip_stream)))

    def read_temporal_history(self):
        """The history the last temporal_accumulate wrote: float32 [H, W, 4], rgb = accumulated radiance, a = age (synchronises)."""
        return self._read_image(lib.hrpt_read_temporal_history)

    def temporal_history_device(self):
        """Device pointer of that image (None before the first temporal_accumulate)."""
        return self._device_ptr(lib.hrpt_get_temporal_history_device)

    def upscale(self, display_width, display_height, view, prev_view, params=None):
        """hrpt_upscale: temporal upscaling of Output (the context's size) into a library-owned display_width x display_height image
        (csrc/pt_upscale.h). Frame order: clear_accumulation -> render(accum_count=1 at index i) ->
        render_motion_vectors(constants with m_Jitter = params.jitter, planes = 1 << S.GB_DEPTH) -> upscale -> bloom_device ->
        post_process_device, the last two over upscaled_device(). params.jitter = (halton(i + 1, 2) - 0.5, halton(i + 1, 3) - 0.5); with
        accum_count > 1 pass (0, 0) and render the planes without jitter. view / prev_view: the render-size views of this and of last
        frame. The history lives in the context; the first call, a call with another display size, the first call after resize and
        S.UPSCALE_RESET run without it. Asynchronous."""
        v, pv = records(view, "PlanarViewConstants"), records(prev_view, "PlanarViewConstants")
        self._check(lib.hrpt_upscale(self._h, int(display_width), int(display_height), v.ctypes.data, pv.ctypes.data, C.byref(or_default(params, S.UpscaleParams))))
        self._upscale_size = (int(display_width), int(display_height))

    def upscale_device(self, images, width, height, display_width, display_height, view, prev_view, params=None, hip_stream=0):
        """The same over caller-owned device images (S.UpscaleImages of device addresses), asynchronously on `hip_stream` (integer handle)."""
        v, pv = records(view, "PlanarViewConstants"), records(prev_view, "PlanarViewConstants")
        self._check(lib.hrpt_upscale_device(self._h, C.byref(images), int(width), int(height), int(display_width), int(display_height),
                                            v.ctypes.data, pv.ctypes.data, C.byref(or_default(params, S.UpscaleParams)), address(hip_stream)))

    def _read_upscale_image(self, fn):
        W, H = self._upscale_size
        out = np.empty((H, W, 4), np.float32)
        self._check(fn(self._h, out.ctypes.data, out.nbytes))
        return out

    def read_upscaled(self):
        """The colour image the last upscale wrote: float32 [H, W, 4] at its display size (synchronises)."""
        return self._read_upscale_image(lib.hrpt_read_upscaled)

    def read_upscale_history(self):
        """The history the last upscale wrote: rgb = resolved radiance, a = accumulated sample weight (synchronises)."""
        return self._read_upscale_image(lib.hrpt_read_upscale_history)

    def upscaled_device(self):
        """Device pointer of the upscaled colour image (None before the first upscale and after resize)."""
        return self._device_ptr(lib.hrpt_get_upscaled_device)

    def denoise(self, view, params=None):
        """hrpt_denoise: the edge-stopping Poisson filter over the temporal history (csrc/pt_denoise.h), after
        temporal_accumulate and before bloom; the planes S.GB_DEPTH, S.GB_NORMAL and S.GB_GEO_NORMAL must have been requested for this frame.
        params.iterations passes with a doubling radius; the last one also writes Output. By default the filtered image becomes the history
        the next temporal_accumulate reprojects (read_temporal_history returns it); with S.DENOISE_OUTPUT_ONLY the history is left alone and
        only Output is filtered. Asynchronous."""
        v = records(view, "PlanarViewConstants")
        self._check(lib.hrpt_denoise(self._h, v.ctypes.data, C.byref(or_default(params, S.DenoiseParams))))

    def denoise_device(self, images, width, height, view, params=None, hip_stream=0):
        """One pass over caller-owned device images (S.DenoiseImages of device addresses; noise None = the default tile), asynchronously on
        `hip_stream` (integer handle). output must differ from input; color / colorOut are both None or both set; colorOut may be color."""
        v = records(view, "PlanarViewConstants")
        self._check(lib.hrpt_denoise_device(self._h, C.byref(images), int(width), int(height), v.ctypes.data, C.byref(or_default(params, S.DenoiseParams)), address(hip_stream)))

    def set_denoise_noise(self, tile):
        """hrpt_set_denoise_noise: the float32 [64, 64, 2] noise tile that denoise, and denoise_device without a tile, use from now on (e.g.
        native.noise_tile_from_png of the reference's blue-noise file); None restores the built-in default tile (white noise)."""
        if tile is None:
            self._check(lib.hrpt_set_denoise_noise(self._h, None))
            return
        t = np.ascontiguousarray(tile, np.float32)
        if t.shape != (64, 64, 2):
            raise ValueError("set_denoise_noise: a float32 [64, 64, 2] tile expected")
        self._check(lib.hrpt_set_denoise_noise(self._h, t.ctypes.data))

    def demodulate(self, view, params=None):
        """hrpt_demodulate: divides the first-hit BRDF factor out of Output, in place, and keeps the factor in a context image
        (csrc/pt_modulation.h). After render and render_motion_vectors / render_gbuffer with the planes S.GB_ALBEDO,
        S.GB_NORMAL, S.GB_GEO_NORMAL, S.GB_EMISSIVE and S.GB_DEPTH of this frame, before temporal_accumulate. view: as for
        temporal_accumulate. Asynchronous."""
        v = records(view, "PlanarViewConstants")
        self._check(lib.hrpt_demodulate(self._h, v.ctypes.data, C.byref(or_default(params, S.ModulationParams))))

    def compose(self):
        """hrpt_compose: multiplies the factor the last demodulate stored back into Output and adds the emissive plane, in place; after
        denoise, before bloom. Asynchronous."""
        self._check(lib.hrpt_compose(self._h))

    def demodulate_device(self, images, width, height, view, params=None, hip_stream=0):
        """The demodulate stage over caller-owned device images (S.DemodulateImages of device addresses; emissive None = 0), asynchronously
        on `hip_stream` (integer handle). colorOut may be color; modulationOut must differ from every other image."""
        v = records(view, "PlanarViewConstants")
        self._check(lib.hrpt_demodulate_device(self._h, C.byref(images), int(width), int(height), v.ctypes.data, C.byref(or_default(params, S.ModulationParams)), address(hip_stream)))

    def compose_device(self, images, width, height, hip_stream=0):
        """The compose stage over caller-owned device images (S.ComposeImages of device addresses), asynchronously on `hip_stream`."""
        self._check(lib.hrpt_compose_device(self._h, C.byref(images), int(width), int(height), address(hip_stream)))

    def read_modulation(self):
        """The factor image the last demodulate wrote: float32 [H, W, 4], rgb = Mf, a = 1 at a hit, 0 at a miss (synchronises)."""
        return self._read_image(lib.hrpt_read_modulation)

    def modulation_device(self):
        """Device pointer of that image (None before the first demodulate and after a resize)."""
        return self._device_ptr(lib.hrpt_get_modulation_device)
