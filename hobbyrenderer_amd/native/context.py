"""PathTracerContext: the context's own calls (csrc/pt_capi.cpp, pt_capi_scene.cpp and the frame calls of pt_capi_render.cpp) and the
mixins of the subject modules."""
import ctypes as C

import numpy as np

from .. import structs as S
from ._lib import HrptError, _check_rc, _frame_params, address, declare, lib, records
from .geometry import GeometryCalls
from .lighting import LightingCalls
from .post import PostCalls
from .probes import ProbeCalls
from .queries import QueryCalls
from .rcache import RcacheCalls
from .selftest import SelftestCalls

declare("hrpt_create", [C.POINTER(S.DeviceDesc), C.POINTER(C.c_void_p)])
declare("hrpt_destroy", [C.c_void_p], restype=None)
declare("hrpt_upload_scene", [C.c_void_p, C.POINTER(S.SceneDesc)])
declare("hrpt_resize", [C.c_void_p, C.c_uint32, C.c_uint32])
declare("hrpt_render", [C.c_void_p, C.c_void_p])
declare("hrpt_set_stream", [C.c_void_p, C.c_void_p, C.c_int])
declare("hrpt_synchronize", [C.c_void_p])
declare("hrpt_get_device_images", [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)])
declare("hrpt_read_accumulation", [C.c_void_p, C.c_void_p, C.c_size_t])
declare("hrpt_read_output", [C.c_void_p, C.c_void_p, C.c_size_t])
declare("hrpt_read_display", [C.c_void_p, C.c_void_p, C.c_size_t])
declare("hrpt_write_accumulation", [C.c_void_p, C.c_void_p, C.c_size_t])
declare("hrpt_clear_accumulation", [C.c_void_p])
declare("hrpt_resolve_output", [C.c_void_p])
declare("hrpt_resolve_device", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p])
declare("hrpt_resolve_columns_device", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p])
declare("hrpt_allgather", [C.POINTER(C.c_void_p), C.c_int])
declare("hrpt_set_shadow_overlap", [C.c_void_p, C.c_int])
declare("hrpt_set_bvh_builder", [C.c_void_p, C.c_int])
declare("hrpt_set_acceleration_structure", [C.c_void_p, C.c_int])
declare("hrpt_update_instances", [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32])
declare("hrpt_refit_instances", [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32])
declare("hrpt_update_lights", [C.c_void_p, C.c_void_p, C.c_uint32])
declare("hrpt_update_materials", [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32])
declare("hrpt_get_build_info", [C.c_void_p, C.POINTER(S.BuildInfo)])
declare("hrpt_get_stats", [C.c_void_p, C.POINTER(S.Stats)])
declare("hrpt_reset_stats", [C.c_void_p])
declare("hrpt_halton", [C.c_uint32, C.c_uint32], restype=C.c_float)


def allgather(contexts):
    """hrpt_allgather over PathTracerContext objects living in this process (one per GPU, or several on one GPU)."""
    arr = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
    rc = lib.hrpt_allgather(arr, len(contexts))
    if rc != 0:
        raise HrptError(rc, lib.hrpt_last_error(contexts[0]._h).decode() if contexts else "hrpt_allgather")


class PathTracerContext(QueryCalls, GeometryCalls, PostCalls, ProbeCalls, LightingCalls, RcacheCalls, SelftestCalls):
    """One context = one GPU = one stream (include/hobbyrt_pt.h)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        desc = S.DeviceDesc(device, S.ABI_VERSION)
        _check_rc(lib.hrpt_create(C.byref(desc), C.byref(self._h)))
        self.width = self.height = 0
        self._upscale_size = (0, 0)      # display size of the last upscale (PostCalls)

    def _check(self, rc):
        if rc != 0:
            raise HrptError(rc, lib.hrpt_last_error(self._h).decode())

    def _read_image(self, fn, dtype=np.float32, args=()):
        """A context image of the current size, [H, W, 4], through one of the library's readers (synchronises)."""
        out = np.empty((self.height, self.width, 4), dtype)
        self._check(fn(self._h, *args, out.ctypes.data, out.nbytes))
        return out

    def _device_ptr(self, fn, args=()):
        ptr = C.c_void_p()
        self._check(fn(self._h, *args, C.byref(ptr)))
        return ptr.value

    def close(self):
        if self._h:
            lib.hrpt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_scene(self, scene):
        d, keep = scene.desc()
        self._check(lib.hrpt_upload_scene(self._h, C.byref(d)))
        del keep

    def resize(self, width, height):
        self._check(lib.hrpt_resize(self._h, width, height))
        self.width, self.height = width, height

    def render(self, constants, accum_count=1, tile=(0, 0, 0, 0), flags=S.FRAME_DEFAULT, stripes=(1, 0)):
        """stripes = (count, index): of the tile's 8-pixel columns only those with column % count == index are rendered."""
        p = _frame_params(constants, accum_count, tile, flags, stripes)
        self._check(lib.hrpt_render(self._h, p.ctypes.data))

    def set_stream(self, hip_stream):
        """hip_stream: integer handle (e.g. torch.cuda.current_stream().cuda_stream; 0 = the default stream), or None to go
        back to the context's own stream."""
        self._check(lib.hrpt_set_stream(self._h, address(hip_stream), 0 if hip_stream is None else 1))

    def synchronize(self):
        self._check(lib.hrpt_synchronize(self._h))

    def device_images(self):
        a, o = C.c_void_p(), C.c_void_p()
        self._check(lib.hrpt_get_device_images(self._h, C.byref(a), C.byref(o)))
        return a.value, o.value

    def read_accumulation(self):
        return self._read_image(lib.hrpt_read_accumulation)

    def read_output(self):
        return self._read_image(lib.hrpt_read_output)

    def read_display(self):
        return self._read_image(lib.hrpt_read_display)

    def write_accumulation(self, img):
        img = np.ascontiguousarray(img, np.float32)
        self._check(lib.hrpt_write_accumulation(self._h, img.ctypes.data, img.nbytes))

    def clear_accumulation(self):
        """hrpt_clear_accumulation: zeroes the Accumulation image on the context stream, so that the next render may start a fresh frame at
        a non-zero accumulation index (new RNG seeds every frame -- what a temporal accumulator needs)."""
        self._check(lib.hrpt_clear_accumulation(self._h))

    def resolve_output(self):
        self._check(lib.hrpt_resolve_output(self._h))

    def resolve_device(self, accumulation_ptr, output_ptr, pixel_count, hip_stream=0):
        """Output = accum.rgb / accum.a over caller-owned device images, asynchronously on `hip_stream` (integer handle)."""
        self._check(lib.hrpt_resolve_device(self._h, address(accumulation_ptr), address(output_ptr), int(pixel_count), address(hip_stream)))

    def resolve_columns_device(self, shards_ptr, accumulation_ptr, output_ptr, width, height, ranks, hip_stream=0):
        """Rank-major column shards -> Output (= rgb / a, image order) and, unless accumulation_ptr is 0/None, the assembled accumulation image."""
        self._check(lib.hrpt_resolve_columns_device(self._h, address(shards_ptr), address(accumulation_ptr), address(output_ptr), int(width), int(height),
                                                    int(ranks), address(hip_stream)))

    def set_shadow_overlap(self, enabled):
        """Intra-frame overlap of the shadow stage with the next bounce's traversal (default on); turn off for contexts used as lanes of
        a two-frames-in-flight loop."""
        self._check(lib.hrpt_set_shadow_overlap(self._h, 1 if enabled else 0))

    def set_bvh_builder(self, builder):
        """S.BVH_BUILDER_AUTO (default: host SAH below 65 536 triangles, GPU PLOC above), _HOST_SAH, _GPU_LBVH or _GPU_PLOC; used by the next upload_scene / update_instances."""
        self._check(lib.hrpt_set_bvh_builder(self._h, int(builder)))

    def set_acceleration_structure(self, structure):
        """S.ACCEL_AUTO (default), S.ACCEL_FLAT (one world-space tree) or S.ACCEL_TWO_LEVEL (a tree per distinct mesh + a tree over the instances;
        opaque and non-opaque instances alike; a scene with a singular instance matrix is built flat -- build_info().structure tells); used by the next upload_scene."""
        self._check(lib.hrpt_set_acceleration_structure(self._h, int(structure)))

    def update_instances(self, instances, first=0):
        """New transforms for the instances [first, first + len(instances)) (PerInstanceData records); rebuilds the acceleration structure."""
        instances = records(instances, "PerInstanceData")
        self._check(lib.hrpt_update_instances(self._h, instances.ctypes.data, int(first), len(instances)))

    def refit_instances(self, instances, first=0):
        """update_instances for small motions: a tree built on the GPU keeps its hierarchy and gets new boxes (hrpt_refit_instances);
        build_info().usedBuilder then carries S.BVH_BUILDER_REFITTED."""
        instances = records(instances, "PerInstanceData")
        self._check(lib.hrpt_refit_instances(self._h, instances.ctypes.data, int(first), len(instances)))

    def update_lights(self, lights):
        """Replaces the light buffer (GPULight records; the count may change)."""
        lights = records(lights, "GPULight")
        self._check(lib.hrpt_update_lights(self._h, lights.ctypes.data, len(lights)))

    def update_materials(self, materials, first=0):
        """New constants for the materials [first, first + len(materials)) (MaterialConstants records)."""
        materials = records(materials, "MaterialConstants")
        self._check(lib.hrpt_update_materials(self._h, materials.ctypes.data, int(first), len(materials)))

    def build_info(self):
        bi = S.BuildInfo()
        self._check(lib.hrpt_get_build_info(self._h, C.byref(bi)))
        return bi

    def stats(self):
        st = S.Stats()
        self._check(lib.hrpt_get_stats(self._h, C.byref(st)))
        return st

    def reset_stats(self):
        self._check(lib.hrpt_reset_stats(self._h))
