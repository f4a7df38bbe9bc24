"""Deforming geometry (csrc/pt_capi_geometry.cpp): vertex updates, the quantiser, skinning and morph targets, keyframe animation."""
import ctypes as C

import numpy as np

from .. import structs as S
from ._lib import _check_rc, address, declare, lib, records

declare("hrpt_update_vertices", [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32])
declare("hrpt_update_vertices_device", [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p])
declare("hrpt_quantize_vertices_host", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int])
declare("hrpt_quantize_vertices_device", [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p])
declare("hrpt_skin_vertices_host", [C.POINTER(S.SkinArgs), C.c_void_p, C.c_int])
declare("hrpt_skin_vertices_device", [C.c_void_p, C.POINTER(S.SkinArgs), C.c_void_p, C.c_void_p, C.c_void_p])
declare("hrpt_update_vertices_skinned", [C.c_void_p, C.POINTER(S.SkinArgs), C.c_uint32, C.c_uint32, C.c_void_p])
declare("hrpt_animation_create", [C.POINTER(S.AnimationDesc), C.POINTER(C.c_void_p)])
declare("hrpt_animation_destroy", [C.c_void_p], restype=None)
declare("hrpt_animation_advance", [C.c_void_p, C.c_float])
declare("hrpt_animation_set_times", [C.c_void_p, C.c_void_p, C.c_uint32])
declare("hrpt_animation_get_times", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32])
declare("hrpt_animate_host", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])
declare("hrpt_animate", [C.c_void_p, C.c_void_p, C.c_uint32])
declare("hrpt_get_animation_device", [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)])
declare("hrpt_read_animation", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
declare("hrpt_animation_release", [C.c_void_p, C.c_void_p])


def quantize_vertices_host(vertices, nthreads=0):
    """hrpt_quantize_vertices_host: S.VertexFloat records -> S.VertexQuantized records by the library's quantiser (csrc/pt_deform.h) on host
    threads; needs no GPU and is bit-identical to PathTracerContext.quantize_vertices_device and to scenes.quantize_vertices."""
    v = records(vertices, "VertexFloat")
    out = np.zeros(len(v), S.VertexQuantized)
    _check_rc(lib.hrpt_quantize_vertices_host(v.ctypes.data if len(v) else None, len(v), out.ctypes.data if len(v) else None, int(nthreads)))
    return out


def animation_desc(samplers=(), channels=(), nodes=(), joints=(), key_times=(), key_values=(), targets=(), node_instances=(), animation_count=0,
                   morph_weight_count=0, reserved=0):
    """The tables of an animation as contiguous arrays in the library's layouts and the S.AnimationDesc over them: (desc, arrays). The
    arrays must outlive the desc. samplers S.AnimSampler, channels S.AnimChannel, nodes S.AnimNode, joints S.AnimJoint, key_times float32
    [keys], key_values float32 [keys, 4], targets and node_instances uint32."""
    table = lambda a, name: records(a, name) if len(a) else np.zeros(0, getattr(S, name))      # noqa: E731
    arrays = [table(samplers, "AnimSampler"), table(channels, "AnimChannel"), table(nodes, "AnimNode"),
              table(joints, "AnimJoint"), np.ascontiguousarray(key_times, np.float32).reshape(-1),
              np.ascontiguousarray(key_values, np.float32).reshape(-1, 4), np.ascontiguousarray(targets, np.uint32).reshape(-1),
              np.ascontiguousarray(node_instances, np.uint32).reshape(-1)]
    if len(arrays[5]) != len(arrays[4]):
        raise ValueError("animation_desc: one float4 value per key time expected")
    counts = [len(arrays[k]) for k in (0, 1, 2, 3, 4, 6, 7)]
    desc = S.AnimationDesc(*[a.ctypes.data if a.size else None for a in arrays], *counts, int(animation_count), int(morph_weight_count), int(reserved))
    return desc, arrays


class Animation:
    """hrpt_animation_create: validated, resolved copy of animation tables (animation_desc's keywords); context-free. times / durations,
    advance(dt) and set_times are the host clock; evaluate_host runs csrc/pt_anim.h on host threads; PathTracerContext.animate runs it on
    the device."""

    def __init__(self, **tables):
        desc, arrays = animation_desc(**tables)
        self._h = C.c_void_p()
        _check_rc(lib.hrpt_animation_create(C.byref(desc), C.byref(self._h)))
        self.animation_count, self.node_count = desc.animationCount, desc.nodeCount
        self.joint_count, self.morph_weight_count = desc.jointCount, desc.morphWeightCount

    def close(self):
        if self._h:
            lib.hrpt_animation_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def advance(self, dt):
        _check_rc(lib.hrpt_animation_advance(self._h, float(dt)))

    def set_times(self, times):
        times = np.ascontiguousarray(times, np.float32).reshape(-1)
        _check_rc(lib.hrpt_animation_set_times(self._h, times.ctypes.data if times.size else None, len(times)))

    def _clock(self, which):
        out = np.zeros(self.animation_count, np.float32)
        args = [None, None]
        args[which] = out.ctypes.data
        _check_rc(lib.hrpt_animation_get_times(self._h, *args, self.animation_count))
        return out

    @property
    def times(self):
        return self._clock(0)

    @property
    def durations(self):
        return self._clock(1)

    def evaluate_host(self, instances=None, nthreads=0):
        """hrpt_animate_host at the current times: (instances, palette [joints, 3, 4], weights, node worlds [nodes, 4, 4]). `instances`
        (S.PerInstanceData records of the whole scene, or None) is not modified: the first result is the rolled and moved copy."""
        out = None if instances is None else np.array(instances, S.PerInstanceData, copy=True, order="C")
        palette = np.zeros((self.joint_count, 3, 4), np.float32)
        weights = np.zeros(self.morph_weight_count, np.float32)
        worlds = np.zeros((self.node_count, 4, 4), np.float32)
        _check_rc(lib.hrpt_animate_host(self._h, None, None if out is None else out.ctypes.data, 0 if out is None else len(out),
                                        palette.ctypes.data, weights.ctypes.data, worlds.ctypes.data, int(nthreads)))
        return out, palette, weights, worlds


def skin_arrays(base, joints=None, weights=None, joint_matrices=None, deltas=None, morph_weights=None):
    """The arrays of an S.SkinArgs in the layout the library reads: base S.VertexFloat [count]; joints uint16 [count, 4], weights float32
    [count, 4] and joint_matrices float32 [jointCount, 3, 4] (or all three None); deltas S.SkinMorphDelta [targetCount, count] and
    morph_weights float32 [targetCount] (or both None). Returns (arrays, count, jointCount, targetCount); what was given as None stays None."""
    base = records(base, "VertexFloat")
    n = len(base)
    if joints is not None:
        joints = np.ascontiguousarray(joints, np.uint16).reshape(n, 4)
        weights = np.ascontiguousarray(weights, np.float32).reshape(n, 4)
        joint_matrices = np.ascontiguousarray(joint_matrices, np.float32).reshape(-1, 3, 4)
    if deltas is not None:
        morph_weights = np.ascontiguousarray(morph_weights, np.float32).reshape(-1)
        deltas = records(deltas, "SkinMorphDelta").reshape(len(morph_weights), n)
    arrays = (base, joints, weights, joint_matrices, deltas, morph_weights)
    return arrays, n, 0 if joints is None else len(joint_matrices), 0 if deltas is None else len(morph_weights)


def _aligned_copy(a, align=16):
    """A copy of array `a` whose first byte lies on a multiple of `align` (NumPy promises no more than the item's own alignment)."""
    raw = np.empty(a.nbytes + align, np.uint8)
    start = -raw.ctypes.data % align
    out = raw[start:start + a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


def skin_vertices_host(base, joints=None, weights=None, joint_matrices=None, deltas=None, morph_weights=None, nthreads=0):
    """hrpt_skin_vertices_host: morph targets, then four-joint skinning, then unit normal and tangent (csrc/pt_skin.h) of the bind pose
    `base` (S.VertexFloat records) on host threads; the arrays are those of skin_arrays(). Returns S.VertexFloat records. Needs no GPU and
    is bit-identical to PathTracerContext.skin_vertices_device and to tests/skin_reference.py. A joint index out of range raises."""
    arrays, n, joint_count, target_count = skin_arrays(base, joints, weights, joint_matrices, deltas, morph_weights)
    arrays = [None if a is None else _aligned_copy(a) for a in arrays]
    out = _aligned_copy(np.zeros(n, S.VertexFloat))
    args = S.SkinArgs(*[None if a is None or not a.size else a.ctypes.data for a in arrays], n, joint_count, target_count, 0)
    _check_rc(lib.hrpt_skin_vertices_host(C.byref(args), out.ctypes.data if n else None, int(nthreads)))
    return out


def _device_skin_args(base, joints, weights, joint_matrices, deltas, morph_weights, count, joint_count, target_count):
    return S.SkinArgs(*[address(p) for p in (base, joints, weights, joint_matrices, deltas, morph_weights)], int(count), int(joint_count), int(target_count), 0)


class GeometryCalls:
    def update_vertices(self, vertices, first=0, flags=0):
        """hrpt_update_vertices: new S.VertexQuantized records for the vertices [first, first + len(vertices)) of the scene's vertex buffer;
        the acceleration structure and the per-triangle records follow. flags: S.VERTICES_REFIT (keep the hierarchy of a GPU-built flat
        tree), S.VERTICES_SAME_FRAME (a further range of the same frame: the previous positions render_motion_vectors reads are not
        reset first)."""
        vertices = records(vertices, "VertexQuantized")
        self._check(lib.hrpt_update_vertices(self._h, vertices.ctypes.data if len(vertices) else None, int(first), len(vertices), int(flags)))

    def update_vertices_device(self, ptr, first, count, flags=0, stream=0):
        """hrpt_update_vertices_device: the same from `count` S.VertexFloat records in device memory at `ptr` (16-byte aligned; e.g. a torch
        tensor's data_ptr()), quantised on the device. `stream` (integer handle, 0 = the default stream) is synchronised before they are read."""
        self._check(lib.hrpt_update_vertices_device(self._h, address(ptr), int(first), int(count), int(flags), address(stream)))

    def end_vertex_frame(self):
        """A frame in which nothing deforms: previous positions = current positions, nothing is rebuilt (the count-0 call)."""
        self._check(lib.hrpt_update_vertices(self._h, None, 0, 0, 0))

    def quantize_vertices_device(self, in_ptr, count, out_ptr, stream=0):
        """hrpt_quantize_vertices_device: the quantiser kernel alone, `count` S.VertexFloat records at in_ptr (16-byte aligned) ->
        S.VertexQuantized records at out_ptr, both device addresses; asynchronous on `stream` (integer handle)."""
        self._check(lib.hrpt_quantize_vertices_device(self._h, address(in_ptr), int(count), address(out_ptr), address(stream)))

    def skin_vertices_device(self, base, joints, weights, joint_matrices, deltas, morph_weights, count, joint_count, target_count, out_ptr,
                             status_ptr=0, stream=0):
        """hrpt_skin_vertices_device: the skinning kernel alone. The first six arguments are device addresses (0 = NULL) of the arrays
        skin_arrays() describes, out_ptr that of `count` S.VertexFloat records (16-byte aligned), status_ptr that of two zeroed uint32
        (word 0: an output position is not finite; word 1: a joint index is out of range) or 0. Asynchronous on `stream`."""
        args = _device_skin_args(base, joints, weights, joint_matrices, deltas, morph_weights, count, joint_count, target_count)
        self._check(lib.hrpt_skin_vertices_device(self._h, C.byref(args), address(out_ptr), address(status_ptr), address(stream)))

    def update_vertices_skinned(self, base, joints, weights, joint_matrices, deltas, morph_weights, count, joint_count, target_count, first,
                                flags=0, stream=0):
        """hrpt_update_vertices_skinned: update_vertices_device with the skinning kernel in front of the quantiser, in one call; the same
        device addresses as skin_vertices_device, for the vertices [first, first + count) of the scene."""
        args = _device_skin_args(base, joints, weights, joint_matrices, deltas, morph_weights, count, joint_count, target_count)
        self._check(lib.hrpt_update_vertices_skinned(self._h, C.byref(args), int(first), int(flags), address(stream)))

    def animate(self, animation, flags=0):
        """hrpt_animate: evaluates `animation` (an Animation) at its current times on the device and commits the instances like
        update_instances (S.ANIMATE_REFIT: like refit_instances); S.ANIMATE_NO_COMMIT: node worlds, palette and weights only, asynchronous."""
        self._check(lib.hrpt_animate(self._h, animation._h, int(flags)))

    def animation_device(self, animation):
        """hrpt_get_animation_device: device addresses (palette, weights, node worlds) of the last animate of `animation`; None for an
        empty array."""
        p = [C.c_void_p() for _ in range(3)]
        self._check(lib.hrpt_get_animation_device(self._h, animation._h, *[C.byref(x) for x in p]))
        return tuple(x.value for x in p)

    def read_animation(self, animation):
        """hrpt_read_animation: (palette [joints, 3, 4], weights, node worlds [nodes, 4, 4]) of the last animate (synchronises)."""
        palette = np.zeros((animation.joint_count, 3, 4), np.float32)
        weights = np.zeros(animation.morph_weight_count, np.float32)
        worlds = np.zeros((animation.node_count, 4, 4), np.float32)
        self._check(lib.hrpt_read_animation(self._h, animation._h, palette.ctypes.data, weights.ctypes.data, worlds.ctypes.data))
        return palette, weights, worlds

    def release_animation(self, animation):
        """hrpt_animation_release: drops the context's device copy of `animation`; the next animate uploads it again."""
        self._check(lib.hrpt_animation_release(self._h, animation._h))
