"""Time of hrpt_render_motion_vectors at 1920 x 1080 on one MI355X, on config 1 (cube), config 2 (Cornell-class, tree in LDS) and the config-4
stand-in (Sponza-class, ~100 k textured triangles, tree in global memory), wavefront path. Jobs, alternating inside every round:

  (a) hrpt_render_gbuffer(0x3F) through the PARENT commit's library (--parent-library, loaded next to this one through its C ABI) -- and through
      this build, which runs the same kernels;
  (b) hrpt_render_motion_vectors with planeMask 0: motion only;
  (c) hrpt_render_motion_vectors with planeMask 0x3F: the six planes and motion from one traversal.

What the numbers are for: whether (c) < (a) + (b) -- the point of the mask --, and how (b) sits against the byte floor of the front end plus
16 B per pixel. Method as scripts/gbuffer_bench.py: everything on one torch stream; a round times CALLS back-to-back calls of one job between
two HIP events (device time per call including the gaps between its kernels); ROUNDS rounds after a warm-up; median, min..max = the spread a
difference has to exceed. The previous view is a camera a little to the side and every instance has a slightly different m_PrevWorld, so the
motion arithmetic runs on real data; before timing, (b) and (c) must give the same motion plane bit for bit, and (c)'s planes those of (a).

Byte floor of (b): gbuffer_bench's queue bytes of the bounce-0 front end (path record written and read, radiance slot zeroed, hit record
written and read; wf_gbuffer_motion reads the hit record and the sample index, not the ray) + 16 B per pixel for the plane; the table gathers
(64 B instance record, 12 B of indices, 36 B of positions, 48 B of GpuTri or GpuInstance rows per HIT pixel, cached where neighbours share
them) are reported next to it, not inside it. Against 6.29 TB/s (the float4-copy rate profiles/bloom_bench.txt uses).

    python scripts/motion_bench.py --parent-library PATH [--calls 20 --rounds 21] > profiles/motion_bench.txt
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/motion_bench.py --rounds 2 --configs 4       (per-kernel durations, a run of its own)
"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

HBM_ACHIEVABLE = 6.29e12        # bytes / s, float4 copy on an MI355X


class ParentLibrary:
    """hrpt_render_gbuffer through another build of the same ABI (create / upload / resize / set_stream / render_gbuffer / read_gbuffer only)."""

    def __init__(self, path, S):
        self.lib, self.S = C.CDLL(path), S
        L = self.lib
        L.hrpt_create.argtypes = [C.POINTER(S.DeviceDesc), C.POINTER(C.c_void_p)]
        L.hrpt_destroy.argtypes = [C.c_void_p]; L.hrpt_destroy.restype = None
        L.hrpt_upload_scene.argtypes = [C.c_void_p, C.POINTER(S.SceneDesc)]
        L.hrpt_resize.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.hrpt_render_gbuffer.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.hrpt_read_gbuffer.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
        L.hrpt_set_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_int]

    def context(self, scene, width, height, stream):
        h = C.c_void_p()
        desc = self.S.DeviceDesc(0, self.S.ABI_VERSION)
        assert self.lib.hrpt_create(C.byref(desc), C.byref(h)) == 0
        d, keep = scene.desc()
        assert self.lib.hrpt_upload_scene(h, C.byref(d)) == 0
        del keep
        assert self.lib.hrpt_resize(h, width, height) == 0
        assert self.lib.hrpt_set_stream(h, C.c_void_p(int(stream)), 1) == 0
        return h

    def render_gbuffer(self, h, constants, planes):
        p = np.zeros((), self.S.FrameParams)
        p["constants"] = constants; p["accumCount"] = 1; p["stripeCount"] = 1
        assert self.lib.hrpt_render_gbuffer(h, p.ctypes.data, planes) == 0

    def read_gbuffer(self, h, plane, width, height):
        out = np.empty((height, width, 4), np.float32)
        assert self.lib.hrpt_read_gbuffer(h, plane, out.ctypes.data, out.nbytes) == 0
        return out


def with_previous_transforms(scene):
    """Every instance's m_PrevWorld = m_World followed by a small rotation about y and a shift, different per instance."""
    import copy
    out = copy.copy(scene)
    inst = scene.instances.copy()
    for k in range(len(inst)):
        a = 0.01 + 0.002 * (k % 7)
        m = np.array([[math.cos(a), 0, -math.sin(a), 0], [0, 1, 0, 0], [math.sin(a), 0, math.cos(a), 0], [0.01 * (k % 3), 0.004, -0.006, 1]], np.float64)
        inst["m_PrevWorld"][k] = (inst["m_World"][k].astype(np.float64) @ m).astype(np.float32)
    out.instances = inst
    return out


def motion_byte_floor(pixels, path_record_bytes, two_level):
    inst = 4 if two_level else 0
    queue = pixels * (2 * path_record_bytes + 16 + 2 * (16 + inst) + 4)      # raygen + extend, radiance, hit w + r (+ instance), sample index
    return 16 * pixels, queue


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--configs", default="1,2,4")
    ap.add_argument("--parent-library", default=None, help="libhobbyrt_pt.so of the parent commit: its hrpt_render_gbuffer(0x3F) is job (a)")
    a = ap.parse_args()

    import torch
    from hobbyrenderer_amd import native, scenes, structs as S
    if not torch.cuda.is_available():
        raise SystemExit("motion_bench: no GPU; this script measures and does not fall back")
    W, H = a.width, a.height
    luts = native.precompute_atmosphere()
    parent = ParentLibrary(a.parent_library, S) if a.parent_library else None
    stream = torch.cuda.Stream()

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        for _ in range(calls):
            fn()
        e1.record(stream)
        host = time.perf_counter() - t0
        stream.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls, host * 1e6 / calls      # microseconds per call: device, host enqueue

    for config in [int(c) for c in a.configs.split(",")]:
        if config == 1:
            sc = scenes.cube_scene(luts); view, pos = scenes.planar_view(W, H); name = "config 1 (cube, 12 triangles, tree in LDS)"
            prev_view, _ = scenes.planar_view(W, H, position=(0.05, 0.02, -5.05), yaw=0.01)
        elif config == 2:
            sc, view, pos, _ = scenes.config_cornell(luts, W, H); name = "config 2 (Cornell-class, 38 triangles, tree in LDS)"
            prev_view, _ = scenes.planar_view(W, H, position=(0.02, 1.0, -3.43), yaw=0.005, fov_y=math.radians(40.0), aspect=16.0 / 9.0)
        else:
            sc, view, pos, _ = scenes.config_sponza_class(luts, W, H); name = "config-4 stand-in (Sponza-class, textured, tree in global memory)"
            prev_view, _ = scenes.planar_view(W, H, position=(-9.03, 1.7, -0.42), yaw=math.radians(78.3), pitch=math.radians(-3.0), fov_y=math.radians(55.0),
                                              aspect=16.0 / 9.0)
        sc = with_previous_transforms(sc)
        cb = scenes.fill_constants(view, pos, sc, 0, 1)                    # index 0, Halton jitter of the index
        ctx = native.PathTracerContext(0)
        ctx.set_stream(stream.cuda_stream)
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        jobs = [("gbuffer 6 planes (this build)", lambda: ctx.render_gbuffer(cb)),
                ("(b) motion, mask 0", lambda: ctx.render_motion_vectors(cb, prev_view)),
                ("(c) motion, mask 0x3F", lambda: ctx.render_motion_vectors(cb, prev_view, planes=S.GB_ALL_PLANES))]
        ph = None
        if parent:
            ph = parent.context(sc, W, H, stream.cuda_stream)
            jobs.insert(0, ("(a) gbuffer 6 planes, parent", lambda: parent.render_gbuffer(ph, cb, S.GB_ALL_PLANES)))
        # the jobs must agree before their times are compared
        ctx.render_gbuffer(cb); planes = [ctx.read_gbuffer(k) for k in range(S.GB_PLANES)]
        ctx.render_motion_vectors(cb, prev_view); mv0 = ctx.read_motion_vectors()
        ctx.render_motion_vectors(cb, prev_view, planes=S.GB_ALL_PLANES); mv = ctx.read_motion_vectors()
        assert np.array_equal(mv0.view(np.uint32), mv.view(np.uint32)), "motion planes of mask 0 and mask 0x3F differ"
        for k in range(S.GB_PLANES):
            assert np.array_equal(ctx.read_gbuffer(k).view(np.uint32), planes[k].view(np.uint32)), "planes of the motion call differ from hrpt_render_gbuffer's"
        if parent:
            parent.render_gbuffer(ph, cb, S.GB_ALL_PLANES)
            for k in range(S.GB_PLANES):
                assert np.array_equal(parent.read_gbuffer(ph, k, W, H).view(np.uint32), planes[k].view(np.uint32)), "parent planes differ"
        hit = mv[..., 3] == 1
        mag = np.hypot(mv[..., 0], mv[..., 1])[hit]
        for _, fn in jobs:
            timed(fn, 5)                                                    # warm-up: code objects, pools, planes, tables
        dev = {n: [] for n, _ in jobs}; host = {n: [] for n, _ in jobs}
        for r in range(a.rounds):
            for n, fn in (jobs if r % 2 == 0 else jobs[::-1]):
                d, h = timed(fn, a.calls)
                dev[n].append(d); host[n].append(h)
        bi = ctx.build_info()
        print(f"motion_bench {W}x{H}, {name}: {bi.triangleCount} triangles, {len(sc.instances)} instances, {int(hit.sum())} of {W * H} primary rays hit, "
              f"motion {mag.min():.3f} .. {mag.max():.3f} px; {a.rounds} rounds x {a.calls} calls per job, alternating; microseconds per call")
        med = {}
        for n, _ in jobs:
            d = dev[n]; med[n] = statistics.median(d)
            line = f"{n:32s} device median {med[n]:8.2f}  min {min(d):8.2f}  max {max(d):8.2f}   host enqueue median {statistics.median(host[n]):7.2f}"
            if n.startswith("(b)"):
                pb, qb = motion_byte_floor(W * H, 48, bi.structure == S.ACCEL_TWO_LEVEL)
                floor_us = (pb + qb) / HBM_ACHIEVABLE * 1e6
                gather = int(hit.sum()) * (64 + 12 + 36 + 48)
                line += (f"   floor {(pb + qb) / 1e6:.1f} MB (plane {pb / 1e6:.1f} + queues {qb / 1e6:.1f}) = {floor_us:.1f} us, floor / median = {floor_us / med[n]:.2f};"
                         f" table gathers up to {gather / 1e6:.1f} MB uncached")
            print(line)
        ga = "(a) gbuffer 6 planes, parent" if parent else "gbuffer 6 planes (this build)"
        b, c = med["(b) motion, mask 0"], med["(c) motion, mask 0x3F"]
        print(f"(c) = {c:.2f} us against (a) + (b) = {med[ga] + b:.2f} us ({'(a) = the parent library' if parent else '(a) = this build: no parent library given'}); "
              f"(c) - (a) = {c - med[ga]:.2f} us, the price of motion inside the shared pass")
        if parent:
            parent.lib.hrpt_destroy(ph)
        ctx.close()


if __name__ == "__main__":
    main()
