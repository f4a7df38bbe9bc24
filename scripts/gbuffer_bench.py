"""Time of hrpt_render_gbuffer at 1920 x 1080 on one MI355X, on config 2 (Cornell-class, tree in LDS) and the config-4 stand-in (Sponza-class,
~100 k textured triangles, tree in global memory): all six planes and albedo + normal only, wavefront path (and, for orientation, the
validation kernel), next to the nearest existing work -- hrpt_render with accumCount = 1, m_MaxBounces = 1: the same front end plus shade,
shadow and resolve -- and to the byte floor of the call.

Method (as scripts/bloom_bench.py): everything on one torch stream; a round times CALLS back-to-back calls of one job between two HIP events
on that stream (device time per call including the gaps between its kernels); the jobs alternate inside every round, ROUNDS rounds after a
warm-up; reported: median over the rounds, min..max = the run-to-run spread a difference has to exceed. With --parent-library the 1-bounce
render also runs through that build of the library (the parent commit's libhobbyrt_pt.so, loaded next to this one through its C ABI), in the
same rounds on the same box.

Byte floor: 16 B x planes x pixels written + the bounce-0 queue bytes (path record written by wf_raygen and read by wf_extend, radiance slot
zeroed, hit record written and read, ray + sample index + hit read by wf_gbuffer), against 6.29 TB/s (the float4-copy rate profiles/bloom_bench.txt uses).

    python scripts/gbuffer_bench.py [--calls 20 --rounds 21] [--parent-library PATH]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/gbuffer_bench.py --rounds 2          (per-kernel durations, a run of its own)
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

HBM_ACHIEVABLE = 6.29e12        # bytes / s, float4 copy on an MI355X


class ParentLibrary:
    """hrpt_render through another build of the same ABI (create / upload / resize / set_stream / render only)."""

    def __init__(self, path, S):
        self.lib, self.S = C.CDLL(path), S
        L = self.lib
        L.hrpt_create.argtypes = [C.POINTER(S.DeviceDesc), C.POINTER(C.c_void_p)]
        L.hrpt_destroy.argtypes = [C.c_void_p]; L.hrpt_destroy.restype = None
        L.hrpt_upload_scene.argtypes = [C.c_void_p, C.POINTER(S.SceneDesc)]
        L.hrpt_resize.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.hrpt_render.argtypes = [C.c_void_p, C.c_void_p]
        L.hrpt_set_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.hrpt_read_accumulation.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]

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

    def render(self, h, constants):
        p = np.zeros((), self.S.FrameParams)
        p["constants"] = constants; p["accumCount"] = 1; p["stripeCount"] = 1
        assert self.lib.hrpt_render(h, p.ctypes.data) == 0

    def read_accumulation(self, h, width, height):
        out = np.empty((height, width, 4), np.float32)
        assert self.lib.hrpt_read_accumulation(h, out.ctypes.data, out.nbytes) == 0
        return out


def byte_floor(pixels, planes, path_record_bytes, two_level):
    inst = 4 if two_level else 0
    queue = pixels * (2 * path_record_bytes + 16 + 2 * (16 + inst) + (32 + 4 + 16 + inst))    # raygen + extend, radiance, hit w + r, wf_gbuffer reads
    return 16 * planes * pixels, queue


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--parent-library", default=None, help="libhobbyrt_pt.so of the parent commit: its 1-bounce hrpt_render is timed in the same rounds")
    a = ap.parse_args()

    import torch
    from hobbyrenderer_amd import native, scenes, structs as S
    if not torch.cuda.is_available():
        raise SystemExit("gbuffer_bench: no GPU; this script measures and does not fall back")
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
        if config == 2:
            sc, view, pos, _ = scenes.config_cornell(luts, W, H); name = "config 2 (Cornell-class, 38 triangles, tree in LDS)"
        else:
            sc, view, pos, _ = scenes.config_sponza_class(luts, W, H); name = "config-4 stand-in (Sponza-class, textured, tree in global memory)"
        cb = scenes.fill_constants(view, pos, sc, 0, 1)                    # index 0, one bounce, Halton jitter of the index
        ctx = native.PathTracerContext(0)
        ctx.set_stream(stream.cuda_stream)
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        two = (1 << S.GB_ALBEDO) | (1 << S.GB_NORMAL)
        jobs = [("gbuffer 6 planes", lambda: ctx.render_gbuffer(cb)),
                ("gbuffer albedo+normal", lambda: ctx.render_gbuffer(cb, planes=two)),
                ("gbuffer 6 planes, megakernel", lambda: ctx.render_gbuffer(cb, flags=S.FRAME_MEGAKERNEL)),
                ("render 1 spp 1 bounce", lambda: ctx.render(cb, accum_count=1))]
        ph = None
        if parent:
            ph = parent.context(sc, W, H, stream.cuda_stream)
            jobs.append(("render 1 spp 1 bounce, parent", lambda: parent.render(ph, cb)))
        # the paths must agree before their times are compared
        ctx.render_gbuffer(cb); wf = [ctx.read_gbuffer(k) for k in range(S.GB_PLANES)]
        ctx.render_gbuffer(cb, flags=S.FRAME_MEGAKERNEL)
        for k in range(S.GB_PLANES):
            assert np.array_equal(ctx.read_gbuffer(k).view(np.uint32), wf[k].view(np.uint32)), "wavefront and megakernel planes differ"
        ctx.render(cb, accum_count=1)
        if parent:
            parent.render(ph, cb)
            assert np.array_equal(parent.read_accumulation(ph, W, H).view(np.uint32), ctx.read_accumulation().view(np.uint32)), "parent render differs"
        hits = int((wf[S.GB_IDS][..., 3] & S.GB_FLAG_HIT).sum())
        for _, fn in jobs:
            timed(fn, 5)                                                    # warm-up: code objects, pools, planes
        dev = {n: [] for n, _ in jobs}; host = {n: [] for n, _ in jobs}
        for r in range(a.rounds):
            for n, fn in (jobs if r % 2 == 0 else jobs[::-1]):
                d, h = timed(fn, a.calls)
                dev[n].append(d); host[n].append(h)
        bi = ctx.build_info()
        print(f"gbuffer_bench {W}x{H}, {name}: {bi.triangleCount} triangles, {hits} of {W * H} primary rays hit; {a.rounds} rounds x {a.calls} calls per job, alternating; microseconds per call")
        for n, _ in jobs:
            d = dev[n]; med = statistics.median(d)
            line = f"{n:32s} device median {med:8.2f}  min {min(d):8.2f}  max {max(d):8.2f}   host enqueue median {statistics.median(host[n]):7.2f}"
            if n.startswith("gbuffer") and "megakernel" not in n:
                planes = 6 if "6" in n else 2
                pb, qb = byte_floor(W * H, planes, 48, bi.structure == S.ACCEL_TWO_LEVEL)
                floor_us = (pb + qb) / HBM_ACHIEVABLE * 1e6
                line += f"   floor {(pb + qb) / 1e6:.1f} MB (planes {pb / 1e6:.1f} + queues {qb / 1e6:.1f}) = {floor_us:.1f} us, floor / median = {floor_us / med:.2f}"
            print(line)
        if parent:
            parent.lib.hrpt_destroy(ph)
        ctx.close()


if __name__ == "__main__":
    main()
