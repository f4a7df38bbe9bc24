"""Time of hrpt_upscale on one MI355X over config 2's Cornell scene: 960 x 540, 1280 x 720 and 1920 x 1080 frames into a 1920 x 1080 display
image, next to hrpt_temporal_accumulate at 1920 x 1080 (the yardstick of the same kernel class) and the stage's byte floor -- the
compulsory bytes: three render-size 16-byte reads, one display-size history read, two display-size writes; the history taps beyond the
first touch of a texel are served by the caches. Then the headline: the frame chain clear_accumulation + render (one sample per pixel) +
render_motion_vectors (depth plane) + upscale at 960 x 540 -> 1920 x 1080 against clear_accumulation + render at 1920 x 1080.

Method: one context per render size, each rendered once at accumulation index 0 with that index's jitter and given its motion and depth
planes (and the normal plane for the temporal yardstick), all on one torch stream; a round times CALLS back-to-back calls of one variant
between two HIP events on that stream; the variants alternate inside every round, ROUNDS rounds after a warm-up; reported: median over the
rounds, min..max = the run-to-run spread a difference has to exceed. Every upscale call reads the history the previous one wrote
(ping-pong), as a frame loop does. Host wall time per call (enqueue only) is printed too.

Every size is timed through both kernels: upscale_resolve (the nine current-frame taps are global gathers, the default) and
upscale_resolve_staged (they come from an LDS-staged window; a context created with HRPT_UPSCALE_STAGED=1), alternating like the rest.

    python scripts/upscale_bench.py [--display 1920x1080 --calls 100 --rounds 9 --frames 20]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

HBM_ACHIEVABLE = 6.29e12        # bytes / s, float4 copy on an MI355X (8.0e12 is the specification)
TEMPORAL_BYTES_PER_PIXEL = 7 * 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--display", default="1920x1080")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--frames", type=int, default=20, help="frames per round of the headline chains")
    a = ap.parse_args()

    import torch
    from hobbyrenderer_amd import native, scenes, structs as S
    if not torch.cuda.is_available():
        raise SystemExit("upscale_bench: no GPU; this script measures and does not fall back")

    DW, DH = (int(v) for v in a.display.split("x"))
    sizes = [(DW // 2, DH // 2), (DW * 2 // 3, DH * 2 // 3), (DW, DH)]
    luts = native.precompute_atmosphere()
    stream = torch.cuda.Stream()
    planes = (1 << S.GB_DEPTH) | (1 << S.GB_NORMAL)

    ctxs = {}
    for (w, h, staged) in [(w, h, staged) for (w, h) in sizes for staged in (False, True)]:
        sc, view, pos, cfg = scenes.config_cornell(luts, w, h)
        full = view.copy()
        full["m_CameraDirectionOrPosition"] = (pos[0], pos[1], pos[2], 1.0)
        os.environ["HRPT_UPSCALE_STAGED"] = "1" if staged else "0"        # read at hrpt_create
        c = native.PathTracerContext(0)
        c.set_stream(stream.cuda_stream)
        c.upload_scene(sc)
        c.resize(w, h)
        cb = scenes.fill_constants(view, pos, sc, 0, cfg["max_bounces"])
        c.render(cb, accum_count=1)
        c.render_motion_vectors(cb, full, planes=planes)
        ctxs[(w, h, staged)] = dict(ctx=c, full=full, cb=cb, sc=sc, view=view, pos=pos, bounces=cfg["max_bounces"],
                                    params=S.UpscaleParams(jitter=tuple(float(j) for j in cb["m_Jitter"])))
    del os.environ["HRPT_UPSCALE_STAGED"]

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

    def measure(jobs, calls, warm):
        for _, fn in jobs:                                                 # warm-up: code objects, history pair, colour image
            timed(fn, warm)
        dev = {name: [] for name, _ in jobs}
        host = {name: [] for name, _ in jobs}
        for r in range(a.rounds):
            for name, fn in (jobs if r % 2 == 0 else jobs[::-1]):
                d, h = timed(fn, calls)
                dev[name].append(d); host[name].append(h)
        return dev, host

    # ---- the stage ----
    jobs, floors = [], {}
    for (w, h, staged), k in ctxs.items():
        name = f"upscale {w}x{h} -> {DW}x{DH} {'staged' if staged else 'gather'}"
        jobs.append((name, (lambda k=k: k["ctx"].upscale(DW, DH, k["full"], k["full"], k["params"]))))
        floors[name] = (3 * w * h + 3 * DW * DH) * 16
    native_k = ctxs[(DW, DH, False)]
    tp = S.TemporalParams(0.9, S.TEMPORAL_LINEAR)
    jobs.append((f"temporal {DW}x{DH}", (lambda: native_k["ctx"].temporal_accumulate(native_k["full"], native_k["full"], tp))))
    floors[f"temporal {DW}x{DH}"] = TEMPORAL_BYTES_PER_PIXEL * DW * DH
    dev, host = measure(jobs, a.calls, 20)
    print(f"upscale_bench: {a.rounds} rounds x {a.calls} calls per variant, alternating; microseconds per call; byte floor at {HBM_ACHIEVABLE / 1e12:.2f} TB/s")
    for name, _ in jobs:
        d, h = dev[name], host[name]
        med, floor_us = statistics.median(d), floors[name] / HBM_ACHIEVABLE * 1e6
        print(f"{name:41s} device median {med:7.2f}  min {min(d):7.2f}  max {max(d):7.2f}   host enqueue median {statistics.median(h):6.2f}"
              f"   floor {floors[name] / 1e6:6.1f} MB = {floor_us:6.2f} us, floor / median = {floor_us / med:.2f}")

    # ---- the headline: a frame through the chain at half resolution against the native frame ----
    half_k = ctxs[sizes[0] + (False,)]
    index = [1]

    def frame(k, upscale):
        def run():
            i = index[0] = index[0] + 1
            cb = scenes.fill_constants(k["view"], k["pos"], k["sc"], i, k["bounces"])
            c = k["ctx"]
            c.clear_accumulation()
            c.render(cb, accum_count=1)
            if upscale:
                c.render_motion_vectors(cb, k["full"], planes=1 << S.GB_DEPTH)
                c.upscale(DW, DH, k["full"], k["full"], S.UpscaleParams(jitter=tuple(float(j) for j in cb["m_Jitter"])))
        return run

    def part(k, what):
        c = k["ctx"]
        return {"render": lambda: (c.clear_accumulation(), c.render(k["cb"], accum_count=1)),
                "motion": lambda: c.render_motion_vectors(k["cb"], k["full"], planes=1 << S.GB_DEPTH)}[what]
    w, h = sizes[0]
    jobs = [(f"chain {w}x{h} -> {DW}x{DH}: render + motion + upscale", frame(half_k, True)), (f"native {DW}x{DH}: render", frame(native_k, False)),
            (f"  part: render {w}x{h}", part(half_k, "render")), (f"  part: motion + depth {w}x{h}", part(half_k, "motion"))]
    dev, host = measure(jobs, a.frames, 5)
    print(f"headline: config 2 (Cornell, {half_k['bounces']} bounces), one sample per pixel per frame; {a.rounds} rounds x {a.frames} frames, alternating; microseconds per frame")
    for name, _ in jobs:
        d, hh = dev[name], host[name]
        print(f"{name:58s} device median {statistics.median(d):9.2f}  min {min(d):9.2f}  max {max(d):9.2f}   host enqueue median {statistics.median(hh):8.2f}")
    chain, nat = statistics.median(dev[jobs[0][0]]), statistics.median(dev[jobs[1][0]])
    print(f"chain / native = {chain / nat:.3f}  (native / chain = {nat / chain:.2f} x)")
    for k in ctxs.values():
        k["ctx"].close()


if __name__ == "__main__":
    main()
