"""Time of the demodulate and compose stages at 1920 x 1080 on one MI355X over config 2's Cornell scene, next to hrpt_denoise (radius 3, one
pass, on a history of age 0) on the same images in the same run, and the byte floor of each: demodulate reads six float4 and writes two per
pixel (128 B), compose reads three and writes one (64 B).

Method: one context on one torch stream, rendered once and given its motion vectors and the five planes the stages read, then one temporal
call so that the denoise stage has its history. The two stages are timed through the _device calls from the context's own Output and planes
into scratch images, so that every call sees the same inputs (the in-place context calls would divide or multiply the same image again
and again); the in-place pair hrpt_demodulate + hrpt_compose, which returns Output to where it was up to rounding, is timed as one job
next to them. A round times CALLS back-to-back calls of one job between two HIP events on that stream; the jobs alternate inside every
round, ROUNDS rounds after a warm-up; reported: median over the rounds, min..max = the run-to-run spread a difference has to exceed.
Host wall time per call (enqueue only) is printed too.

    python scripts/modulation_bench.py [--width 1920 --height 1080 --calls 100 --rounds 9]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

HBM_ACHIEVABLE = 6.29e12        # bytes / s, float4 copy on an MI355X (8.0e12 is the specification)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()

    import torch
    from hobbyrenderer_amd import native, scenes, structs as S
    if not torch.cuda.is_available():
        raise SystemExit("modulation_bench: no GPU; this script measures and does not fall back")

    W, H = a.width, a.height
    luts = native.precompute_atmosphere()
    sc, view, pos, cfg = scenes.config_cornell(luts, W, H)
    full = view.copy()
    full["m_CameraDirectionOrPosition"] = (pos[0], pos[1], pos[2], 1.0)
    needed = (S.GB_ALBEDO, S.GB_NORMAL, S.GB_GEO_NORMAL, S.GB_EMISSIVE, S.GB_DEPTH)

    stream = torch.cuda.Stream()
    c = native.PathTracerContext(0)
    c.set_stream(stream.cuda_stream)
    c.upload_scene(sc)
    c.resize(W, H)
    cb = scenes.fill_constants(view, pos, sc, 0, cfg["max_bounces"])
    c.clear_accumulation()
    c.render(cb, accum_count=1)
    c.render_motion_vectors(cb, full, planes=sum(1 << k for k in needed))
    c.temporal_accumulate(full, full, S.TemporalParams(0.9, 0))
    hit = c.read_gbuffer(S.GB_DEPTH)[..., 0] != np.float32(1e10)
    print(f"{hit.mean() * 100:.1f} % of the pixels hit")

    with torch.cuda.stream(stream):
        scratch = [torch.zeros((H, W, 4), device="cuda:0") for _ in range(3)]
    output = c.device_images()[1]
    g = {k: c.gbuffer_device(k) for k in needed}
    dem = S.DemodulateImages(output, g[S.GB_ALBEDO], g[S.GB_NORMAL], g[S.GB_GEO_NORMAL], g[S.GB_DEPTH], g[S.GB_EMISSIVE], scratch[0].data_ptr(),
                             scratch[1].data_ptr())
    com = S.ComposeImages(scratch[0].data_ptr(), scratch[1].data_ptr(), g[S.GB_EMISSIVE], scratch[2].data_ptr())
    mp = S.ModulationParams()
    dp = S.DenoiseParams(radius=3.0, iterations=1, frame=11, flags=S.DENOISE_OUTPUT_ONLY)

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

    def pair():
        c.demodulate(full, mp)
        c.compose()

    jobs = [("demodulate", lambda: c.demodulate_device(dem, W, H, full, mp, stream.cuda_stream), 128),
            ("compose", lambda: c.compose_device(com, W, H, stream.cuda_stream), 64),
            ("demodulate + compose, in place", pair, 192),
            ("denoise x1 age 0 output-only", lambda: c.denoise(full, dp), 96)]
    for name, fn, _ in jobs:                                              # warm-up: code objects, the noise tile, the scratch images
        timed(fn, 20)
    dev = {name: [] for name, _, _ in jobs}
    host = {name: [] for name, _, _ in jobs}
    for r in range(a.rounds):
        order = jobs if r % 2 == 0 else jobs[::-1]
        for name, fn, _ in order:
            d, h = timed(fn, a.calls)
            dev[name].append(d); host[name].append(h)

    print(f"modulation_bench {W}x{H} ({os.path.basename(native.LIB_PATH)}): {a.rounds} rounds x {a.calls} calls per job, alternating; microseconds per call")
    for name, _, bytes_per_pixel in jobs:
        d, h = dev[name], host[name]
        med = statistics.median(d)
        floor = bytes_per_pixel * W * H / HBM_ACHIEVABLE * 1e6
        print(f"{name:32s} device median {med:8.2f}  min {min(d):8.2f}  max {max(d):8.2f}   host enqueue median {statistics.median(h):7.2f}"
              f"   byte floor ({bytes_per_pixel} B per pixel at {HBM_ACHIEVABLE / 1e12:.2f} TB/s) {floor:6.1f} = {floor / med:.3f} of the median")
    c.close()


if __name__ == "__main__":
    main()
