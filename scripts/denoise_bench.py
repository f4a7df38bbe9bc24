"""Time of hrpt_denoise at 1920 x 1080 on one MI355X over config 2's Cornell scene: radius 3, iterations 1 and 3, on a history of age 0 (a
camera cut: the widest kernel) and of age 15 (sixteen static frames), next to hrpt_temporal_accumulate on the same images and the byte floor
of one pass (four 16-byte reads and one or two 16-byte writes per pixel; the taps are gathers the caches serve, or do not).

Method: three contexts on one torch stream (denoise on a fresh history, denoise on an aged history, the temporal stage), each rendered once
and given its motion, depth, normal and geo-normal planes; a round times CALLS back-to-back calls of one variant between two HIP events on
that stream; the variants alternate inside every round, ROUNDS rounds after a warm-up; reported: median over the rounds, min..max = the
run-to-run spread a difference has to exceed. In the default mode every call filters the image the previous one wrote (the ages do not
change), as iterated passes do. Host wall time per call (enqueue only) is printed too.

    python scripts/denoise_bench.py [--width 1920 --height 1080 --calls 100 --rounds 9]
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
        raise SystemExit("denoise_bench: no GPU; this script measures and does not fall back")

    W, H = a.width, a.height
    luts = native.precompute_atmosphere()
    sc, view, pos, cfg = scenes.config_cornell(luts, W, H)
    full = view.copy()
    full["m_CameraDirectionOrPosition"] = (pos[0], pos[1], pos[2], 1.0)
    planes = (1 << S.GB_DEPTH) | (1 << S.GB_NORMAL) | (1 << S.GB_GEO_NORMAL)
    tp = S.TemporalParams(0.9, 0)

    stream = torch.cuda.Stream()
    ctxs = {}
    for name, frames in (("age 0", 1), ("age 15", 16), ("temporal", 1)):
        c = native.PathTracerContext(0)
        c.set_stream(stream.cuda_stream)
        c.upload_scene(sc)
        c.resize(W, H)
        for k in range(frames):
            cb = scenes.fill_constants(view, pos, sc, k, cfg["max_bounces"])
            c.clear_accumulation()
            c.render(cb, accum_count=1)
            if k == 0:
                c.render_motion_vectors(cb, full, planes=planes)
            c.temporal_accumulate(full, full, tp)
        hist = c.read_temporal_history()
        hit = c.read_gbuffer(S.GB_DEPTH)[..., 0] != np.float32(1e10)
        print(f"{name}: {hit.mean() * 100:.1f} % of the pixels hit, median age {np.median(hist[..., 3][hit]):.2f}")
        ctxs[name] = c

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

    jobs = []
    for name in ("age 0", "age 15"):
        for iterations in (1, 3):
            for label, flags in (("", 0), (" output-only", S.DENOISE_OUTPUT_ONLY)):
                if flags and iterations == 3:
                    continue
                p = S.DenoiseParams(radius=3.0, iterations=iterations, frame=11, flags=flags)
                jobs.append((f"denoise x{iterations} {name}{label}", (lambda c=ctxs[name], p=p: c.denoise(full, p)), iterations))
    jobs.append(("temporal_accumulate", (lambda c=ctxs["temporal"]: c.temporal_accumulate(full, full, tp)), 0))
    for name, fn, _ in jobs:                                              # warm-up: code objects, the noise tile, the scratch pair
        timed(fn, 20)
    dev = {name: [] for name, _, _ in jobs}
    host = {name: [] for name, _, _ in jobs}
    for r in range(a.rounds):
        order = jobs if r % 2 == 0 else jobs[::-1]
        for name, fn, _ in order:
            d, h = timed(fn, a.calls)
            dev[name].append(d); host[name].append(h)

    floors = {n: (4 + n) * 16 * W * H / HBM_ACHIEVABLE * 1e6 for n in (1, 2)}
    print(f"denoise_bench {W}x{H} ({os.path.basename(native.LIB_PATH)}): {a.rounds} rounds x {a.calls} calls per variant, alternating; microseconds per call")
    print(f"byte floor of one pass at {HBM_ACHIEVABLE / 1e12:.2f} TB/s: 4 reads + 1 write = 80 B per pixel = {floors[1]:.1f} us; + the colour write = 96 B = {floors[2]:.1f} us")
    for name, _, iterations in jobs:
        d, h = dev[name], host[name]
        med = statistics.median(d)
        line = f"{name:32s} device median {med:8.2f}  min {min(d):8.2f}  max {max(d):8.2f}   host enqueue median {statistics.median(h):7.2f}"
        if iterations:
            floor = floors[1] * (iterations - 1) + floors[2]
            line += f"   byte floor {floor:6.1f} = {floor / med:.3f} of the median"
        print(line)
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    main()
