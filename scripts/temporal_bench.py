"""Time of hrpt_temporal_accumulate at 1920 x 1080 on one MI355X over config 2's Cornell scene: both colour spaces, a static and a moving
camera, next to hrpt_post_process on the same image and the stage's byte floor (five 16-byte reads and two 16-byte writes per pixel; the
history taps beyond the first touch of a texel are served by the caches).

Method: two contexts (static camera: prevView == view; moving camera: last frame's view yawed by 0.02 rad, some 30 px of motion), each rendered
once and given its motion, depth and normal planes, both on one torch stream; a round times CALLS back-to-back calls of one variant between
two HIP events on that stream; the variants alternate inside every round, ROUNDS rounds after a warm-up; reported: median over the rounds,
min..max = the run-to-run spread a difference has to exceed. Every call reads the history the previous one wrote (ping-pong) and blends
into Output in place, as a frame loop does. Host wall time per call (enqueue only) is printed too.

    python scripts/temporal_bench.py [--width 1920 --height 1080 --calls 100 --rounds 9]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

HBM_ACHIEVABLE = 6.29e12        # bytes / s, float4 copy on an MI355X (8.0e12 is the specification)
BYTES_PER_PIXEL = 7 * 16        # colour, motion, depth, normal, history in; history, colour out


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
        raise SystemExit("temporal_bench: no GPU; this script measures and does not fall back")

    W, H = a.width, a.height
    luts = native.precompute_atmosphere()
    sc, view, pos, cfg = scenes.config_cornell(luts, W, H)
    full = view.copy()
    full["m_CameraDirectionOrPosition"] = (pos[0], pos[1], pos[2], 1.0)
    moved, mpos = scenes.planar_view(W, H, position=(0.0, 1.0, -3.4), yaw=0.02, fov_y=np.radians(40.0), aspect=16.0 / 9.0)
    moved["m_CameraDirectionOrPosition"] = (mpos[0], mpos[1], mpos[2], 1.0)
    planes = (1 << S.GB_DEPTH) | (1 << S.GB_NORMAL)

    stream = torch.cuda.Stream()
    ctxs = {}
    for name, prev in (("static", full), ("moving", moved)):
        c = native.PathTracerContext(0)
        c.set_stream(stream.cuda_stream)
        c.upload_scene(sc)
        c.resize(W, H)
        cb = scenes.fill_constants(view, pos, sc, 0, cfg["max_bounces"])
        c.render(cb, accum_count=1)
        c.render_motion_vectors(cb, prev, planes=planes)
        mv = c.read_motion_vectors()
        hit = mv[..., 3] == 1
        print(f"{name} camera: {hit.mean() * 100:.1f} % of the pixels hit, motion median {np.median(np.hypot(mv[..., 0], mv[..., 1])[hit]):.2f} px")
        ctxs[name] = (c, prev)
    pp = S.PostParams(1, 1.0, 0.016, 5.0, -7.0, 23.0, 0.0, 0, 80.0)

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
    for name, (c, prev) in ctxs.items():
        for space, flags in (("linear", S.TEMPORAL_LINEAR), ("log", 0)):
            p = S.TemporalParams(0.9, flags)
            jobs.append((f"temporal {name} {space}", (lambda c=c, prev=prev, p=p: c.temporal_accumulate(full, prev, p)), c))
    jobs.append(("post_process", (lambda c=ctxs["static"][0]: c.post_process(pp)), ctxs["static"][0]))
    for name, fn, c in jobs:                                              # warm-up: code objects, history pair, display image
        c.resolve_output(); timed(fn, 20)
    dev = {name: [] for name, _, _ in jobs}
    host = {name: [] for name, _, _ in jobs}
    for r in range(a.rounds):
        order = jobs if r % 2 == 0 else jobs[::-1]
        for name, fn, c in order:
            c.resolve_output()                                            # every round starts from the same image
            d, h = timed(fn, a.calls)
            dev[name].append(d); host[name].append(h)

    total = BYTES_PER_PIXEL * W * H
    floor_us = total / HBM_ACHIEVABLE * 1e6
    print(f"temporal_bench {W}x{H}: {a.rounds} rounds x {a.calls} calls per variant, alternating; microseconds per call")
    print(f"byte floor: {BYTES_PER_PIXEL} B per pixel = {total / 1e6:.1f} MB / {HBM_ACHIEVABLE / 1e12:.2f} TB/s = {floor_us:.1f} us")
    for name, _, _ in jobs:
        d, h = dev[name], host[name]
        med = statistics.median(d)
        line = f"{name:24s} device median {med:7.2f}  min {min(d):7.2f}  max {max(d):7.2f}   host enqueue median {statistics.median(h):7.2f}"
        if name.startswith("temporal"):
            line += f"   floor / median = {floor_us / med:.2f}"
        print(line)
    for c, _ in ctxs.values():
        c.close()


if __name__ == "__main__":
    main()
