"""Time of hrpt_bloom at 1920 x 1080 on one MI355X: one kernel per pass (HRPT_BLOOM_FUSED_TAIL=0) against the fused tail (the levels of
at most N texels in one workgroup's LDS; 8192 = levels 3..5 at this size, 2048 = levels 4..5), next to hrpt_post_process on the same
image and the byte floor of the chain.

Method: one context per variant (the knob is read by hrpt_create), all on one torch stream; a round times CALLS back-to-back calls of one
variant between two HIP events on that stream (device time per call including the gaps between its kernels, which is what the stage
costs a frame); the variants alternate inside every round, ROUNDS rounds after a warm-up; reported: median over the rounds, min..max =
the run-to-run spread a difference has to exceed. Host wall time per call (enqueue only) is printed too: a stage whose enqueue takes longer
than its device time is host-bound in a loop that does nothing else.

    python scripts/bloom_bench.py [--width 1920 --height 1080 --calls 200 --rounds 9]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/bloom_bench.py --rounds 2      (per-kernel durations, a run of its own)
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

HBM_ACHIEVABLE = 6.29e12        # bytes / s, float4 copy on an MI355X (8.0e12 is the specification)


def chain_bytes(width, height):
    """Bytes the passes move when every level is read and written once per pass that touches it (packed 4-byte texels, 16-byte pixels)."""
    n = []
    for i in range(6):
        w, h = (width // 2) >> i, (height // 2) >> i
        if w < 1 or h < 1:
            break
        n.append(w * h)
    if not n:
        return 0, {}
    parts = {"prefilter": 16 * width * height + 4 * n[0],
             "downsamples": sum(4 * n[i - 1] + 4 * n[i] for i in range(1, len(n))),
             "upsamples": sum(4 * n[i + 1] + 8 * n[i] for i in range(len(n) - 1)),
             "composite": 32 * width * height + 4 * n[0]}
    return sum(parts.values()), parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--variants", default="0,8192,2048", help="values of HRPT_BLOOM_FUSED_TAIL to compare")
    a = ap.parse_args()

    import torch
    from hobbyrenderer_amd import native, structs as S
    if not torch.cuda.is_available():
        raise SystemExit("bloom_bench: no GPU; this script measures and does not fall back")

    W, H = a.width, a.height
    rng = np.random.default_rng(1)
    img = np.empty((H, W, 4), np.float32)
    img[..., :3] = (10.0 ** rng.uniform(-3.0, 4.0, (H, W, 3))).astype(np.float32)
    img[..., 3] = 1.0

    stream = torch.cuda.Stream()
    variants = [int(v) for v in a.variants.split(",")]
    ctxs = {}
    for v in variants:
        os.environ["HRPT_BLOOM_FUSED_TAIL"] = str(v)
        c = native.PathTracerContext(0)
        c.set_stream(stream.cuda_stream)
        c.resize(W, H)
        c.write_accumulation(img)
        ctxs[v] = c
    os.environ.pop("HRPT_BLOOM_FUSED_TAIL", None)
    bp = S.BloomParams()
    pp = S.PostParams(1, 1.0, 0.016, 5.0, -7.0, 23.0, 0.0, 0, 80.0)

    # the variants must agree before their times are compared
    outs = []
    for v in variants:
        ctxs[v].resolve_output(); ctxs[v].bloom(bp); outs.append(ctxs[v].read_output())
    for o in outs[1:]:
        assert np.array_equal(o.view(np.uint32), outs[0].view(np.uint32)), "variants differ"

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

    jobs = [(f"bloom tail={v}", (lambda c=ctxs[v]: c.bloom(bp)), ctxs[v]) for v in variants]
    jobs.append(("post_process", (lambda c=ctxs[variants[0]]: c.post_process(pp)), ctxs[variants[0]]))
    for name, fn, c in jobs:                                              # warm-up: code objects, pyramids, display image
        c.resolve_output(); timed(fn, 20)
    dev = {name: [] for name, _, _ in jobs}
    host = {name: [] for name, _, _ in jobs}
    for r in range(a.rounds):
        order = jobs if r % 2 == 0 else jobs[::-1]
        for name, fn, c in order:
            c.resolve_output()                                            # every round starts from the same image
            d, h = timed(fn, a.calls)
            dev[name].append(d); host[name].append(h)

    total, parts = chain_bytes(W, H)
    floor_us = total / HBM_ACHIEVABLE * 1e6
    print(f"bloom_bench {W}x{H}: {a.rounds} rounds x {a.calls} calls per variant, alternating; microseconds per call")
    print(f"byte floor: {total / 1e6:.1f} MB ({', '.join(f'{k} {v / 1e6:.1f}' for k, v in parts.items())}) / {HBM_ACHIEVABLE / 1e12:.2f} TB/s = {floor_us:.1f} us")
    for name, _, _ in jobs:
        d, h = dev[name], host[name]
        med = statistics.median(d)
        line = f"{name:18s} device median {med:7.2f}  min {min(d):7.2f}  max {max(d):7.2f}   host enqueue median {statistics.median(h):7.2f}"
        if name.startswith("bloom"):
            line += f"   floor / median = {floor_us / med:.2f}"
        print(line)
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    main()
