"""Time of hrpt_trace_radiance on one MI355X next to hrpt_render, on config 2 (Cornell box, 4 bounces) and config 4 (Sponza-class, 8 bounces)
at BASELINE.json's 1920 x 1080, one accumulation index per call:

  (a)  hrpt_render, default plan                      (config 2: fused primary rays and fused bounce 0)
  (b)  hrpt_render with HRPT_WF_FUSED_PRIMARY=0       (wf_raygen + the kernels every bounce runs: what (c) runs between its two ends)
  (c)  hrpt_trace_radiance, the same camera rays as device records in the render's sample order (8 x 8 pixel tiles), on the context of (b)
  (c2) the same call on the context of (a)
  (c3) the same records in row-major pixel order (a wave gets a 64 x 1 strip instead of an 8 x 8 tile)
  (d)  the same records in a random permutation
  (e)  as many random probe rays from the scene's interior (uniform origins, uniform directions)

(c) differs from (b) by a 48-byte read per ray in its raygen pass, a 16-byte store per ray at the end, and no Accumulation / Output
traffic; (d) and (e) are incoherent full paths. Before anything is timed the script checks that (c3) and (d) give the bits of the render's
Accumulation for the index.

Two contexts (default, HRPT_WF_FUSED_PRIMARY=0) share one torch stream, and each has a shadow stream of its own for the wf_shadow / wf_extend
overlap. Which hardware queue the runtime gives such a stream is not the library's choice: when one lands on the main stream's queue that
context loses the overlap, renders and radiance calls alike. So every comparison is made within ONE context -- (b), (c), (c3), (d), (e) on
the second, (a) and (c2) on the first -- and a difference between (c) and (c2) is the difference between the two contexts.

Method: the legs alternate inside every round, ROUNDS rounds after a warm-up; a leg's time is CALLS back-to-back calls between two HIP
events on that stream, divided by CALLS; reported: median over the rounds and min..max, the run-to-run spread a difference has to exceed;
paths/s = 1920 * 1080 / median.

    python scripts/radiance_bench.py [--size 1920x1080 --calls 4 --rounds 9 --configs 2,4]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

f32 = np.float32


def pcg_hash(seed):
    state = (seed.astype(np.uint64) * 747796405 + 2891336453) & 0xFFFFFFFF
    word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & 0xFFFFFFFF
    return ((word >> 22) ^ word).astype(np.uint32)


def camera_rays(S, cb, w, h):
    """The primary rays of PathTracer.hlsl:61-72 for `cb`, binary32 operation by operation, as S.Ray records in pixel order."""
    view = cb["m_View"]
    M = np.asarray(view["m_MatClipToWorldNoOffset"], f32)
    px = np.broadcast_to(np.arange(w, dtype=np.uint32)[None, :], (h, w))
    py = np.broadcast_to(np.arange(h, dtype=np.uint32)[:, None], (h, w))
    u = ((px.astype(f32) + f32(0.5)) + f32(cb["m_Jitter"][0])) * f32(view["m_ViewportSizeInv"][0])
    v = ((py.astype(f32) + f32(0.5)) + f32(cb["m_Jitter"][1])) * f32(view["m_ViewportSizeInv"][1])
    cx, cy = u * f32(2.0) + f32(-1.0), v * f32(-2.0) + f32(1.0)
    e = [((cx * M[0, k] + cy * M[1, k]) + f32(0.9) * M[2, k]) + f32(1.0) * M[3, k] for k in range(4)]
    o = np.asarray(cb["m_CameraPos"], f32)[:3]
    d = np.stack([e[0] / e[3], e[1] / e[3], e[2] / e[3]], -1) - o
    d = d * (f32(1.0) / np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]))[..., None]
    rays = np.zeros(w * h, S.Ray)
    rays["origin"] = o; rays["direction"] = d.reshape(-1, 3).astype(f32); rays["tmax"] = f32(1e10)
    index = np.uint64(int(cb["m_AccumulationIndex"]))
    rays["rng"] = pcg_hash(((px.astype(np.uint64) + py.astype(np.uint64) * 65536 + index * 6700417) & 0xFFFFFFFF).reshape(-1))
    return rays


def probe_rays(S, rng, n, lo, hi):
    rays = np.zeros(n, S.Ray)
    rays["origin"] = rng.uniform(lo, hi, (n, 3)).astype(f32)
    d = rng.normal(size=(n, 3))
    rays["direction"] = (d / np.sqrt((d * d).sum(1, keepdims=True))).astype(f32)
    rays["tmin"] = f32(1e-4); rays["tmax"] = f32(1e10)
    rays["rng"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--configs", default="2,4")
    a = ap.parse_args()

    import torch
    from hobbyrenderer_amd import native, scenes, structs as S
    if not torch.cuda.is_available():
        raise SystemExit("radiance_bench: no GPU; this script measures and does not fall back")
    W, H = (int(v) for v in a.size.split("x"))
    n = W * H
    luts = native.precompute_atmosphere()
    stream = torch.cuda.Stream()
    index = 3

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        e0.record(stream)
        for _ in range(a.calls):
            fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / a.calls            # ms per call

    print(f"radiance_bench: {W} x {H} = {n} paths per call, one accumulation index; {a.rounds} rounds x {a.calls} calls per leg, alternating; device ms per call")
    for config in (int(c) for c in a.configs.split(",")):
        if config == 2:
            sc, view, pos, cfg = scenes.config_cornell(luts, W, H)
            bounces, lo, hi = 4, (-0.9, 0.1, -3.9), (0.9, 1.9, 0.9)
        else:
            sc, view, pos, cfg = scenes.config_sponza_class(luts, W, H)
            bounces, lo, hi = 8, (-10.0, 0.3, -5.0), (10.0, 3.5, 5.0)
        cb = scenes.fill_constants(view, pos, sc, index, bounces)
        ctxs = {}
        for name, fused in (("default", "1"), ("unfused", "0")):
            os.environ["HRPT_WF_FUSED_PRIMARY"] = fused          # read at hrpt_create
            c = native.PathTracerContext(0)
            c.set_stream(stream.cuda_stream)
            c.upload_scene(sc)
            c.resize(W, H)
            ctxs[name] = c
        del os.environ["HRPT_WF_FUSED_PRIMARY"]
        cam = camera_rays(S, cb, W, H)
        rng = np.random.default_rng(11)
        perm = rng.permutation(n)
        p = np.arange(n)                                             # sample -> pixel of a render: 8 x 8 tiles, row-major over the image (W, H multiples of 8)
        tiles = (p >> 6) % (W // 8) * 8 + (p & 7) + ((p >> 6) // (W // 8) * 8 + ((p & 63) >> 3)) * W
        with torch.cuda.stream(stream):
            d_cam = torch.from_numpy(cam.view(np.uint8).copy()).to("cuda:0")
            d_tiles = torch.from_numpy(cam[tiles].view(np.uint8).copy()).to("cuda:0")
            d_perm = torch.from_numpy(cam[perm].view(np.uint8).copy()).to("cuda:0")
            d_probe = torch.from_numpy(probe_rays(S, rng, n, lo, hi).view(np.uint8).copy()).to("cuda:0")
            d_out = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
        stream.synchronize()
        c = ctxs["unfused"]            # the radiance legs run on the context of leg (b): same scene copy, same streams, same kernels in between

        # the radiance legs compute what the render computes
        c.clear_accumulation(); c.render(cb, accum_count=1)
        want = c.read_accumulation().reshape(-1, 4).view(np.uint32)
        same = []
        for rays, order in ((d_cam, None), (d_perm, perm)):
            c.trace_radiance_device(rays.data_ptr(), d_out.data_ptr(), n, cb)
            c.synchronize()
            got = d_out.cpu().numpy().view(np.uint32)
            same.append(bool(np.array_equal(got, want if order is None else want[order])))
        print(f"config {config}: {bounces} bounces, {len(sc.lights)} light(s); camera rays through hrpt_trace_radiance == the render's Accumulation, bit for bit: "
              f"pixel order {same[0]}, permuted {same[1]}")

        def render(ctx):
            return lambda: ctx.render(cb, accum_count=1)

        def radiance(rays, ctx=c):
            return lambda: ctx.trace_radiance_device(rays.data_ptr(), d_out.data_ptr(), n, cb)
        legs = [("(a)  hrpt_render, default plan", render(ctxs["default"])), ("(b)  hrpt_render, HRPT_WF_FUSED_PRIMARY=0", render(ctxs["unfused"])),
                ("(c)  hrpt_trace_radiance, camera rays, 8x8 tiles", radiance(d_tiles)),
                ("(c2) ... on the context of (a)", radiance(d_tiles, ctxs["default"])),
                ("(c3) hrpt_trace_radiance, camera rays, row-major", radiance(d_cam)),
                ("(d)  hrpt_trace_radiance, camera rays permuted", radiance(d_perm)),
                ("(e)  hrpt_trace_radiance, interior probe rays", radiance(d_probe))]
        for _, fn in legs:
            timed(fn); timed(fn)
        ms = {name: [] for name, _ in legs}
        for r in range(a.rounds):
            for name, fn in (legs if r % 2 == 0 else legs[::-1]):
                ms[name].append(timed(fn))
        for name, _ in legs:
            t = ms[name]
            med = statistics.median(t)
            print(f"  {name:48s} median {med:8.3f}  min {min(t):8.3f}  max {max(t):8.3f}   {n / med / 1e3:9.1f} M paths/s")
        b, cc = statistics.median(ms[legs[1][0]]), statistics.median(ms[legs[2][0]])
        spread = max(ms[legs[1][0]]) - min(ms[legs[1][0]])
        a_, c2 = statistics.median(ms[legs[0][0]]), statistics.median(ms[legs[3][0]])
        print(f"  (c) - (b) = {cc - b:+.3f} ms = {100 * (cc - b) / b:+.1f} %; run-to-run spread of (b): {spread:.3f} ms = {100 * spread / b:.1f} %;"
              f" (c2) - (a) = {c2 - a_:+.3f} ms; (c2) - (c) = {c2 - cc:+.3f} ms between the contexts")
        for ctx in ctxs.values():
            ctx.close()


if __name__ == "__main__":
    main()
