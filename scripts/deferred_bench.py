"""Time of deferred lighting on one MI355X at 1920 x 1080 inside the scenes of config 2 (Cornell box) and config 4
(Sponza-class), one context:

  (a)  hrpt_render_gbuffer, the five planes the stage reads
  (b)  hrpt_deferred_lighting with shadows and sky, per light count (the scene's lights, then 4 and 9 with point and spot lights added)
  (c)  the same without HRPT_DEFERRED_SHADOWS: the two kernels' arithmetic alone
  (d)  hrpt_render at one sample and m_MaxBounces = 1 on the same scene: the path tracer's noisy bounce-0 frame, the comparison

Method: the legs alternate inside every round, ROUNDS rounds after a warm-up; a leg's time is CALLS back-to-back calls between two HIP events
on the context's stream, divided by CALLS; reported: median over the rounds and min..max, the run-to-run spread a difference has to exceed.
Per-kernel times come from a `rocprofv3 --kernel-trace --stats` run of its own over this script.

The byte floor, printed with the measurement: per (pixel, light) pair 48 B of ray record written by deferred_rays and read by the trace, 32 B
of hit record written by the trace (4 B of it read by deferred_shade): 80 B written per pair; per pixel the planes read (depth and normal
twice, albedo, metallic, emissive: 7 x 16 B) and Output written (16 B); between batches 2 x 16 B of running sums written and read; over the
device's memory bandwidth.

    python scripts/deferred_bench.py [--calls 4 --rounds 9 --configs 2,4 --size 1920x1080]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

HBM_BYTES_PER_S = 8.0e12                      # MI355X: 8 TB/s


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
        raise SystemExit("deferred_bench: no GPU; this script measures and does not fall back")
    W, H = (int(v) for v in a.size.split("x"))
    luts = native.precompute_atmosphere()
    stream = torch.cuda.Stream()
    five = sum(1 << p for p in (S.GB_ALBEDO, S.GB_NORMAL, S.GB_GEO_NORMAL, S.GB_EMISSIVE, S.GB_DEPTH))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        e0.record(stream)
        for _ in range(a.calls):
            fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / a.calls            # ms per call

    def run(legs):
        for _, fn in legs:
            timed(fn); timed(fn)
        ms = {name: [] for name, _ in legs}
        for r in range(a.rounds):
            for name, fn in (legs if r % 2 == 0 else legs[::-1]):
                ms[name].append(timed(fn))
        for name, _ in legs:
            t = ms[name]
            print(f"  {name:62s} median {statistics.median(t):8.3f}  min {min(t):8.3f}  max {max(t):8.3f}")
        return ms

    print(f"deferred_bench: {W} x {H}; {a.rounds} rounds x {a.calls} calls per leg, alternating; device ms per call")
    for config in (int(c) for c in a.configs.split(",")):
        if config == 2:
            sc, view, pos, cfg = scenes.config_cornell(luts, W, H, extra_lights=True)
            lo, hi = (-0.8, 0.8, -3.0), (0.8, 1.9, 0.5)
        else:
            sc, view, pos, cfg = scenes.config_sponza_class(luts, W, H)
            lo, hi = (-9.0, 1.0, -4.0), (9.0, 3.5, 4.0)
        ctx = native.PathTracerContext(0)
        ctx.set_stream(stream.cuda_stream)
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        cb = scenes.fill_constants(view, pos, sc, 0, 1)
        rng = np.random.default_rng(5)
        base = np.array(sc.lights, S.GPULight)
        extra = []
        for k in range(9):
            l = np.zeros((), S.GPULight)
            l["m_Type"] = S.LIGHT_POINT if k % 2 else S.LIGHT_SPOT
            l["m_Position"] = [rng.uniform(lo[i], hi[i]) for i in range(3)]
            l["m_Direction"], l["m_Color"], l["m_Intensity"], l["m_Range"] = (0.2, -1.0, 0.1), rng.uniform(0.3, 1.0, 3), 4.0, 0.0
            l["m_SpotInnerConeAngle"], l["m_SpotOuterConeAngle"], l["m_CosSunAngularRadius"] = 0.4, 0.9, 1.0
            extra.append(l[()])
        print(f"config {config}: {len(base)} scene light(s)")
        legs = [("(a) hrpt_render_gbuffer, five planes", lambda: ctx.render_gbuffer(cb, planes=five)),
                ("(d) hrpt_render, one sample, m_MaxBounces = 1", lambda: ctx.render(cb, accum_count=1))]
        run(legs)
        for count in sorted({len(base), 4, 9}):
            ctx.update_lights(np.array(list(base) + extra, S.GPULight)[:max(count, len(base))])
            c = cb.copy(); c["m_LightCount"] = count
            ctx.render_gbuffer(c, planes=five)
            pairs = W * H * count
            floor = (pairs * 80 + W * H * (7 * 16 + 16) + (W * H * 64 * ((count - 1) // 4) if count > 4 else 0)) / HBM_BYTES_PER_S * 1e3
            print(f"  {count} light(s): {pairs} pairs, byte floor {floor:.4f} ms")
            run([(f"(b) hrpt_deferred_lighting, shadows + sky, {count} light(s)", lambda: ctx.deferred_lighting(c, S.DeferredParams(S.DEFERRED_SHADOWS | S.DEFERRED_SKY))),
                 (f"(c) hrpt_deferred_lighting, sky only, {count} light(s)", lambda: ctx.deferred_lighting(c, S.DeferredParams(S.DEFERRED_SKY)))])
            out = ctx.read_output()
            print(f"  Output: mean {out[..., :3].mean():.4f}, finite {bool(np.isfinite(out).all())}")
        ctx.close()


if __name__ == "__main__":
    main()
