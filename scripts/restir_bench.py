"""Time of resampled direct lighting against all-lights deferred lighting on one MI355X at 1920 x 1080 inside the
scenes of config 2 (Cornell box) and config 4 (Sponza-class), with point and spot lights added up to 9, 64 and 512:

  (a)  hrpt_deferred_lighting with shadows and sky at 9 and 64 lights (its kernels are the parent's: scripts/kernel_diff.py)
  (b)  hrpt_restir_lighting with the documented defaults (8 candidates, 1 neighbour, both reuse passes, shadows, sky) at each light count
  (c)  the same with each reuse flag off in turn, at 64 lights
  (d)  the same on a context created with HRPT_RESTIR_GLOBAL_LIGHTS=1: restir_initial gathers from global memory instead of LDS

The finding to read off: where resampling starts to beat all-lights deferred lighting, and whether its time is flat in the light count.

Method: one stream, the legs alternate inside every round, ROUNDS rounds after a warm-up; a leg's time is CALLS back-to-back calls between
two HIP events on the stream, divided by CALLS; reported: median over the rounds and min..max, the run-to-run spread a difference has to
exceed. Every restir call has a new frameSeed and reuses the previous call's reservoirs. Per-kernel times come from a `rocprofv3
--kernel-trace --stats` run of its own over this script.

The byte floor, printed with the measurement, per pixel: initial reads 4 planes and writes a record (80 B); temporal reads 4 planes, motion,
two records and a key and writes a record (144 B); spatial reads 4 planes and a record for the pixel and for each of k neighbours and writes
a record, a key and a ray (80 (1 + k) + 80 B); the trace reads the ray and writes a hit (80 B); shade reads 5 planes, a record and a hit and
writes Output (144 B); over the device's memory bandwidth. Nothing in it depends on the light count.

    python scripts/restir_bench.py [--calls 4 --rounds 9 --configs 2,4 --size 1920x1080]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

HBM_BYTES_PER_S = 8.0e12                      # MI355X: 8 TB/s
COUNTS = (9, 64, 512)


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
        raise SystemExit("restir_bench: no GPU; this script measures and does not fall back")
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
            print(f"  {name:66s} median {statistics.median(t):8.3f}  min {min(t):8.3f}  max {max(t):8.3f}")

    def context(sc, global_lights):
        if global_lights:
            os.environ["HRPT_RESTIR_GLOBAL_LIGHTS"] = "1"
        else:
            os.environ.pop("HRPT_RESTIR_GLOBAL_LIGHTS", None)
        ctx = native.PathTracerContext(0)                # the knob is read here
        os.environ.pop("HRPT_RESTIR_GLOBAL_LIGHTS", None)
        ctx.set_stream(stream.cuda_stream)
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        return ctx

    seed = [0]

    def restir(ctx, cb, flags=None, **kw):
        def call():
            seed[0] += 1
            p = S.RestirParams(frameSeed=seed[0]) if flags is None else S.RestirParams(flags, seed[0])
            for k, v in kw.items():
                setattr(p, k, v)
            ctx.restir_lighting(cb, p)
        return call

    k = S.RestirParams().spatialSamples
    floor = W * H * (80 + 144 + 80 * (1 + k) + 80 + 80 + 144) / HBM_BYTES_PER_S * 1e3
    print(f"restir_bench: {W} x {H}; {a.rounds} rounds x {a.calls} calls per leg, alternating; device ms per call; byte floor of a restir call {floor:.4f} ms at any light count")
    default = S.RESTIR_SHADOWS | S.RESTIR_SKY | S.RESTIR_TEMPORAL | S.RESTIR_SPATIAL
    for config in (int(c) for c in a.configs.split(",")):
        if config == 2:
            sc, view, pos, cfg = scenes.config_cornell(luts, W, H, extra_lights=True)
            lo, hi = (-0.8, 0.8, -3.0), (0.8, 1.9, 0.5)
        else:
            sc, view, pos, cfg = scenes.config_sponza_class(luts, W, H)
            lo, hi = (-9.0, 1.0, -4.0), (9.0, 3.5, 4.0)
        full = np.array(view, S.PlanarViewConstants)
        full["m_CameraDirectionOrPosition"] = (pos[0], pos[1], pos[2], 1.0)
        cb = scenes.fill_constants(view, pos, sc, 0, 1)
        rng = np.random.default_rng(5)
        base = np.array(sc.lights, S.GPULight)
        extra = []
        for j in range(max(COUNTS)):
            l = np.zeros((), S.GPULight)
            l["m_Type"] = S.LIGHT_POINT if j % 2 else S.LIGHT_SPOT
            l["m_Position"] = [rng.uniform(lo[i], hi[i]) for i in range(3)]
            l["m_Direction"], l["m_Color"], l["m_Intensity"], l["m_Range"] = (0.2, -1.0, 0.1), rng.uniform(0.3, 1.0, 3), 4.0, 0.0
            l["m_SpotInnerConeAngle"], l["m_SpotOuterConeAngle"], l["m_CosSunAngularRadius"] = 0.4, 0.9, 1.0
            extra.append(l[()])
        lights = np.array(list(base) + extra, S.GPULight)[:max(COUNTS)]
        ctx, ctx_global = context(sc, False), context(sc, True)
        print(f"config {config}: {len(base)} scene light(s), point and spot lights added up to {max(COUNTS)}")
        for c in (ctx, ctx_global):
            c.update_lights(lights)
            c.render_motion_vectors(cb, full, planes=five)
        for count in COUNTS:
            c = cb.copy(); c["m_LightCount"] = count
            legs = []
            if count <= 64:
                legs.append((f"(a) hrpt_deferred_lighting, shadows + sky, {count} lights", lambda c=c: ctx.deferred_lighting(c, S.DeferredParams(S.DEFERRED_SHADOWS | S.DEFERRED_SKY))))
            legs.append((f"(b) hrpt_restir_lighting, defaults, {count} lights", restir(ctx, c)))
            legs.append((f"(d) the same, restir_initial from global memory, {count} lights", restir(ctx_global, c)))
            if count == 64:
                legs.append((f"(c) without HRPT_RESTIR_TEMPORAL, {count} lights", restir(ctx, c, default & ~S.RESTIR_TEMPORAL)))
                legs.append((f"(c) without HRPT_RESTIR_SPATIAL, {count} lights", restir(ctx, c, default & ~S.RESTIR_SPATIAL)))
                legs.append((f"(c) without either, {count} lights", restir(ctx, c, default & ~S.RESTIR_SPATIAL & ~S.RESTIR_TEMPORAL)))
                legs.append((f"(b') 32 candidates, {count} lights", restir(ctx, c, default, candidates=32)))
            run(legs)
            ctx.restir_lighting(c, S.RestirParams(frameSeed=1))
            out, res = ctx.read_output(), ctx.read_restir_reservoirs()
            print(f"  Output: mean {out[..., :3].mean():.4f}, finite {bool(np.isfinite(out).all())}; non-empty reservoirs {float((res['light'] != S.RESTIR_EMPTY).mean()):.3f}, mean M {float(res['M'].mean()):.1f}")
        ctx.close(); ctx_global.close()


if __name__ == "__main__":
    main()
