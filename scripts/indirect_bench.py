"""Time of traced indirect lighting on one MI355X at 1920 x 1080 inside the scenes of config 2 (Cornell box) and
config 4 (Sponza-class), one context:

  (a)  hrpt_render_gbuffer, the five planes the frame reads
  (b)  hrpt_deferred_lighting with shadows and sky
  (c)  hrpt_indirect_lighting with the diffuse lobe only, with the specular lobe only, and with both
  (d)  hrpt_indirect_compose
  (e)  hrpt_render at one sample and the same m_MaxBounces on the same scene: the path tracer's frame, the comparison

Method: the legs alternate inside every round, ROUNDS rounds after a warm-up; a leg's time is CALLS back-to-back calls between two HIP events
on the context's stream, divided by CALLS; reported: median over the rounds and min..max, the run-to-run spread a difference has to exceed.
The three kernels alone (indirect_rays, indirect_resolve, indirect_compose) come from a `rocprofv3 --kernel-trace --stats` run of its own over
this script.

The byte floor, printed with the measurement: per record 48 B of ray written by indirect_rays and read by the trace and 16 B of radiance
written by the trace and read by indirect_resolve; per pixel the four planes read by indirect_rays and again by indirect_resolve (4 x 16 B
each) and the two planes written (2 x 16 B); over the device's memory bandwidth. The traversal in between is the cost, as for deferred
lighting.

    python scripts/indirect_bench.py [--calls 4 --rounds 9 --configs 2,4 --size 1920x1080 --bounces 3]
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
    ap.add_argument("--bounces", type=int, default=3)
    a = ap.parse_args()

    import torch
    from hobbyrenderer_amd import native, scenes, structs as S
    if not torch.cuda.is_available():
        raise SystemExit("indirect_bench: no GPU; this script measures and does not fall back")
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

    print(f"indirect_bench: {W} x {H}, m_MaxBounces {a.bounces}; {a.rounds} rounds x {a.calls} calls per leg, alternating; device ms per call")
    for config in (int(c) for c in a.configs.split(",")):
        if config == 2:
            sc, view, pos, cfg = scenes.config_cornell(luts, W, H, extra_lights=True)
        else:
            sc, view, pos, cfg = scenes.config_sponza_class(luts, W, H)
        ctx = native.PathTracerContext(0)
        ctx.set_stream(stream.cuda_stream)
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        cb = scenes.fill_constants(view, pos, sc, 0, a.bounces)
        ctx.render_gbuffer(cb, planes=five)
        ctx.deferred_lighting(cb)
        both = S.IndirectParams(S.INDIRECT_DIFFUSE | S.INDIRECT_SPECULAR, 1)
        ctx.indirect_lighting(cb, both)
        traced = [int((ctx.read_indirect(k)[..., 3] == 1).sum()) for k in (0, 1)]
        px = W * H
        floor = lambda lobes: (lobes * px * (2 * 48 + 2 * 16) + px * (2 * 4 * 16 + 2 * 16)) / HBM_BYTES_PER_S * 1e3       # noqa: E731
        print(f"config {config}: {len(sc.lights)} light(s); traced records: diffuse {traced[0]}, specular {traced[1]} of {px} each; "
              f"byte floor {floor(1):.4f} ms (one lobe), {floor(2):.4f} ms (both)")
        run([("(a) hrpt_render_gbuffer, five planes", lambda: ctx.render_gbuffer(cb, planes=five)),
             ("(b) hrpt_deferred_lighting, shadows + sky", lambda: ctx.deferred_lighting(cb)),
             ("(c) hrpt_indirect_lighting, diffuse", lambda: ctx.indirect_lighting(cb, S.IndirectParams(S.INDIRECT_DIFFUSE, 1))),
             ("(c) hrpt_indirect_lighting, specular", lambda: ctx.indirect_lighting(cb, S.IndirectParams(S.INDIRECT_SPECULAR, 1))),
             ("(c) hrpt_indirect_lighting, both", lambda: ctx.indirect_lighting(cb, both)),
             ("(d) hrpt_indirect_compose", lambda: ctx.indirect_compose(both)),
             (f"(e) hrpt_render, one sample, m_MaxBounces = {a.bounces}", lambda: ctx.render(cb, accum_count=1))])
        dif, spec = ctx.read_indirect(0), ctx.read_indirect(1)
        print(f"  planes: diffuse mean {dif[..., :3].mean():.4f}, specular mean {spec[..., :3].mean():.4f}, finite {bool(np.isfinite(dif).all() and np.isfinite(spec).all())}")
        ctx.close()


if __name__ == "__main__":
    main()
