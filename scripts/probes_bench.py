"""Time of the irradiance probe volume on one MI355X: a volume of 16 x 8 x 16 = 2 048 probes with 256 rays each
(524 288 rays per update) inside the scenes of config 2 (Cornell box, 4 bounces) and config 4 (Sponza-class, 8 bounces), one context:

  (a)  hrpt_trace_radiance + hrpt_trace_rays on the volume's own ray records as device arrays: what a host could do before the stage existed
  (b)  hrpt_probes_update: ray generation, the same two trace calls, the blend
  (b) - (a) is the cost of ray generation plus blend
  (c)  hrpt_probes_shade_gbuffer at 1920 x 1080 next to hrpt_demodulate on the same planes (the other full-screen pass that reconstructs
       the world position and the view vector per pixel)

Method: the legs alternate inside every round, ROUNDS rounds after a warm-up; a leg's time is CALLS back-to-back calls between two HIP events
on the context's stream, divided by CALLS; reported: median over the rounds and min..max, the run-to-run spread a difference has to exceed.
Per-kernel times come from a `rocprofv3 --kernel-trace --stats` run of its own over this script.

Two floors for probes_blend, printed with the measurement:
  bytes    radiance 16 B + hits 32 B per ray read, the atlases (3 KiB per probe) read and written, over the device's memory bandwidth
  weights  every one of the 232 interior texels of a probe evaluates a weight for every ray: P * 232 * N evaluations. A distance weight is a
           dot product, hrt_pow (hrt_log2: 31 operations, one multiply, hrt_exp2: 22) and three multiply-adds; an irradiance weight a dot
           product, a max and four multiply-adds (counted in pt_probes.h / detmath.h; OPS_* below), over the device's binary32 lane rate.

    python scripts/probes_bench.py [--calls 4 --rounds 9 --configs 2,4 --size 1920x1080]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

COUNTS, RAYS = (16, 8, 16), 256
OPS_DISTANCE = 6 + 31 + 1 + 22 + 2 + 6        # dot and max, log2, exponent multiply, exp2, the two tests, d * d and three multiply-adds
OPS_IRRADIANCE = 6 + 2 + 8                    # dot and max, the two tests, four multiply-adds
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
        raise SystemExit("probes_bench: no GPU; this script measures and does not fall back")
    W, H = (int(v) for v in a.size.split("x"))
    luts = native.precompute_atmosphere()
    stream = torch.cuda.Stream()
    props = torch.cuda.get_device_properties(0)
    cus = int(props.multi_processor_count)
    ghz = float(getattr(props, "clock_rate", 2400000)) / 1e6
    lane_rate = cus * 64 * ghz * 1e9                                   # binary32 operations per second, one per lane and clock
    P = COUNTS[0] * COUNTS[1] * COUNTS[2]
    n = P * RAYS

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        e0.record(stream)
        for _ in range(a.calls):
            fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / a.calls            # ms per call

    def report(ms, legs):
        for name, _ in legs:
            t = ms[name]
            print(f"  {name:62s} median {statistics.median(t):8.3f}  min {min(t):8.3f}  max {max(t):8.3f}")

    def run(legs):
        for _, fn in legs:
            timed(fn); timed(fn)
        ms = {name: [] for name, _ in legs}
        for r in range(a.rounds):
            for name, fn in (legs if r % 2 == 0 else legs[::-1]):
                ms[name].append(timed(fn))
        report(ms, legs)
        return ms

    print(f"probes_bench: {COUNTS[0]} x {COUNTS[1]} x {COUNTS[2]} = {P} probes x {RAYS} rays = {n} rays per update; {a.rounds} rounds x {a.calls} calls per leg, "
          f"alternating; device ms per call; {cus} CUs at {ghz:.2f} GHz")
    read_bytes, write_bytes = n * 48 + P * 3072 + RAYS * 16, P * 3072
    floor_bytes = (read_bytes + write_bytes) / HBM_BYTES_PER_S * 1e3
    evaluations = P * 232 * RAYS
    floor_weights = (P * 196 * RAYS * OPS_DISTANCE + P * 36 * RAYS * OPS_IRRADIANCE) / lane_rate * 1e3
    print(f"probes_blend floors: bytes {read_bytes / 1e6:.1f} MB read + {write_bytes / 1e6:.1f} MB written = {floor_bytes:.4f} ms; "
          f"weights {evaluations} evaluations ({OPS_DISTANCE} / {OPS_IRRADIANCE} operations each) = {floor_weights:.4f} ms; "
          f"the {'weight' if floor_weights > floor_bytes else 'byte'} floor binds")
    for config in (int(c) for c in a.configs.split(",")):
        if config == 2:
            sc, view, pos, cfg = scenes.config_cornell(luts, W, H)
            bounces, lo, hi = 4, (-0.9, 0.1, -3.9), (0.9, 1.9, 0.9)
        else:
            sc, view, pos, cfg = scenes.config_sponza_class(luts, W, H)
            bounces, lo, hi = 8, (-10.0, 0.3, -5.0), (10.0, 3.5, 5.0)
        cb = scenes.fill_constants(view, pos, sc, 0, bounces)
        spacing = [(hi[k] - lo[k]) / (COUNTS[k] - 1) for k in range(3)]
        vol = native.probe_volume(lo, spacing, COUNTS, RAYS, hysteresis=0.97, max_ray_distance=float(max(spacing)) * 1.5, distance_exponent=50.0,
                                  normal_bias=0.02, view_bias=0.02)
        ctx = native.PathTracerContext(0)
        ctx.set_stream(stream.cuda_stream)
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        pv = native.ProbeVolume(ctx, vol)
        rays, _ = native.probes_rays_host(vol, 1)
        with torch.cuda.stream(stream):
            d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda:0")
            d_rad = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
            d_hits = torch.zeros((n, 8), dtype=torch.float32, device="cuda:0")
        stream.synchronize()
        seed = [0]

        def two_calls():
            ctx.trace_radiance_device(d_rays.data_ptr(), d_rad.data_ptr(), n, cb)
            ctx.trace_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n)

        def update():
            seed[0] += 1
            pv.update(cb, seed[0])
        print(f"config {config}: {bounces} bounces, {len(sc.lights)} light(s)")
        legs = [("(a) hrpt_trace_radiance + hrpt_trace_rays on the same records", two_calls), ("(b) hrpt_probes_update", update)]
        ms = run(legs)
        ta, tb = statistics.median(ms[legs[0][0]]), statistics.median(ms[legs[1][0]])
        spread = max(ms[legs[0][0]]) - min(ms[legs[0][0]])
        print(f"  (b) - (a) = {tb - ta:+.3f} ms: ray generation plus blend; run-to-run spread of (a): {spread:.3f} ms")
        irr, _ = pv.read()
        print(f"  atlas after the updates: mean texel radiance {irr[:, 1:-1, 1:-1, :3].mean():.4f}, finite {bool(np.isfinite(irr).all())}")

        full = np.array(view, S.PlanarViewConstants)
        full["m_CameraDirectionOrPosition"] = (pos[0], pos[1], pos[2], 1.0)
        ctx.render(cb, accum_count=1)
        g = cb.copy(); g["m_Jitter"] = (0.0, 0.0)
        ctx.render_gbuffer(g, planes=S.GB_ALL_PLANES)
        legs = [(f"(c) hrpt_probes_shade_gbuffer at {W} x {H}", lambda: pv.shade_gbuffer(full, 1.0)), (f"    hrpt_demodulate at {W} x {H}", lambda: ctx.demodulate(full))]
        run(legs)
        e = ctx.read_probe_irradiance()
        print(f"  probe irradiance plane: {int((e[..., 3] == 1).sum())} hit pixels, mean E {e[..., :3][e[..., 3] == 1].mean():.4f}")
        pv.close(); ctx.close()


if __name__ == "__main__":
    main()
