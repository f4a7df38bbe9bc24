"""Time of the hash-grid radiance cache against the traced diffuse lobe it replaces, on one MI355X at 1920 x 1080
inside the scenes of config 2 (Cornell box) and config 4 (Sponza-class):

  (a)  hrpt_indirect_lighting(HRPT_INDIRECT_DIFFUSE): one path of up to m_MaxBounces segments per pixel. Its kernels are the parent
       commit's (scripts/kernel_diff.py reports every existing kernel identical), so this leg IS the parent's stage in the same run.
  (b)  hrpt_rcache_update, one frame of filling (one pixel per 5 x 5 block), with the wave-local combine and without
  (c)  hrpt_rcache_indirect after 1, 8 and 60 updates, with the traced fallback and with HRPT_RCACHE_NO_FALLBACK, and the served fraction
  (d)  the kernels alone over caller-owned device arrays: the surface query over the frame's diffuse records, insert over one sample per
       pixel (the coherent case: neighbours share a voxel) and over every 25th (the update's density) with and without the combine,
       resolve over the 2^22-entry table, query over one point per pixel

Method (measuring-on-mi355x): one stream, the legs alternate inside every round, ROUNDS rounds after a warm-up; a leg's time is CALLS
back-to-back calls between two HIP events on the stream, divided by CALLS; reported: median over the rounds and min..max, the run-to-run
spread a difference has to exceed.

Byte floors, printed with the measurement, over 8 TB/s: insert gathers an 8-byte key and adds into a 32-byte record per sample and reads
the 48-byte sample; query reads a 32- or 48-byte record, gathers a key and a 16-byte entry and writes 20 bytes; resolve streams 56 bytes
per entry of the table.

    python scripts/rcache_bench.py [--calls 4 --rounds 9 --configs 2,4 --size 1920x1080 --bounces 3 --out profiles/rcache_bench.txt]
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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rcache_bench.txt"))
    a = ap.parse_args()

    import torch
    from hobbyrenderer_amd import native, scenes, structs as S
    if not torch.cuda.is_available():
        raise SystemExit("rcache_bench: no GPU; this script measures and does not fall back")
    W, H = (int(v) for v in a.size.split("x"))
    px = W * H
    luts = native.precompute_atmosphere()
    stream = torch.cuda.Stream()
    four = sum(1 << p for p in (S.GB_ALBEDO, S.GB_NORMAL, S.GB_GEO_NORMAL, S.GB_DEPTH))
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

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
            say(f"  {name:66s} median {statistics.median(t):8.3f}  min {min(t):8.3f}  max {max(t):8.3f}")
        return {name: statistics.median(t) for name, t in ms.items()}

    say(f"rcache_bench: {W} x {H}, m_MaxBounces {a.bounces}; {a.rounds} rounds x {a.calls} calls per leg, alternating; device ms per call")
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
        cam = np.asarray(cb["m_CameraPos"], np.float32).reshape(-1)[:3]
        ctx.render_gbuffer(cb, planes=four)
        desc = native.rcache_desc()
        cache = native.RadianceCache(ctx, desc)
        dif = S.IndirectParams(S.INDIRECT_DIFFUSE, 1)
        say(f"config {config}: table 2^{int(desc['capacityLog2'])} entries, block {int(desc['sparseBlock'])}")
        frame = [0]

        def update(flags=0):
            frame[0] += 1
            cache.update(cb, frame[0], flags)

        def served_after(n):
            while frame[0] < n:
                update()
            cache.indirect(cb, S.RcacheParams(0, 1))
            plane = ctx.read_rcache_served()
            keys, _, _, drops = cache.read()
            return float((plane[..., 3] == 1).mean()), int((keys != 0).sum()), drops

        for n in (1, 8, 60):
            frac, entries, drops = served_after(n)
            say(f"  after {n:2d} update(s): served fraction {frac:.4f}, {entries} entries, {drops} drops")
            if n == 60:
                continue
            run([(f"(c) hrpt_rcache_indirect after {n} update(s)", lambda: cache.indirect(cb, S.RcacheParams(0, 1))),
                        (f"(c) hrpt_rcache_indirect after {n} update(s), NO_FALLBACK", lambda: cache.indirect(cb, S.RcacheParams(S.RCACHE_NO_FALLBACK, 1)))])
        t = run([("(a) hrpt_indirect_lighting, diffuse (the parent's stage)", lambda: ctx.indirect_lighting(cb, dif)),
                 ("(b) hrpt_rcache_update, wave combine", lambda: update()),
                 ("(b) hrpt_rcache_update, HRPT_RCACHE_NO_WAVE_COMBINE", lambda: update(S.RCACHE_NO_WAVE_COMBINE)),
                 ("(c) hrpt_rcache_indirect after 60+ updates", lambda: cache.indirect(cb, S.RcacheParams(0, 1))),
                 ("(c) hrpt_rcache_indirect after 60+ updates, NO_FALLBACK", lambda: cache.indirect(cb, S.RcacheParams(S.RCACHE_NO_FALLBACK, 1)))])
        a_ms = t["(a) hrpt_indirect_lighting, diffuse (the parent's stage)"]
        both = t["(b) hrpt_rcache_update, wave combine"] + t["(c) hrpt_rcache_indirect after 60+ updates"]
        say(f"  update + indirect = {both:.3f} ms against {a_ms:.3f} ms of the traced diffuse lobe: {a_ms / both:.2f} x")
        cache.indirect(cb, S.RcacheParams(0, 1))
        mean_cache = ctx.read_indirect(0)[..., :3].mean()
        ctx.indirect_lighting(cb, dif)
        mean_traced = ctx.read_indirect(0)[..., :3].mean()
        say(f"  diffuse plane mean: cache {mean_cache:.4f}, traced {mean_traced:.4f} (one seed each)")

        # (d) the kernels alone
        planes = [ctx.gbuffer_device(p) for p in (S.GB_ALBEDO, S.GB_NORMAL, S.GB_GEO_NORMAL, S.GB_DEPTH)]
        with torch.cuda.stream(stream):
            rays = torch.zeros(px * 12, dtype=torch.float32, device="cuda:0")
            surf = torch.zeros(px * 12, dtype=torch.float32, device="cuda:0")
            out4, voxel = torch.zeros(px * 4, dtype=torch.float32, device="cuda:0"), torch.zeros(px, dtype=torch.float32, device="cuda:0")
        ctx.indirect_rays_device(S.IndirectImages(*planes, None, None, None), W, H, cb, rays.data_ptr(), dif, stream.cuda_stream)
        ctx.rcache_surfaces_device(rays.data_ptr(), surf.data_ptr(), px, stream.cuda_stream)
        stream.synchronize()
        hs = surf.cpu().numpy().view(S.RcacheSurface)
        samples = np.zeros(px, S.RcacheSample)
        samples["position"], samples["normal"], samples["radiance"], samples["valid"] = hs["position"], hs["normal"], 1.0, (hs["hit"] != 0)
        sparse = np.ascontiguousarray(samples.reshape(H, W)[2::5, 2::5]).reshape(-1)
        n = 1 << int(desc["capacityLog2"])
        with torch.cuda.stream(stream):
            d_full, d_sparse = (torch.from_numpy(s.view(np.uint8).copy()).to("cuda:0") for s in (samples, sparse))
            keys, accum = torch.zeros(n, dtype=torch.int64, device="cuda:0"), torch.zeros(n * 4, dtype=torch.int64, device="cuda:0")
            resolved, drops = torch.zeros(n * 2, dtype=torch.int64, device="cuda:0"), torch.zeros(2, dtype=torch.int64, device="cuda:0")
        tab = (keys.data_ptr(), accum.data_ptr())
        ins = lambda d, c, f: ctx.rcache_insert_device(desc, cam, *tab, drops.data_ptr(), d.data_ptr(), c, f, stream.cuda_stream)     # noqa: E731
        ins(d_full, px, 0)                                  # the table holds the frame's keys before anything is timed
        ctx.rcache_resolve_device(desc, *tab, resolved.data_ptr(), 0, stream.cuda_stream)
        floor = lambda b: b / HBM_BYTES_PER_S * 1e3         # noqa: E731
        say(f"  byte floors: insert {floor(px * 88):.4f} ms (one per pixel) / {floor(len(sparse) * 88):.4f} ms (every 25th); query {floor(px * 92):.4f} ms; "
            f"resolve {floor(n * 56):.4f} ms; surfaces (records only) {floor(px * 96):.4f} ms")
        run([("(d) pt_surface_rays_kernel, one ray per pixel", lambda: ctx.rcache_surfaces_device(rays.data_ptr(), surf.data_ptr(), px, stream.cuda_stream)),
             ("(d) rcache_insert<true>, one sample per pixel", lambda: ins(d_full, px, 0)),
             ("(d) rcache_insert<false>, one sample per pixel", lambda: ins(d_full, px, S.RCACHE_NO_WAVE_COMBINE)),
             ("(d) rcache_insert<true>, every 25th pixel", lambda: ins(d_sparse, len(sparse), 0)),
             ("(d) rcache_insert<false>, every 25th pixel", lambda: ins(d_sparse, len(sparse), S.RCACHE_NO_WAVE_COMBINE)),
             ("(d) rcache_resolve, 2^22 entries", lambda: (ins(d_sparse, len(sparse), 0), ctx.rcache_resolve_device(desc, *tab, resolved.data_ptr(), 0, stream.cuda_stream))),
             ("(d) rcache_query, one point per pixel", lambda: ctx.rcache_query_device(desc, cam, keys.data_ptr(), resolved.data_ptr(), surf.data_ptr(), out4.data_ptr(),
                                                                                      voxel.data_ptr(), px, stream.cuda_stream))])
        say("  (the resolve leg includes one every-25th insert, which keeps the table alive; subtract that leg)")
        cache.close()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
