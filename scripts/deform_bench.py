"""Cost of a per-frame vertex update (hrpt_update_vertices / hrpt_update_vertices_device) on one MI355X, next to the instance calls the
library already had, on the same context and scene in the same run -- the difference between a vertex call and its instance counterpart
is what a deforming mesh adds to a frame -- and the quantiser kernel alone against its byte floor (48 B read + 24 B written per vertex).

Scenes: sponza_class_scene at detail 1.0 (101 k world triangles) and 3.4 (1.17 M); builders LBVH and PLOC. Jobs, all over the full range:
update_vertices, update_vertices_device, both with VERTICES_REFIT, update_instances, refit_instances. The calls are synchronous, so a job
is timed on the host clock: a round times CALLS back-to-back calls of one job; the jobs alternate inside every round (the order reverses
every other round), ROUNDS rounds after a warm-up; reported: median over the rounds with min..max, the run-to-run spread a difference has
to exceed. The quantiser is timed between two HIP events on a stream of its own, CALLS launches back to back.

    python scripts/deform_bench.py [--details 1.0 3.4 --calls 10 --rounds 7]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

HBM_ACHIEVABLE = 6.29e12        # bytes / s, float4 copy on an MI355X


def float_records(sc, S):
    """S.VertexFloat records for the scene's vertices: the positions as they are, a unit normal and tangent, uv in [0, 1)."""
    rng = np.random.default_rng(1)
    n = len(sc.vertices)
    v = np.zeros(n, S.VertexFloat)
    v["pos"] = sc.vertices["m_Pos"]
    nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    tan = np.cross(nrm, rng.normal(size=(n, 3))); tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    v["normal"], v["uv"] = nrm, rng.random((n, 2))
    v["tangent"][:, :3], v["tangent"][:, 3] = tan, 1.0
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--details", type=float, nargs="+", default=[1.0, 3.4])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()

    import torch
    from hobbyrenderer_amd import native, scenes, structs as S
    if not torch.cuda.is_available():
        raise SystemExit("deform_bench: no GPU; this script measures and does not fall back")
    luts = native.precompute_atmosphere()
    print(f"deform_bench ({os.path.basename(native.LIB_PATH)}): {a.rounds} rounds x {a.calls} calls per job, alternating; milliseconds per call, host clock")

    for detail in a.details:
        sc = scenes.sponza_class_scene(luts, detail, 8)
        fv = float_records(sc, S)
        quantised = native.quantize_vertices_host(fv)
        n = len(fv)
        for builder, label in ((S.BVH_BUILDER_GPU_LBVH, "lbvh"), (S.BVH_BUILDER_GPU_PLOC, "ploc")):
            c = native.PathTracerContext(0)
            c.set_bvh_builder(builder)
            c.upload_scene(sc)
            tris = c.build_info().triangleCount
            dev = torch.from_numpy(fv.view(np.uint8).copy()).to("cuda:0")
            ptr = dev.data_ptr()
            jobs = [("update_vertices", lambda: c.update_vertices(quantised)),
                    ("update_vertices_device", lambda: c.update_vertices_device(ptr, 0, n)),
                    ("update_instances", lambda: c.update_instances(sc.instances)),
                    ("update_vertices REFIT", lambda: c.update_vertices(quantised, 0, S.VERTICES_REFIT)),
                    ("update_vertices_device REFIT", lambda: c.update_vertices_device(ptr, 0, n, S.VERTICES_REFIT)),
                    ("refit_instances", lambda: c.refit_instances(sc.instances))]

            def timed(fn):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                return (time.perf_counter() - t0) * 1e3 / a.calls

            for _, fn in jobs:                                   # warm-up: code objects, the staging buffer
                fn(); fn()
            ms = {name: [] for name, _ in jobs}
            for r in range(a.rounds):
                for name, fn in (jobs if r % 2 == 0 else jobs[::-1]):
                    ms[name].append(timed(fn))
            print(f"detail {detail}: {n} vertices, {tris} world triangles, {label}; PCIe payload {24 * n / 1e6:.2f} MB of quantised vertices")
            for name, _ in jobs:
                m = ms[name]
                print(f"  {name:30s} median {statistics.median(m):8.3f}  min {min(m):8.3f}  max {max(m):8.3f}")
            for vertex, instance in (("update_vertices", "update_instances"), ("update_vertices_device", "update_instances"),
                                     ("update_vertices REFIT", "refit_instances"), ("update_vertices_device REFIT", "refit_instances")):
                print(f"  {vertex:30s} - {instance:16s} = {statistics.median(ms[vertex]) - statistics.median(ms[instance]):+8.3f} ms (medians)")

            # the quantiser alone, between HIP events
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                out = torch.zeros(n * 24, dtype=torch.uint8, device="cuda:0")
            calls = 50

            def kernel_round():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                stream.synchronize()
                e0.record(stream)
                for _ in range(calls):
                    c.quantize_vertices_device(ptr, n, out.data_ptr(), stream.cuda_stream)
                e1.record(stream)
                stream.synchronize()
                return e0.elapsed_time(e1) * 1e3 / calls
            if label == "lbvh":                                  # (the kernel does not depend on the builder)
                kernel_round()
                us = [kernel_round() for _ in range(a.rounds)]
                floor = 72 * n / HBM_ACHIEVABLE * 1e6
                print(f"  quantise_vertices kernel, {n} vertices: median {statistics.median(us):7.2f} us  min {min(us):7.2f}  max {max(us):7.2f}"
                      f"   byte floor (72 B per vertex at {HBM_ACHIEVABLE / 1e12:.2f} TB/s) {floor:6.3f} us")
            c.close()


if __name__ == "__main__":
    main()
