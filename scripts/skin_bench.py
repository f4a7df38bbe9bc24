"""Cost of GPU skinning and morph targets (hrpt_skin_vertices_device / hrpt_update_vertices_skinned) on one MI355X.

1. The skinning kernel alone, between two HIP events on a stream of its own, CALLS launches back to back: vertex counts 5 293 and 58 417
   (the two scenes below) and larger ones up to where the kernel leaves the launch floor; palettes on both sides of
   HRPT_SKIN_LDS_MAX_JOINTS, and the palettes that fit the LDS once staged and once gathered from global memory (HRPT_SKIN_PALETTE=1,
   read by the library at every call); 0 and 2 morph targets. Against the byte floor at the copy figure of DESIGN.md section 15:
   48 + 24 + 36 T bytes read and 48 written per vertex. The quantiser kernel at the same counts stands next to it.
2. The full-range update on sponza_class_scene at detail 1.0 and 3.4, builders LBVH and PLOC, with and without VERTICES_REFIT:
   update_vertices_skinned (one call), the two-call route (skin_vertices_device + update_vertices_device), the host route
   (skin_vertices_host on 16 threads + quantize_vertices_host + update_vertices) and update_vertices_device alone (what a caller with
   its own skinning kernel pays after it). The calls are synchronous, so a job is timed on the host clock.
Both parts: the jobs alternate inside every round (the order reverses every other round), ROUNDS rounds after a warm-up; reported:
median over the rounds with min..max, the run-to-run spread a difference has to exceed.

    python scripts/skin_bench.py [--details 1.0 3.4 --calls 10 --rounds 7 --counts 5293 58417 262144 1048576 4194304]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

HBM_ACHIEVABLE = 6.29e12        # bytes / s, float4 copy on an MI355X


def pose(n, joint_count, targets, S, positions=None):
    """A case for native.skin_arrays: unit normals and tangents, four random joints per vertex out of near-identity joint matrices."""
    rng = np.random.default_rng(1)
    v = np.zeros(n, S.VertexFloat)
    v["pos"] = rng.uniform(-10, 10, (n, 3)) if positions is None else positions
    nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    tan = np.cross(nrm, rng.normal(size=(n, 3))); tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    v["normal"], v["uv"] = nrm, rng.random((n, 2))
    v["tangent"][:, :3], v["tangent"][:, 3] = tan, 1.0
    P = np.zeros((joint_count, 3, 4), np.float32)
    P[:, :, :3] = np.eye(3) + rng.uniform(-0.01, 0.01, (joint_count, 3, 3))
    P[:, :, 3] = rng.uniform(-0.01, 0.01, (joint_count, 3))
    joints = rng.integers(0, joint_count, (n, 4)).astype(np.uint16)
    w = rng.random((n, 4)) + 0.05
    case = dict(base=v, joints=joints, weights=(w / w.sum(1, keepdims=True)).astype(np.float32), joint_matrices=P)
    if targets:
        d = np.zeros((targets, n), S.SkinMorphDelta)
        for f in ("pos", "normal", "tangent"):
            d[f] = rng.normal(size=(targets, n, 3)) * 0.001
        case.update(deltas=d, morph_weights=np.full(targets, 0.5, np.float32))
    return case


class OnDevice:
    def __init__(self, case, native, torch):
        arrays, self.count, self.joint_count, self.target_count = native.skin_arrays(**case)
        self.tensors = [None if a is None else torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0") for a in arrays]
        self.args = tuple(0 if t is None else t.data_ptr() for t in self.tensors) + (self.count, self.joint_count, self.target_count)


def report(name, values, unit, extra=""):
    print(f"  {name:44s} median {statistics.median(values):9.3f}  min {min(values):9.3f}  max {max(values):9.3f} {unit}{extra}")


def alternate(jobs, rounds, one):
    """one(fn) -> a time; the jobs in turn inside every round, the order reversed every other round."""
    for _, fn in jobs:
        one(fn)
    out = {name: [] for name, _ in jobs}
    for r in range(rounds):
        for name, fn in (jobs if r % 2 == 0 else jobs[::-1]):
            out[name].append(one(fn))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--details", type=float, nargs="*", default=[1.0, 3.4])
    ap.add_argument("--counts", type=int, nargs="*", default=[5293, 58417, 262144, 1048576, 4194304])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()

    import torch
    from hobbyrenderer_amd import native, scenes, structs as S
    if not torch.cuda.is_available():
        raise SystemExit("skin_bench: no GPU; this script measures and does not fall back")
    T = S.SKIN_LDS_MAX_JOINTS
    print(f"skin_bench ({os.path.basename(native.LIB_PATH)}): {a.rounds} rounds, alternating; HRPT_SKIN_LDS_MAX_JOINTS = {T}")

    def palette_mode(gather):
        os.environ["HRPT_SKIN_PALETTE"] = "1" if gather else "0"

    # ---- 1. the kernels alone
    c = native.PathTracerContext(0)
    stream = torch.cuda.Stream()
    calls = 50
    for n in a.counts:
        with torch.cuda.stream(stream):
            out = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
            packed = torch.zeros(n * 24, dtype=torch.uint8, device="cuda:0")
        for targets in (0, 2):
            devs = {jc: OnDevice(pose(n, jc, targets, S), native, torch) for jc in (64, T, T + 1, 4 * T)}

            def launch(jc, gather):
                def fn():
                    c.skin_vertices_device(*devs[jc].args, out.data_ptr(), 0, stream.cuda_stream)
                fn.gather = gather
                return fn

            jobs = [(f"skin_vertices {jc:5d} joints, {'gather' if gather else 'LDS'}", launch(jc, gather))
                    for jc, gather in ((64, False), (64, True), (T, False), (T, True), (T + 1, True), (4 * T, True))]
            jobs.append(("quantise_vertices (48 B in, 24 B out)", lambda: c.quantize_vertices_device(out.data_ptr(), n, packed.data_ptr(), stream.cuda_stream)))

            def kernel_round(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                palette_mode(getattr(fn, "gather", False))              # (once per round, outside the timed launches)
                stream.synchronize()
                e0.record(stream)
                for _ in range(calls):
                    fn()
                e1.record(stream)
                stream.synchronize()
                return e0.elapsed_time(e1) * 1e3 / calls

            us = alternate(jobs, a.rounds, kernel_round)
            bytes_per_vertex = 48 + 24 + 36 * targets + 48
            floor = bytes_per_vertex * n / HBM_ACHIEVABLE * 1e6
            print(f"kernels, {n} vertices, {targets} targets: microseconds per launch between HIP events, {calls} launches back to back; "
                  f"byte floor ({bytes_per_vertex} B per vertex at {HBM_ACHIEVABLE / 1e12:.2f} TB/s) {floor:.3f} us")
            for name, _ in jobs:
                f = floor if name.startswith("skin") else 72 * n / HBM_ACHIEVABLE * 1e6
                report(name, us[name], "us", f"   floor / median {f / statistics.median(us[name]):6.3f}")
            del devs
    palette_mode(False)
    c.close()

    # ---- 2. the full-range update
    luts = native.precompute_atmosphere() if a.details else None
    for detail in a.details:
        sc = scenes.sponza_class_scene(luts, detail, 8)
        n = len(sc.vertices)
        case = pose(n, 64, 2, S, sc.vertices["m_Pos"])
        for builder, label in ((S.BVH_BUILDER_GPU_LBVH, "lbvh"), (S.BVH_BUILDER_GPU_PLOC, "ploc")):
            c = native.PathTracerContext(0)
            c.set_bvh_builder(builder)
            c.upload_scene(sc)
            tris = c.build_info().triangleCount
            dev = OnDevice(case, native, torch)
            floats = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
            ptr = floats.data_ptr()

            def two_calls(flags):
                c.skin_vertices_device(*dev.args, ptr)
                c.update_vertices_device(ptr, 0, n, flags)

            def host_route(flags):
                c.update_vertices(native.quantize_vertices_host(native.skin_vertices_host(**case, nthreads=16), nthreads=16), 0, flags)

            jobs = []
            for flags, tag in ((0, ""), (S.VERTICES_REFIT, " REFIT")):
                jobs += [("update_vertices_skinned" + tag, lambda flags=flags: c.update_vertices_skinned(*dev.args, 0, flags)),
                         ("skin_vertices_device + update_vertices_device" + tag, lambda flags=flags: two_calls(flags)),
                         ("host skin + quantise + update_vertices" + tag, lambda flags=flags: host_route(flags)),
                         ("update_vertices_device alone" + tag, lambda flags=flags: c.update_vertices_device(ptr, 0, n, flags))]

            def timed(fn):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                return (time.perf_counter() - t0) * 1e3 / a.calls

            two_calls(0)
            ms = alternate(jobs, a.rounds, timed)
            print(f"detail {detail}: {n} vertices, {tris} world triangles, {label}; 64 joints, 2 targets; milliseconds per call, host clock, {a.calls} calls back to back")
            for name, _ in jobs:
                report(name, ms[name], "ms")
            for tag in ("", " REFIT"):
                fused, two = ms["update_vertices_skinned" + tag], ms["skin_vertices_device + update_vertices_device" + tag]
                print(f"  one call - two calls{tag:6s} = {statistics.median(fused) - statistics.median(two):+8.3f} ms (medians; spreads {max(fused) - min(fused):.3f} and {max(two) - min(two):.3f})")
            c.close()


if __name__ == "__main__":
    main()
