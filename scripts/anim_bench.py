"""Measures the animation stage on the GPU (output kept in profiles/anim_bench.txt). Not part of bench.py.

Two workloads, each through the device route and through the host route it replaces, on one context each, alternating round by round:
  instances  N single-node instances (default 65 536 cubes, flat structure, the builder the library picks), every node with a slerp
             rotation and a linear translation channel:  hrpt_animate   against   hrpt_animate_host (16 threads) + hrpt_update_instances
  skeleton   a 256-joint skeleton driving a mesh of about 100 k vertices:  hrpt_animate(NO_COMMIT) + hrpt_update_vertices_skinned with the
             palette and weights taken from hrpt_get_animation_device   against   hrpt_animate_host + palette upload + the same call
Host clock around the whole route (every route ends synchronised); with HRPT_ANIM_TIMING the library reports the device time of the three
animate kernels between stream events and the host time of the read-back + roll and of the commit (the rebuild). Per figure: the median
over the rounds with min..max, the run-to-run spread a difference has to exceed. The first rounds are warm-up and are dropped."""
import argparse
import os
import re
import statistics
import sys
import tempfile
import time

os.environ["HRPT_ANIM_TIMING"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import numpy as np  # noqa: E402

from hobbyrenderer_amd import native, scenes, structs as S  # noqa: E402


class Stderr:
    """File descriptor 2 into a file while the library reports its timings there."""

    def __enter__(self):
        self.file = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.file.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.file.seek(0)
        self.text = self.file.read().decode(errors="replace")
        self.file.close()


def report(name, values, unit="ms"):
    print(f"  {name:58s} median {statistics.median(values):9.4f}  min {min(values):9.4f}  max {max(values):9.4f} {unit}", flush=True)


def library_figures(text, into):
    for line in text.splitlines():
        if line.startswith("[animate]"):
            for key, value in re.findall(r"([a-z\- ]+?) ([0-9.]+) ms", line[len("[animate]"):]):
                into.setdefault(key.strip(), []).append(float(value))


def quaternions(rng, n):
    q = rng.standard_normal((n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def instance_tables(n, rng):
    side = int(np.ceil(n ** (1 / 3)))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n].astype(np.float32) * 3.0
    nodes = np.zeros(n, S.AnimNode)
    nodes["parent"], nodes["translation"], nodes["rotation"], nodes["scale"] = -1, grid, quaternions(rng, n), 1.0
    nodes["firstInstance"], nodes["instanceCount"] = np.arange(n), 1
    samplers, channels = np.zeros(2 * n, S.AnimSampler), np.zeros(2 * n, S.AnimChannel)
    samplers["interpolation"] = np.tile([S.ANIM_SLERP, S.ANIM_LINEAR], n)
    samplers["firstKey"], samplers["keyCount"] = 4 * np.arange(2 * n), 4
    channels["path"] = np.tile([S.ANIM_PATH_ROTATION, S.ANIM_PATH_TRANSLATION], n)
    channels["sampler"], channels["firstTarget"], channels["targetCount"] = np.arange(2 * n), np.arange(2 * n), 1
    values = np.zeros((2 * n, 4, 4), np.float32)
    values[0::2] = quaternions(rng, 4 * n).reshape(n, 4, 4)
    values[1::2, :, :3] = grid[:, None, :] + rng.uniform(-0.5, 0.5, (n, 4, 3))
    tables = dict(samplers=samplers, channels=channels, nodes=nodes, key_times=np.tile(np.array([0, 1, 2, 3], np.float32), 2 * n), key_values=values.reshape(-1, 4),
                  targets=np.repeat(np.arange(n), 2), node_instances=np.arange(n), animation_count=1)
    anim = native.Animation(**tables)
    anim.set_times([0.0])
    nodes["baseWorld"] = anim.evaluate_host()[3]
    anim.close()
    return tables


def bench_instances(n, rounds, warmup, luts):
    print(f"instances: {n} single-node instances, two channels each", flush=True)
    rng = np.random.default_rng(1)
    tables = instance_tables(n, rng)
    b = scenes.SceneBuilder()
    mesh, mat = b.add_mesh(*scenes.generate_default_cube()), b.add_material()
    for w in tables["nodes"]["baseWorld"]:
        b.add_instance(mesh, mat, w)
    sc = b.finalize(luts)
    anim = native.Animation(**tables)
    device, host = native.PathTracerContext(0), native.PathTracerContext(0)
    for c in (device, host):
        c.upload_scene(sc)
    print(f"  builder {device.build_info().usedBuilder}, {device.build_info().triangleCount} triangles", flush=True)
    now = sc.instances.copy()
    figures, lib = {}, {}
    for r in range(rounds + warmup):
        anim.advance(0.11)
        with Stderr() as err:
            t0 = time.perf_counter()
            device.animate(anim)
            t1 = time.perf_counter()
        t2 = time.perf_counter()
        now = anim.evaluate_host(now, nthreads=16)[0]
        t3 = time.perf_counter()
        host.update_instances(now)
        t4 = time.perf_counter()
        if r >= warmup:
            library_figures(err.text, lib)
            for k, v in (("hrpt_animate", t1 - t0), ("host route: animate_host(16) + update_instances", t4 - t2), ("  of which hrpt_animate_host (with the wrapper's copy)", t3 - t2),
                         ("  of which hrpt_update_instances", t4 - t3)):
                figures.setdefault(k, []).append(1e3 * v)
    for k, v in figures.items():
        report(k, v)
    for k, v in lib.items():
        report(f"hrpt_animate, library clock: {k}", v)
    same = device.read_bvh()["triangleCount"] == host.read_bvh()["triangleCount"]
    print(f"  structures agree in size: {same}", flush=True)
    device.close(); host.close(); anim.close()


def bench_skeleton(joints, rounds, warmup, luts):
    import torch
    import skin_cases as SK
    print(f"skeleton: {joints} joints", flush=True)
    rng = np.random.default_rng(2)
    b = scenes.SceneBuilder()
    mesh, mat = b.add_mesh(*scenes.mesh_sphere(448, 224)), b.add_material()
    b.add_instance(mesh, mat)
    sc = b.finalize(luts)
    count = len(sc.vertices)
    base = np.zeros(count, S.VertexFloat)
    base["pos"] = sc.vertices["m_Pos"]
    base["normal"] = base["pos"] / np.maximum(np.linalg.norm(base["pos"], axis=1, keepdims=True), 1e-6)
    base["tangent"][:, 0], base["tangent"][:, 3] = 1, 1
    pose = SK.gentle_pose(base, joints, 3, amplitude=0.01, targets=2)
    nodes = np.zeros(joints + 1, S.AnimNode)
    nodes["parent"] = [-1] + [0 if j == 0 else 1 + (j - 1) // 4 for j in range(joints)]
    nodes["rotation"][:, 3], nodes["scale"] = 1, 1
    nodes["translation"][1:] = rng.uniform(-0.01, 0.01, (joints, 3))
    nodes["baseWorld"] = np.eye(4, dtype=np.float32)
    jt = np.zeros(joints, S.AnimJoint)
    jt["node"], jt["inverseBind"] = 1 + np.arange(joints), np.eye(4, dtype=np.float32)
    samplers, channels = np.zeros(joints + 2, S.AnimSampler), np.zeros(joints + 2, S.AnimChannel)
    samplers["interpolation"], samplers["firstKey"], samplers["keyCount"] = S.ANIM_SLERP, 4 * np.arange(joints + 2), 4
    samplers["interpolation"][joints:] = S.ANIM_LINEAR
    channels["path"], channels["sampler"], channels["firstTarget"], channels["targetCount"] = S.ANIM_PATH_ROTATION, np.arange(joints + 2), np.arange(joints + 2), 1
    channels["path"][joints:] = S.ANIM_PATH_WEIGHTS
    q = np.concatenate([rng.uniform(-0.02, 0.02, (4 * joints, 3)), np.ones((4 * joints, 1))], 1)
    values = np.concatenate([(q / np.linalg.norm(q, axis=1, keepdims=True)), rng.uniform(0, 0.5, (8, 4))]).astype(np.float32)
    tables = dict(samplers=samplers, channels=channels, nodes=nodes, joints=jt, key_times=np.tile(np.array([0, 1, 2, 3], np.float32), joints + 2), key_values=values,
                  targets=np.concatenate([1 + np.arange(joints), [0, 1]]), animation_count=1, morph_weight_count=2)
    anim = native.Animation(**tables)
    arrays, n, jc, tc = native.skin_arrays(**pose)
    tensors = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0") for a in arrays]
    args = [t.data_ptr() for t in tensors]
    device, host = native.PathTracerContext(0), native.PathTracerContext(0)
    for c in (device, host):
        c.set_bvh_builder(S.BVH_BUILDER_GPU_LBVH)
        c.upload_scene(sc)
    print(f"  {count} vertices, {device.build_info().triangleCount} triangles", flush=True)
    figures, lib = {}, {}
    for r in range(rounds + warmup):
        anim.advance(0.11)
        with Stderr() as err:
            t0 = time.perf_counter()
            device.animate(anim, S.ANIMATE_NO_COMMIT)
            palette, weights, _ = device.animation_device(anim)
            device.update_vertices_skinned(args[0], args[1], args[2], palette, args[4], weights, n, jc, tc, 0, 0)
            t1 = time.perf_counter()
        t2 = time.perf_counter()
        _, hp, hw, _ = anim.evaluate_host(nthreads=16)
        t3 = time.perf_counter()
        dp, dw = torch.from_numpy(hp).to("cuda:0"), torch.from_numpy(hw).to("cuda:0")
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        host.update_vertices_skinned(args[0], args[1], args[2], dp.data_ptr(), args[4], dw.data_ptr(), n, jc, tc, 0, 0)
        t5 = time.perf_counter()
        if r >= warmup:
            library_figures(err.text, lib)
            for k, v in (("hrpt_animate(NO_COMMIT) + hrpt_update_vertices_skinned", t1 - t0), ("host route: animate_host(16) + upload + update_vertices_skinned", t5 - t2),
                         ("  of which hrpt_animate_host", t3 - t2), ("  of which palette and weights upload", t4 - t3), ("  of which hrpt_update_vertices_skinned", t5 - t4)):
                figures.setdefault(k, []).append(1e3 * v)
    for k, v in figures.items():
        report(k, v)
    for k, v in lib.items():
        report(f"hrpt_animate, library clock: {k}", v)
    device.close(); host.close(); anim.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=65536)
    ap.add_argument("--joints", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    luts = native.precompute_atmosphere()
    bench_instances(a.instances, a.rounds, a.warmup, luts)
    bench_skeleton(a.joints, a.rounds, a.warmup, luts)


if __name__ == "__main__":
    main()
