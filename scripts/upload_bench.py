"""Wall time of hrpt_upload_scene on three routes of the acceleration-structure upload: the 101 k-triangle Sponza-class scene through the host
SAH builder, the same scene through the default (GPU) builder, and 1100 instances in the two-level structure with the instance tree built on
the GPU. One warm-up upload, then three timed ones; prints one JSON line with their median. HRPT_LIBRARY=<another build of the same ABI> for an
A/B: run the two libraries in alternating processes (profiles/device_headers_refactor.txt)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from hobbyrenderer_amd import native, scenes, structs as S
import bvh_scenes as B

luts = native.precompute_atmosphere()
sponza = scenes.sponza_class_scene(luts, 1.0, 8)
cases = [("sponza101k_host_sah", sponza, S.BVH_BUILDER_HOST_SAH, S.ACCEL_AUTO),
         ("sponza101k_default_gpu", sponza, S.BVH_BUILDER_AUTO, S.ACCEL_AUTO),
         ("instanced1100_two_level", B.instanced_scene(luts, 1100, detail=4), S.BVH_BUILDER_AUTO, S.ACCEL_TWO_LEVEL)]
out = {"library": os.path.basename(native.LIB_PATH)}
for name, sc, builder, accel in cases:
    ctx = native.PathTracerContext(0)
    try:
        ctx.set_bvh_builder(builder)
        ctx.set_acceleration_structure(accel)
        ms = []
        for k in range(4):
            t0 = time.perf_counter()
            ctx.upload_scene(sc)
            ms.append((time.perf_counter() - t0) * 1e3)
        bi = ctx.build_info()
        out[name] = {"median_ms": round(sorted(ms[1:])[1], 3), "all_ms": [round(m, 3) for m in ms], "usedBuilder": int(bi.usedBuilder), "structure": int(bi.structure)}
    finally:
        ctx.close()
print(json.dumps(out))
