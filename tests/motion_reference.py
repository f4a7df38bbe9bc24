"""NumPy restatement of the first-hit motion vectors (hrpt_render_motion_vectors) -- TEST INFRASTRUCTURE.

Shares no code with hobbyrenderer_amd/csrc/pt_motion.h. The hits come from gbuffer_reference.trace (the oracle's TraceRayStandard), the
object-space positions from gbuffer_reference.unpacked_vertices; the two transforms, the interpolation, the two projections, the window
transform and the differences are NumPy float32 with one rounding per operation in the order the definition fixes: row-vector products summed
left to right, no contraction, IEEE division. motion64 states the same projection in float64 (float64 vertices and matrices, the float32
barycentrics) for the accuracy figures of tests/test_motion_cpu.py."""
import numpy as np

f32 = np.float32


def _hit_triangles(scene, verts, tr):
    """(ys, xs, instance records, [q0, q1, q2] float32 [n, 3], u, v) of the hit pixels."""
    ys, xs = np.nonzero(tr["hit"])
    inst = tr["inst"][ys, xs]; prim = tr["prim"][ys, xs]
    rec = scene.instances[inst]
    mesh = scene.mesh_data[rec["m_MeshDataIndex"]]
    base = mesh["m_IndexOffsets"][:, 0].astype(np.int64) + 3 * prim.astype(np.int64)              # LOD 0 (PathTracer.hlsl:102-103)
    q = [np.ascontiguousarray(verts[scene.indices[base + k], 0:3]) for k in range(3)]
    return ys, xs, rec, q, tr["u"][ys, xs], tr["v"][ys, xs]


def _transform_point(p, m):
    """mul(float4(p, 1), M).xyz, left to right; p [n, 3], m [n, 4, 4]."""
    return np.stack([((p[:, 0] * m[:, 0, k] + p[:, 1] * m[:, 1, k]) + p[:, 2] * m[:, 2, k]) + m[:, 3, k] for k in range(3)], -1)


def _interpolate(p, u, v, one):
    bx = (one - u) - v
    return (p[0] * bx[:, None] + p[1] * u[:, None]) + p[2] * v[:, None]


def _project(p, view, dtype):
    """(window xy [n, 2], clip w [n]) of world points p through view's m_MatWorldToClip and window transform."""
    m = np.asarray(view["m_MatWorldToClip"], dtype)
    one = dtype(1.0)
    clip = [((p[:, 0] * m[0, c] + p[:, 1] * m[1, c]) + p[:, 2] * m[2, c]) + one * m[3, c] for c in (0, 1, 3)]
    scale, bias = np.asarray(view["m_ClipToWindowScale"], dtype), np.asarray(view["m_ClipToWindowBias"], dtype)
    win = np.stack([(clip[0] / clip[2]) * scale[0] + bias[0], (clip[1] / clip[2]) * scale[1] + bias[1]], -1)
    return win, clip[2]


def _motion(scene, cb, prev_view, width, height, verts, tr, dtype):
    out = np.zeros((height, width, 4), dtype)
    ys, xs, rec, q, u, v = _hit_triangles(scene, verts, tr)
    if len(ys) == 0:
        return out, None
    q = [p.astype(dtype) for p in q]
    world, prev_world = np.asarray(rec["m_World"], dtype), np.asarray(rec["m_PrevWorld"], dtype)
    cur = [_transform_point(p, world) for p in q]
    prev = [_transform_point(p, prev_world) for p in q]
    u, v = u.astype(dtype), v.astype(dtype)
    world_pos, prev_world_pos = _interpolate(cur, u, v, dtype(1.0)), _interpolate(prev, u, v, dtype(1.0))
    win, w = _project(world_pos, cb["m_View"], dtype)
    prev_win, prev_w = _project(prev_world_pos, prev_view, dtype)
    out[ys, xs] = np.concatenate([prev_win - win, (prev_w - w)[:, None], np.ones((len(ys), 1), dtype)], 1)
    assert out.dtype == dtype
    return out, dict(ys=ys, xs=xs, window=win, prev_window=prev_win, w=w, prev_w=prev_w)


def motion(scene, cb, prev_view, width, height, verts, traced, details=False):
    """The motion plane for constants `cb`, last frame's view `prev_view` and scene.instances' m_World / m_PrevWorld: float32 [H, W, 4] =
    (prevWindow - window, prevClip.w - clip.w, 1) on hits, zeros on misses. `verts`: gbuffer_reference.unpacked_vertices(scene); `traced`:
    gbuffer_reference.trace(...) for the same constants. With details: also the dict of window positions and clip w of the hit pixels."""
    out, d = _motion(scene, cb, prev_view, width, height, verts, traced, f32)
    return (out, d) if details else out


def motion64(scene, cb, prev_view, width, height, verts, traced):
    """The same statement in float64 (float64 copies of the float32 inputs): what the float32 result is measured against."""
    return _motion(scene, cb, prev_view, width, height, verts, traced, np.float64)[0]
