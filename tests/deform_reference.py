"""NumPy restatement of the first-hit motion vectors of a DEFORMING mesh (hrpt_update_vertices + hrpt_render_motion_vectors, DESIGN.md
section 21) -- TEST INFRASTRUCTURE.

The definition of tests/motion_reference.py with one change: the previous world position is formed from the object-space positions of the
PREVIOUS frame, prev_k = qprev_k * m_PrevWorld, the current one from the current positions, cur_k = q_k * m_World. The transform, the
interpolation and the projection are motion_reference's own NumPy statements; no code is shared with hobbyrenderer_amd/csrc/pt_motion.h."""
import numpy as np

import motion_reference as M

f32 = np.float32


def motion(scene, cb, prev_view, width, height, verts, prev_verts, traced):
    """The motion plane, float32 [H, W, 4], for the scene as it is now (`verts`: gbuffer_reference.unpacked_vertices(scene), `traced`:
    gbuffer_reference.trace of it) and the vertices of one frame ago (`prev_verts`: rows whose first three floats are the positions)."""
    out = np.zeros((height, width, 4), f32)
    ys, xs, rec, q, u, v = M._hit_triangles(scene, verts, traced)
    if len(ys) == 0:
        return out
    _, _, _, qprev, _, _ = M._hit_triangles(scene, np.ascontiguousarray(prev_verts, f32), traced)
    world, prev_world = np.asarray(rec["m_World"], f32), np.asarray(rec["m_PrevWorld"], f32)
    cur = [M._transform_point(p.astype(f32), world) for p in q]
    prev = [M._transform_point(p.astype(f32), prev_world) for p in qprev]
    u, v = u.astype(f32), v.astype(f32)
    win, w = M._project(M._interpolate(cur, u, v, f32(1.0)), cb["m_View"], f32)
    prev_win, prev_w = M._project(M._interpolate(prev, u, v, f32(1.0)), prev_view, f32)
    out[ys, xs] = np.concatenate([prev_win - win, (prev_w - w)[:, None], np.ones((len(ys), 1), f32)], 1)
    assert out.dtype == f32
    return out
