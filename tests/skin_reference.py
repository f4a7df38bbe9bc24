"""The vertex producer in front of the quantiser (hrpt_skin_vertices_* / hrpt_update_vertices_skinned) -- TEST
INFRASTRUCTURE: the NumPy float32 statement of csrc/pt_skin.h, which the host executor and the kernels equal bit for bit, and a float64
formulation that shares nothing with it (inverse transpose instead of cofactors, einsum instead of the written-out sums). The reference
renderer has no skinning, so the stage is defined by the project: parity unpinned by the reference."""
import numpy as np

from hobbyrenderer_amd import structs as S

f32 = np.float32


def _unit_or_keep(v):
    """v / sqrt(l2) where l2 = (v0 v0 + v1 v1) + v2 v2 is positive and finite, v itself elsewhere (only those rows are divided)."""
    l2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    ok = (l2 > 0) & np.isfinite(l2)
    out = v.copy()
    out[ok] = v[ok] / np.sqrt(l2[ok])[:, None]
    return out


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def blended_matrices(joints, weights, palette):
    """B = ((w0 M0 + w1 M1) + w2 M2) + w3 M3 per vertex, float32 [n, 3, 4]."""
    B = weights[:, 0, None, None] * palette[joints[:, 0]]
    for j in (1, 2, 3):
        B = B + weights[:, j, None, None] * palette[joints[:, j]]
    return B


def skin(base, joints=None, weights=None, joint_matrices=None, deltas=None, morph_weights=None):
    """The statement: S.VertexFloat records from the arrays native.skin_arrays() describes. Every array operation below is one float32
    operation per element, in the order csrc/pt_skin.h writes them."""
    base = np.asarray(base)
    p, n, t, s = base["pos"].copy(), base["normal"].copy(), base["tangent"][:, :3].copy(), base["tangent"][:, 3].copy()
    assert p.dtype == f32
    if deltas is not None:
        morph_weights = np.asarray(morph_weights, f32)
        deltas = np.asarray(deltas).reshape(len(morph_weights), len(base))
        for k, w in enumerate(morph_weights):
            if w == 0:                                  # +0 or -0: the target is skipped, whatever its deltas hold
                continue
            p = p + w * deltas[k]["pos"]
            n = n + w * deltas[k]["normal"]
            t = t + w * deltas[k]["tangent"]
    if joints is not None:
        joints, weights, palette = np.asarray(joints), np.asarray(weights, f32), np.asarray(joint_matrices, f32).reshape(-1, 3, 4)
        assert joints.max() < len(palette)
        B = blended_matrices(joints, weights, palette)

        def rows(v, translate):
            out = []
            for r in range(3):
                x = (B[:, r, 0] * v[:, 0] + B[:, r, 1] * v[:, 1]) + B[:, r, 2] * v[:, 2]
                out.append(x + B[:, r, 3] if translate else x)
            return np.stack(out, 1)

        b0, b1, b2 = B[:, 0, :3], B[:, 1, :3], B[:, 2, :3]
        c0, c1, c2 = _cross(b1, b2), _cross(b2, b0), _cross(b0, b1)
        det = (b0[:, 0] * c0[:, 0] + b0[:, 1] * c0[:, 1]) + b0[:, 2] * c0[:, 2]
        m = np.stack([(c[:, 0] * n[:, 0] + c[:, 1] * n[:, 1]) + c[:, 2] * n[:, 2] for c in (c0, c1, c2)], 1)
        mirrored = det < 0
        p, t = rows(p, True), rows(t, False)
        n = np.where(mirrored[:, None], -m, m)
        s = np.where(mirrored, -s, s)
    out = np.zeros(len(base), S.VertexFloat)
    out["pos"], out["normal"], out["uv"] = p, _unit_or_keep(n), base["uv"]
    out["tangent"][:, :3], out["tangent"][:, 3] = _unit_or_keep(t), s
    assert p.dtype == f32 and n.dtype == f32 and t.dtype == f32 and s.dtype == f32
    return out


def skin_float64(base, joints=None, weights=None, joint_matrices=None, deltas=None, morph_weights=None):
    """The same pose in float64 by other means: (pos, unit normal, unit tangent, handedness sign, condition numbers of the blended 3 x 3
    parts or None). Normals go through the inverse transpose, whose direction is the cofactor matrix's times sign(det); the statement's
    flip for det < 0 undoes exactly that sign."""
    base = np.asarray(base)
    p, n, t = [base[k].astype(np.float64) for k in ("pos", "normal", "tangent")]
    t, s = t[:, :3], t[:, 3].copy()
    if deltas is not None:
        w = np.asarray(morph_weights, np.float64)
        d = np.asarray(deltas).reshape(len(w), len(base))
        used = np.nonzero(w)[0]
        p = p + np.einsum("k,knc->nc", w[used], d["pos"][used].astype(np.float64))
        n = n + np.einsum("k,knc->nc", w[used], d["normal"][used].astype(np.float64))
        t = t + np.einsum("k,knc->nc", w[used], d["tangent"][used].astype(np.float64))
    cond = None
    if joints is not None:
        P = np.asarray(joint_matrices, np.float64).reshape(-1, 3, 4)
        B = np.einsum("nj,njrc->nrc", np.asarray(weights, np.float64), P[np.asarray(joints)])
        A = B[:, :, :3]
        p = np.einsum("nrc,nc->nr", A, p) + B[:, :, 3]
        n = np.einsum("ncr,nc->nr", np.linalg.inv(A), n)
        t = np.einsum("nrc,nc->nr", A, t)
        s = np.where(np.linalg.det(A) < 0, -s, s)
        cond = np.linalg.cond(A)
    return p, n / np.linalg.norm(n, axis=1, keepdims=True), t / np.linalg.norm(t, axis=1, keepdims=True), s, cond
