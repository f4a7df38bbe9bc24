"""Inputs the skinning tests share (tests/test_skin_cpu.py, tests/test_skin_gpu.py) -- TEST INFRASTRUCTURE: the 4 096-vertex random pose,
the edge rows of the definition, palettes of a given size and gentle poses for the scenes the fused path is rendered on. A case is the
dict of keyword arguments native.skin_vertices_host and skin_reference.skin take."""
import numpy as np

from hobbyrenderer_amd import structs as S

f32 = np.float32
COUNT = 4096
MORPH_WEIGHTS = (0.25, 0.0, 0.7)            # one exactly zero: its target is skipped


def _quat_matrix(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def palette(joint_count, seed=3, mirror_every=5):
    """joint_count random rotations with per-axis scales in [0.5, 2] and translations in [-3, 3]; every mirror_every-th joint mirrored."""
    r = np.random.default_rng(seed)
    P = np.zeros((joint_count, 3, 4))
    for j in range(joint_count):
        q = r.normal(size=4)
        q /= np.linalg.norm(q)
        s = r.uniform(0.5, 2.0, 3)
        if mirror_every and j % mirror_every == mirror_every - 1:
            s[0] = -s[0]
        P[j, :, :3] = _quat_matrix(q) @ np.diag(s)
        P[j, :, 3] = r.uniform(-3, 3, 3)
    return P.astype(f32)


def bind_pose(count, rng):
    """Random S.VertexFloat records with unit normals, unit tangents orthogonal to them and a handedness sign of +-1."""
    v = np.zeros(count, S.VertexFloat)
    v["pos"] = rng.uniform(-10, 10, (count, 3))
    n = rng.normal(size=(count, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    t = np.cross(n, rng.normal(size=(count, 3)))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    v["normal"], v["tangent"][:, :3] = n, t
    v["tangent"][:, 3] = np.where(rng.random(count) < 0.5, 1, -1)
    return v, rng


def influences(count, joint_count, rng):
    """Four random joints per vertex, 30 % of the weights zero, normalised in float64 and then cast."""
    joints = rng.integers(0, joint_count, (count, 4)).astype(np.uint16)
    w = rng.random((count, 4))
    w[rng.random((count, 4)) < 0.3] = 0
    w[:, 0] += 0.05
    w /= w.sum(1, keepdims=True)
    return joints, w.astype(f32)


def morph_targets(count, rng, weights=MORPH_WEIGHTS):
    d = np.zeros((len(weights), count), S.SkinMorphDelta)
    x = (rng.normal(size=(len(weights), count, 9)) * 0.1).astype(f32)
    d["pos"], d["normal"], d["tangent"] = x[..., 0:3], x[..., 3:6], x[..., 6:9]
    return d, np.array(weights, f32)


def random_case(count=COUNT, joint_count=64, seed=7, target_weights=MORPH_WEIGHTS):
    """The case of DESIGN.md section 22: 4 096 vertices, 64 joints, three targets with weights (0.25, 0, 0.7). uv random. The last joint
    of the palette is used at least once."""
    rng = np.random.default_rng(seed)
    base, rng = bind_pose(count, rng)
    joints, weights = influences(count, joint_count, rng)
    joints[0, 0] = joint_count - 1
    deltas, mw = morph_targets(count, rng, target_weights)
    base["uv"] = rng.uniform(-2, 2, (count, 2))
    return dict(base=base, joints=joints, weights=weights, joint_matrices=palette(joint_count), deltas=deltas, morph_weights=mw)


def select(case, count=None, skin=True, morph=True, targets=None):
    """The first `count` vertices of a case, without its joints and / or with only its first `targets` morph targets."""
    n = len(case["base"]) if count is None else count
    out = dict(base=case["base"][:n])
    if skin:
        out.update(joints=case["joints"][:n], weights=case["weights"][:n], joint_matrices=case["joint_matrices"])
    targets = len(case["morph_weights"]) if targets is None else targets
    if morph and targets:
        out.update(deltas=np.ascontiguousarray(case["deltas"][:targets, :n]), morph_weights=case["morph_weights"][:targets])
    return out


EDGE_SIGNS = [1.0, -1.0, 0.0, -0.0]
# (joints, weights): palette of edge_case() is 0 identity, 1 zero 3 x 3 block (a translation alone), 2 mirror in x, 3 a rotation with scales
EDGE_INFLUENCES = [((0, 0, 0, 0), (1, 0, 0, 0)),              # identity
                   ((1, 1, 1, 1), (1, 0, 0, 0)),              # singular: cofactors and B t are zero, the normal and tangent stay zero vectors
                   ((2, 0, 0, 0), (1, 0, 0, 0)),              # mirrored: the normal and tangent[3] are negated
                   ((0, 3, 3, 0), (0.3, 0.3, 0.3, 0.3)),      # weights summing to 1.2: used as given
                   ((3, 2, 0, 1), (0.5, 0.25, 0.125, 0.0625)),
                   ((2, 3, 2, 3), (0.45, 0.05, 0.45, 0.05))]  # mostly mirror


def edge_case():
    """The edge rows: every EDGE_INFLUENCES entry x every tangent sign x (a unit base normal, a zero-length base normal), with two morph
    targets: weight 0.5, and weight -0.0 on deltas that hold inf (skipped: no 0 * inf)."""
    rng = np.random.default_rng(11)
    rows = [(i, s, z) for i in EDGE_INFLUENCES for s in EDGE_SIGNS for z in (False, True)]
    base, rng = bind_pose(len(rows), rng)
    joints, weights = np.zeros((len(rows), 4), np.uint16), np.zeros((len(rows), 4), f32)
    for k, ((j, w), s, zero) in enumerate(rows):
        joints[k], weights[k], base["tangent"][k, 3] = j, w, s
        if zero:
            base["normal"][k] = 0
    P = palette(4, seed=5, mirror_every=0)
    P[0] = np.eye(4, dtype=f32)[:3]
    P[1, :, :3] = 0
    P[2] = np.eye(4, dtype=f32)[:3]
    P[2, 0, 0], P[2, :, 3] = -1, (0.5, -0.25, 2)
    deltas, mw = morph_targets(len(rows), rng, (0.5, -0.0))
    for f in ("pos", "normal", "tangent"):
        deltas[f][1] = np.inf
    # a zero-length normal must stay one through the morph: no normal delta on those rows
    deltas["normal"][0][[z for _, _, z in rows]] = 0
    return dict(base=base, joints=joints, weights=weights, joint_matrices=P, deltas=deltas, morph_weights=mw)


def gentle_pose(base, joint_count, seed, amplitude=0.05, targets=2):
    """A pose that keeps a scene recognisable: joints rotate by at most 0.1 rad, scale within 3 % and move by `amplitude`; no mirroring."""
    rng = np.random.default_rng(seed)
    n = len(base)
    P = np.zeros((joint_count, 3, 4))
    for j in range(joint_count):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        half = 0.5 * rng.uniform(-0.1, 0.1)
        P[j, :, :3] = _quat_matrix((np.cos(half), *(np.sin(half) * axis))) @ np.diag(rng.uniform(0.97, 1.03, 3))
        P[j, :, 3] = rng.uniform(-amplitude, amplitude, 3)
    joints, weights = influences(n, joint_count, rng)
    joints[0, 0] = joint_count - 1
    mw = ((0.6, 0.0, 0.3) * 2)[:targets]
    deltas, mw = morph_targets(n, rng, mw)
    deltas["pos"] *= f32(amplitude)
    return dict(base=np.ascontiguousarray(base), joints=joints, weights=weights, joint_matrices=P.astype(f32), deltas=deltas, morph_weights=mw)
