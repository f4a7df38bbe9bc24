"""The animation stage in NumPy, written from the reference's Scene::Update and EvaluateAnimSampler (src/Scene.cpp:345-570) and the
dynamic-node pass of Scene::FinalizeLoadedScene (src/Scene.cpp:220-273): a float32 statement with one rounding per operation that the
host executor and the gfx950 kernels reproduce bit for bit, and a float64 formulation that shares none of its arithmetic (textbook slerp
through arccos, matrix products in float64). The statement walks the animations and channels in the reference's order and lets later
writes overwrite earlier ones; it walks the nodes parents first, as m_DynamicNodeIndices does. Where the reference calls DirectXMath
(XMQuaternionSlerp's sine and arccosine approximations), the project defines its own deterministic functions: parity with DirectXMath is
unpinned. Weight channels, which the reference drops, write .x into morph-weight slots.

Tables are dicts of arrays in the layouts of hobbyrenderer_amd.structs (see anim_cases.py): samplers, channels, nodes, joints, key_times,
key_values, targets, node_instances, animation_count, morph_weight_count."""
import numpy as np

from hobbyrenderer_amd import structs as S

F = np.float32
SLERP_LINEAR_ABOVE = F(0.9995)


def advance(times, durations, dt):
    """The clock of Scene.cpp:427-432 in float32."""
    t = (np.asarray(times, F) + F(dt)).astype(F)
    d = np.asarray(durations, F)
    wrapped = np.fmod(t, np.where(d > 0, d, F(1)).astype(F)).astype(F)
    return np.where(d > 0, wrapped, t).astype(F)


def durations(tb):
    d = np.zeros(tb["animation_count"], F)
    for s in tb["samplers"]:
        if s["keyCount"]:
            d[s["animation"]] = max(d[s["animation"]], tb["key_times"][s["firstKey"] + s["keyCount"] - 1])
    return d


# ---- detmath.h's sine and the stage's arctangent, in float32 ----
def _sin(x):
    x = F(x)
    fn = np.floor(F(x * F(0.636619772367581343)) + F(0.5)).astype(F)
    q = int(fn)
    r = F(F(F(x - F(fn * F(1.5703125))) - F(fn * F(4.837512969970703125e-4))) - F(fn * F(7.54978995489188216e-8)))
    z = F(r * r)
    s = F(r + F(F(r * z) * F(F(-1.6666654611e-1) + F(z * F(F(8.3321608736e-3) + F(z * F(-1.9515295891e-4)))))))
    c = F(F(F(1) - F(F(0.5) * z)) + F(F(z * z) * F(F(4.166664568298827e-2) + F(z * F(F(-1.388731625493765e-3) + F(z * F(2.443315711809948e-5)))))))
    v = c if q & 1 else s
    return F(-v) if q & 2 else v


def _atan_first_quadrant(y, x):
    if not x > 0:
        return F(1.57079637)
    r, base = F(F(y) / F(x)), F(0)
    if r > F(2.41421366):
        base, r = F(1.57079637), F(-F(F(1) / r))
    elif r > F(0.414213568):
        base, r = F(0.785398185), F(F(r - F(1)) / F(r + F(1)))
    z = F(r * r)
    p = F(F(F(F(F(F(8.05374449538e-2) * z) - F(1.38776856032e-1)) * z) + F(1.99777106478e-1)) * z) - F(3.33329491539e-1)
    p = F(p)
    return F(base + F(F(F(p * z) * r) + r))


def _unit4(q):
    q = np.asarray(q, F)
    l2 = F(F(F(q[0] * q[0]) + F(q[1] * q[1])) + F(q[2] * q[2])) + F(q[3] * q[3])
    l2 = F(l2)
    if l2 > 0 and np.isfinite(l2):
        return (q / np.sqrt(l2)).astype(F)
    return q.copy()


def _slerp(v0, v1, a):
    q0, q1 = _unit4(v0), _unit4(v1)
    p = (q0 * q1).astype(F)
    dot = F(F(F(p[0] + p[1]) + p[2]) + p[3])
    if dot < 0:
        dot, q1 = F(-dot), (-q1).astype(F)
    if dot > SLERP_LINEAR_ABOVE:
        return (q0 + (a * (q1 - q0).astype(F)).astype(F)).astype(F)
    s = np.sqrt(F(F(1) - F(dot * dot))).astype(F)
    omega = _atan_first_quadrant(s, dot)
    w0 = F(_sin(F(F(F(1) - a) * omega)) / s)
    w1 = F(_sin(F(a * omega)) / s)
    return ((w0 * q0).astype(F) + (w1 * q1).astype(F)).astype(F)


def evaluate_sampler(tb, s, t):
    """EvaluateAnimSampler: the scan of the reference, not a binary search."""
    n, first = int(s["keyCount"]), int(s["firstKey"])
    times, values = tb["key_times"][first:first + n], tb["key_values"][first:first + n]
    t = F(t)
    if n == 1 or t <= times[0]:
        return values[0].copy()
    if t >= times[-1]:
        return values[-1].copy()
    k0 = 0
    for i in range(n - 1):
        if t >= times[i]:
            k0 = i
    k1 = k0 + 1
    d = F(times[k1] - times[k0])
    a = F(F(t - times[k0]) / d) if d > 0 else F(0)
    v0, v1 = values[k0], values[k1]
    kind = int(s["interpolation"])
    if kind == S.ANIM_STEP:
        return v0.copy()
    if kind == S.ANIM_SLERP:
        return _slerp(v0, v1, a)
    if kind == S.ANIM_CATMULLROM:
        p0 = values[k0 - 1 if k0 > 0 else k0]
        p3 = values[k1 + 1 if k1 < n - 1 else k1]
        a2 = F(a * a)
        a3 = F(a * a2)
        w0 = F(F(F(F(F(2) * a2) - a3) - a) * F(0.5))
        w1 = F(F(F(F(F(3) * a3) - F(F(5) * a2)) + F(2)) * F(0.5))
        w2 = F(F(F(F(F(4) * a2) - F(F(3) * a3)) + a) * F(0.5))
        w3 = F(F(a3 - a2) * F(0.5))
        return (((w0 * p0).astype(F) + (w1 * v0).astype(F)).astype(F) + ((w2 * v1).astype(F) + (w3 * p3).astype(F)).astype(F)).astype(F)
    return (v0 + (a * (v1 - v0).astype(F)).astype(F)).astype(F)


def _local(t, r, s):
    x, y, z, w = (F(c) for c in r)
    x2, y2, z2 = F(x + x), F(y + y), F(z + z)
    xx, yy, zz, xy, xz, yz = F(x * x2), F(y * y2), F(z * z2), F(x * y2), F(x * z2), F(y * z2)
    wx, wy, wz = F(w * x2), F(w * y2), F(w * z2)
    rot = np.array([[F(F(1) - yy) - zz, xy + wz, xz - wy], [xy - wz, F(F(1) - xx) - zz, yz + wx], [xz + wy, yz - wx, F(F(1) - xx) - yy]], F)
    m = np.zeros((4, 4), F)
    m[:3, :3] = (np.asarray(s, F)[:, None] * rot).astype(F)
    m[3, :3] = t
    m[3, 3] = 1
    return m


def _mul(a, b):
    """Row-vector product a . b, every entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3."""
    out = np.empty((a.shape[0], b.shape[1]), F)
    for i in range(a.shape[0]):
        out[i] = (((a[i, 0] * b[0]).astype(F) + (a[i, 1] * b[1]).astype(F)).astype(F) + (a[i, 2] * b[2]).astype(F)).astype(F) + (a[i, 3] * b[3]).astype(F)
    return out


def _parents_first(nodes):
    depth = np.zeros(len(nodes), np.int64)
    for i in range(len(nodes)):
        p, d = nodes["parent"][i], 0
        while p >= 0:
            p, d = nodes["parent"][p], d + 1
        depth[i] = d
    return np.argsort(depth, kind="stable")


def poses(tb, times):
    """Scene::Update up to the node worlds: (translation, rotation, scale, dirty) per node and the weights, after all channels applied
    in (animation, channel) order."""
    nodes = tb["nodes"]
    T, R, Sc = nodes["translation"].copy(), nodes["rotation"].copy(), nodes["scale"].copy()
    dirty = np.zeros(len(nodes), bool)
    weights = np.zeros(tb["morph_weight_count"], F)
    for a in range(tb["animation_count"]):
        for ch in tb["channels"]:
            s = tb["samplers"][ch["sampler"]]
            if s["animation"] != a or s["keyCount"] == 0:
                continue
            v = evaluate_sampler(tb, s, times[a])
            for target in tb["targets"][ch["firstTarget"]:ch["firstTarget"] + ch["targetCount"]]:
                if ch["path"] == S.ANIM_PATH_WEIGHTS:
                    weights[target] = v[0]
                    continue
                dirty[target] = True
                if ch["path"] == S.ANIM_PATH_TRANSLATION:
                    T[target] = v[:3]
                elif ch["path"] == S.ANIM_PATH_ROTATION:
                    R[target] = _unit4(v)
                else:
                    Sc[target] = v[:3]
    return T, R, Sc, dirty, weights


def animate(tb, times, instances=None):
    """The statement: (instances or None, palette [joints, 3, 4], weights, node worlds [nodes, 4, 4]) in float32."""
    nodes = tb["nodes"]
    T, R, Sc, dirty, weights = poses(tb, times)
    worlds = nodes["baseWorld"].copy()
    out = None if instances is None else np.array(instances, S.PerInstanceData, copy=True)
    if out is not None:
        out["m_PrevWorld"] = out["m_World"]
    for n in _parents_first(nodes):
        p = nodes["parent"][n]
        if p >= 0 and dirty[p]:
            dirty[n] = True
        if not dirty[n]:
            continue
        local = _local(T[n], R[n], Sc[n])
        worlds[n] = _mul(local, worlds[p]) if p >= 0 else local
        if out is not None:
            for k in range(nodes["instanceCount"][n]):
                out["m_World"][tb["node_instances"][nodes["firstInstance"][n] + k]] = worlds[n]
    palette = np.zeros((len(tb["joints"]), 3, 4), F)
    for j, joint in enumerate(tb["joints"]):
        palette[j] = _mul(joint["inverseBind"], worlds[joint["node"]])[:, :3].T
    return out, palette, weights, worlds


# ---- the independent float64 formulation ----
def _slerp64(v0, v1, a, linear):
    """Textbook slerp through arccos; `linear` is the definition's branch above the threshold, decided by the caller as float32 decides it."""
    q0, q1 = np.asarray(v0, np.float64), np.asarray(v1, np.float64)
    q0, q1 = q0 / np.linalg.norm(q0), q1 / np.linalg.norm(q1)
    d = float(q0 @ q1)
    if d < 0:
        d, q1 = -d, -q1
    if linear:
        return q0 + a * (q1 - q0)
    omega = np.arccos(min(d, 1.0))
    return (np.sin((1 - a) * omega) * q0 + np.sin(a * omega) * q1) / np.sin(omega)


def animate_float64(tb, times):
    """(palette, node worlds) in float64: samplers in float64 from the float32 keys and times, rotation matrices from the textbook
    formula, matrix products by numpy.matmul."""
    nodes = tb["nodes"]
    T, R, Sc = (nodes[k].astype(np.float64) for k in ("translation", "rotation", "scale"))
    dirty = np.zeros(len(nodes), bool)
    for a in range(tb["animation_count"]):
        for ch in tb["channels"]:
            s = tb["samplers"][ch["sampler"]]
            if s["animation"] != a or s["keyCount"] == 0 or ch["path"] == S.ANIM_PATH_WEIGHTS:
                continue
            n, first = int(s["keyCount"]), int(s["firstKey"])
            kt, kv = tb["key_times"][first:first + n].astype(np.float64), tb["key_values"][first:first + n].astype(np.float64)
            t = float(times[a])
            if n == 1 or t <= kt[0]:
                v = kv[0]
            elif t >= kt[-1]:
                v = kv[-1]
            else:
                k0 = max(i for i in range(n - 1) if t >= kt[i])
                d = kt[k0 + 1] - kt[k0]
                al = (t - kt[k0]) / d if d > 0 else 0.0
                kind = int(s["interpolation"])
                if kind == S.ANIM_STEP:
                    v = kv[k0]
                elif kind == S.ANIM_SLERP:
                    q0, q1 = _unit4(kv[k0].astype(F)), _unit4(kv[k0 + 1].astype(F))
                    dot = F(F(F(q0[0] * q1[0]) + F(q0[1] * q1[1])) + F(q0[2] * q1[2])) + F(q0[3] * q1[3])
                    v = _slerp64(kv[k0], kv[k0 + 1], al, abs(dot) > SLERP_LINEAR_ABOVE)
                elif kind == S.ANIM_CATMULLROM:
                    p0, p3 = kv[max(k0 - 1, 0)], kv[min(k0 + 2, n - 1)]
                    v = 0.5 * ((-al ** 3 + 2 * al ** 2 - al) * p0 + (3 * al ** 3 - 5 * al ** 2 + 2) * kv[k0] + (-3 * al ** 3 + 4 * al ** 2 + al) * kv[k0 + 1]
                               + (al ** 3 - al ** 2) * p3)
                else:
                    v = kv[k0] + al * (kv[k0 + 1] - kv[k0])
            for target in tb["targets"][ch["firstTarget"]:ch["firstTarget"] + ch["targetCount"]]:
                dirty[target] = True
                if ch["path"] == S.ANIM_PATH_TRANSLATION:
                    T[target] = v[:3]
                elif ch["path"] == S.ANIM_PATH_ROTATION:
                    R[target] = v / np.linalg.norm(v) if np.linalg.norm(v) > 0 else v
                else:
                    Sc[target] = v[:3]
    worlds = nodes["baseWorld"].astype(np.float64)
    for n in _parents_first(nodes):
        p = nodes["parent"][n]
        if p >= 0 and dirty[p]:
            dirty[n] = True
        if not dirty[n]:
            continue
        x, y, z, w = R[n]
        rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w)],
                        [2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w)],
                        [2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y)]])
        local = np.eye(4)
        local[:3, :3] = np.diag(Sc[n]) @ rot
        local[3, :3] = T[n]
        worlds[n] = local @ worlds[p] if p >= 0 else local
    palette = np.zeros((len(tb["joints"]), 3, 4))
    for j, joint in enumerate(tb["joints"]):
        palette[j] = (joint["inverseBind"].astype(np.float64) @ worlds[joint["node"]])[:, :3].T
    return palette, worlds
