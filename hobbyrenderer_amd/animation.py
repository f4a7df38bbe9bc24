"""Animation tables from a parsed glTF 2.0 document, for native.Animation (hrpt_animation_create): tables_from_gltf(doc, buffers).
Pure Python and NumPy; the C++ loader keeps ignoring `animations` and `skins`.

Coordinates follow the project's glTF loader (host/GltfLoader.cpp): glTF is right-handed, the scene left-handed, by
z -> -z. A translation negates z, a rotation quaternion negates x and y, a scale stays; a node given as a matrix is decomposed first, as
the loader does; a 4 x 4 matrix stored column-major for column vectors, read as 16 floats row by row, is already the row-vector matrix,
and its z-flip negates the six entries that couple z with another axis. The rest pose (HrptAnimNode::baseWorld) is computed as the
loader computes node worlds -- local from TRS, world = local . parent with products accumulated in float64 and rounded once -- so that
it equals, to the bit, the world matrices the loader put into the scene's instances.

Instances are numbered as the loader numbers them (Scene::FinalizeLoadedScene): one per (mesh node, primitive) in node order, bucketed
opaque, masked, transparent by the material's alphaMode, nodes that carry a light after the others within a bucket."""
import numpy as np

from . import structs as S

f32 = np.float32
_PATHS = {"translation": S.ANIM_PATH_TRANSLATION, "rotation": S.ANIM_PATH_ROTATION, "scale": S.ANIM_PATH_SCALE, "weights": S.ANIM_PATH_WEIGHTS}
_INTERPOLATIONS = {"STEP": S.ANIM_STEP, "LINEAR": S.ANIM_LINEAR, "CUBICSPLINE": S.ANIM_CUBICSPLINE}
_COMPONENTS = {5120: ("i1", 127.0), 5121: ("u1", 255.0), 5122: ("<i2", 32767.0), 5123: ("<u2", 65535.0), 5125: ("<u4", None), 5126: ("<f4", None)}
_WIDTHS = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}


def read_accessor(doc, buffers, index):
    """Accessor `index` as float32 [count, components]; normalised integers are converted as the glTF specification says."""
    acc = doc["accessors"][index]
    view = doc["bufferViews"][acc["bufferView"]]
    dtype, scale = _COMPONENTS[acc["componentType"]]
    width = _WIDTHS[acc["type"]]
    item = np.dtype(dtype).itemsize * width
    stride = view.get("byteStride") or item
    start = view.get("byteOffset", 0) + acc.get("byteOffset", 0)
    raw = np.frombuffer(buffers[view.get("buffer", 0)], np.uint8)
    rows = np.stack([raw[start + k * stride:start + k * stride + item] for k in range(acc["count"])]) if acc["count"] else np.zeros((0, item), np.uint8)
    out = np.ascontiguousarray(rows).view(dtype).reshape(acc["count"], width).astype(np.float64)
    if acc.get("normalized") and scale:
        out = np.maximum(out / scale, -1.0)
    return out.astype(f32)


# ---- the loader's node arithmetic (float32, DirectXMath conventions) ----
def _matrix_from_trs(t, q, s):
    x, y, z, w = (f32(v) for v in q)
    two, one = f32(2), f32(1)
    r = np.identity(4, dtype=f32)
    r[0, 0] = one - two * f32(f32(y * y) + f32(z * z)); r[0, 1] = two * f32(f32(x * y) + f32(z * w)); r[0, 2] = two * f32(f32(x * z) - f32(y * w))
    r[1, 0] = two * f32(f32(x * y) - f32(z * w)); r[1, 1] = one - two * f32(f32(x * x) + f32(z * z)); r[1, 2] = two * f32(f32(y * z) + f32(x * w))
    r[2, 0] = two * f32(f32(x * z) + f32(y * w)); r[2, 1] = two * f32(f32(y * z) - f32(x * w)); r[2, 2] = one - two * f32(f32(x * x) + f32(y * y))
    for i in range(3):
        r[i, :3] = (r[i, :3] * f32(s[i])).astype(f32)
    r[3, :3] = t
    return r


def _decompose(m):
    """Scale, rotation quaternion, translation of a row-vector matrix (XMMatrixDecompose as the loader restates it)."""
    m = np.asarray(m, f32)
    t = m[3, :3].copy()
    ln = [np.sqrt(f32(f32(f32(m[i, 0] * m[i, 0]) + f32(m[i, 1] * m[i, 1])) + f32(m[i, 2] * m[i, 2]))) for i in range(3)]
    r = np.zeros((3, 3), f32)
    for i in range(3):
        r[i] = (m[i, :3] / ln[i]).astype(f32) if ln[i] > 0 else np.identity(3, dtype=f32)[i]
    c = lambda a, b: f32(a * b)  # noqa: E731
    det = f32(f32(c(r[0, 0], f32(c(r[1, 1], r[2, 2]) - c(r[1, 2], r[2, 1]))) - c(r[0, 1], f32(c(r[1, 0], r[2, 2]) - c(r[1, 2], r[2, 0])))) +
              c(r[0, 2], f32(c(r[1, 0], r[2, 1]) - c(r[1, 1], r[2, 0]))))
    if det < 0:
        a = (0 if ln[0] >= ln[2] else 2) if ln[0] >= ln[1] else (1 if ln[1] >= ln[2] else 2)
        ln[a] = -ln[a]; r[a] = -r[a]
    tr = f32(f32(r[0, 0] + r[1, 1]) + r[2, 2])
    if tr > 0:
        s = f32(np.sqrt(f32(tr + f32(1))) * f32(2)); w = f32(f32(0.25) * s)
        x = f32(f32(r[1, 2] - r[2, 1]) / s); y = f32(f32(r[2, 0] - r[0, 2]) / s); z = f32(f32(r[0, 1] - r[1, 0]) / s)
    elif r[0, 0] > r[1, 1] and r[0, 0] > r[2, 2]:
        s = f32(np.sqrt(f32(f32(f32(f32(1) + r[0, 0]) - r[1, 1]) - r[2, 2])) * f32(2))
        w = f32(f32(r[1, 2] - r[2, 1]) / s); x = f32(f32(0.25) * s); y = f32(f32(r[0, 1] + r[1, 0]) / s); z = f32(f32(r[0, 2] + r[2, 0]) / s)
    elif r[1, 1] > r[2, 2]:
        s = f32(np.sqrt(f32(f32(f32(f32(1) + r[1, 1]) - r[0, 0]) - r[2, 2])) * f32(2))
        w = f32(f32(r[2, 0] - r[0, 2]) / s); x = f32(f32(r[0, 1] + r[1, 0]) / s); y = f32(f32(0.25) * s); z = f32(f32(r[1, 2] + r[2, 1]) / s)
    else:
        s = f32(np.sqrt(f32(f32(f32(f32(1) + r[2, 2]) - r[0, 0]) - r[1, 1])) * f32(2))
        w = f32(f32(r[0, 1] - r[1, 0]) / s); x = f32(f32(r[0, 2] + r[2, 0]) / s); y = f32(f32(r[1, 2] + r[2, 1]) / s); z = f32(f32(0.25) * s)
    return np.array(ln, f32), np.array([x, y, z, w], f32), t


def _matmul(a, b):
    """hobbyrt::MatrixMultiply: float64 accumulation, one rounding to float32."""
    return np.array([[f32(sum(float(a[i, k]) * float(b[k, j]) for k in range(4))) for j in range(4)] for i in range(4)], f32)


def _flip_z(m):
    m = np.array(m, f32).reshape(4, 4)
    for i, j in ((0, 2), (1, 2), (3, 2), (2, 0), (2, 1), (2, 3)):
        m[i, j] = -m[i, j]
    return m


def node_trs(n):
    """(translation, rotation, scale) of a glTF node in the scene's left-handed space."""
    t, q, s = np.zeros(3, f32), np.array([0, 0, 0, 1], f32), np.ones(3, f32)
    if len(n.get("matrix", [])) == 16:
        s, q, t = _decompose(np.array(n["matrix"], f32).reshape(4, 4))
        t[2] = -t[2]; q[0] = -q[0]; q[1] = -q[1]
        return t, q, s
    if len(n.get("translation", [])) == 3:
        t = np.array([n["translation"][0], n["translation"][1], -f32(n["translation"][2])], f32)
    if len(n.get("scale", [])) == 3:
        s = np.array(n["scale"], f32)
    if len(n.get("rotation", [])) == 4:
        r = n["rotation"]
        q = np.array([-f32(r[0]), -f32(r[1]), r[2], r[3]], f32)
    return t, q, s


def instance_order(doc):
    """[(node, primitive)] in the order of the scene's instances."""
    buckets = [[] for _ in range(6)]
    materials = doc.get("materials", [])
    for ni, n in enumerate(doc.get("nodes", [])):
        if "mesh" not in n:
            continue
        dynamic = "light" in n.get("extensions", {}).get("KHR_lights_punctual", {})
        for pi, prim in enumerate(doc["meshes"][n["mesh"]].get("primitives", [])):
            mode = materials[prim["material"]].get("alphaMode", "OPAQUE") if 0 <= prim.get("material", -1) < len(materials) else "OPAQUE"
            buckets[{"OPAQUE": 0, "MASK": 2}.get(mode, 4) + (1 if dynamic else 0)].append((ni, pi))
    return [x for b in buckets for x in b]


def tables_from_gltf(doc, buffers):
    """The keywords of native.Animation / native.animation_desc for all `animations` of the document (animation index = position in the
    file) and all `skins` (joints concatenated in file order), plus two maps the caller needs: "weight_slots" {node: (first slot, count)}
    for every node a weights channel targets, and "skin_joints" [(first joint, count)] per skin. CUBICSPLINE samplers keep the value
    element of each (in-tangent, value, out-tangent) triplet, and the stage interpolates them linearly, as the reference does. A weights
    sampler with N values per key becomes N samplers, one per slot. Channels without a target node are dropped."""
    nodes_json = doc.get("nodes", [])
    nodes = np.zeros(len(nodes_json), S.AnimNode)
    nodes["parent"] = -1
    for k, n in enumerate(nodes_json):
        for c in n.get("children", []):
            nodes["parent"][c] = k
        nodes["translation"][k], nodes["rotation"][k], nodes["scale"][k] = node_trs(n)
    world = {}

    def rest(k):
        if k not in world:
            local = _matrix_from_trs(nodes["translation"][k], nodes["rotation"][k], nodes["scale"][k])
            p = int(nodes["parent"][k])
            world[k] = _matmul(local, rest(p) if p >= 0 else np.identity(4, dtype=f32))
        return world[k]
    for k in range(len(nodes)):
        nodes["baseWorld"][k] = rest(k)
    node_instances = []
    order = instance_order(doc)
    for k in range(len(nodes)):
        mine = [i for i, (ni, _) in enumerate(order) if ni == k]
        nodes["firstInstance"][k], nodes["instanceCount"][k] = len(node_instances), len(mine)
        node_instances += mine

    samplers, channels, key_times, key_values, targets = [], [], [], [], []
    weight_slots, slot_count = {}, 0

    def add_sampler(interpolation, times, values, animation):
        samplers.append((interpolation, len(key_times), len(times), animation))
        key_times.extend(times.tolist())
        key_values.extend(values.tolist())
        return len(samplers) - 1

    for ai, anim in enumerate(doc.get("animations", [])):
        for ch in anim.get("channels", []):
            target = ch.get("target", {})
            if "node" not in target or target.get("path") not in _PATHS:
                continue
            node, path = target["node"], _PATHS[target["path"]]
            smp = anim["samplers"][ch["sampler"]]
            kind = smp.get("interpolation", "LINEAR")
            times = read_accessor(doc, buffers, smp["input"]).reshape(-1)
            out = read_accessor(doc, buffers, smp["output"])
            rows = out.reshape(len(times), -1)                         # one row per key
            if kind == "CUBICSPLINE":                                   # (in-tangents, values, out-tangents) per key: the values
                rows = rows.reshape(len(times), 3, -1)[:, 1, :]
            values = np.zeros((len(times), 4), f32)
            if path == S.ANIM_PATH_WEIGHTS:
                per = rows
                first, count = weight_slots.setdefault(node, (slot_count, per.shape[1]))
                slot_count = max(slot_count, first + count)
                for k in range(count):
                    values = np.zeros((len(times), 4), f32)
                    values[:, 0] = per[:, k]
                    channels.append((path, add_sampler(_INTERPOLATIONS[kind], times, values, ai), len(targets), 1))
                    targets.append(first + k)
                continue
            values[:, :rows.shape[1]] = rows
            if path == S.ANIM_PATH_TRANSLATION:
                values[:, 2] = -values[:, 2]
            elif path == S.ANIM_PATH_ROTATION:
                values[:, :2] = -values[:, :2]
            channels.append((path, add_sampler(_INTERPOLATIONS[kind], times, values, ai), len(targets), 1))
            targets.append(node)

    joints, skin_joints = [], []
    for skin in doc.get("skins", []):
        ibm = read_accessor(doc, buffers, skin["inverseBindMatrices"]) if "inverseBindMatrices" in skin else None
        skin_joints.append((len(joints), len(skin["joints"])))
        for k, node in enumerate(skin["joints"]):
            joints.append((node, _flip_z(ibm[k]) if ibm is not None else np.identity(4, dtype=f32)))
    return dict(samplers=np.array(samplers, S.AnimSampler) if samplers else np.zeros(0, S.AnimSampler),
                channels=np.array(channels, S.AnimChannel) if channels else np.zeros(0, S.AnimChannel), nodes=nodes,
                joints=np.array(joints, S.AnimJoint) if joints else np.zeros(0, S.AnimJoint), key_times=np.array(key_times, f32),
                key_values=np.array(key_values, f32).reshape(-1, 4), targets=np.array(targets, np.uint32), node_instances=np.array(node_instances, np.uint32),
                animation_count=len(doc.get("animations", [])), morph_weight_count=slot_count), dict(weight_slots=weight_slots, skin_joints=skin_joints)
