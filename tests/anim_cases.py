"""Generated animation tables with fixed seeds for the tests of the animation stage (tests/test_anim_cpu.py, tests/test_anim_gpu.py):
every edge of the definition in csrc/pt_anim.h at the smallest size that reaches it. A case is a dict: "tables" (the keywords of
native.animation_desc, which are also what anim_reference reads), "times" (a list of time vectors, one time per animation, each evaluated)
and "instance_count" (the scene instances the tables index, a few more than they list)."""
import numpy as np

from hobbyrenderer_amd import structs as S
import anim_reference as R

F = np.float32
INTERPOLATIONS = (S.ANIM_STEP, S.ANIM_LINEAR, S.ANIM_CUBICSPLINE, S.ANIM_CATMULLROM, S.ANIM_SLERP)
PATHS = (S.ANIM_PATH_TRANSLATION, S.ANIM_PATH_ROTATION, S.ANIM_PATH_SCALE, S.ANIM_PATH_WEIGHTS)


def random_quaternion(rng):
    q = rng.standard_normal(4)
    return (q / np.linalg.norm(q)).astype(F)


class Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.nodes, self.samplers, self.channels, self.joints = [], [], [], []
        self.key_times, self.key_values, self.targets = [], [], []
        self.instances_of = []
        self.animation_count, self.morph_weight_count = 1, 0

    def trs(self, negative_scale=False):
        scale = self.rng.uniform(0.6, 1.5, 3)
        if negative_scale:
            scale[1] = -scale[1]
        return self.rng.uniform(-1, 1, 3).astype(F), random_quaternion(self.rng), scale.astype(F)

    def node(self, parent=-1, trs=None, base_world=None, instances=0):
        """A node whose baseWorld is its rest pose composed by the statement's arithmetic, unless base_world is given."""
        t, r, s = trs if trs is not None else self.trs()
        if base_world is None:
            local = R._local(t, r, s)
            base_world = R._mul(local, self.nodes[parent]["baseWorld"]) if parent >= 0 else local
        n = np.zeros((), S.AnimNode)
        n["parent"], n["translation"], n["rotation"], n["scale"], n["baseWorld"] = parent, t, r, s, base_world
        self.nodes.append(n)
        self.instances_of.append(instances)
        return len(self.nodes) - 1

    def sampler(self, interpolation, times, values, animation=0):
        times, values = np.asarray(times, F).reshape(-1), np.asarray(values, F).reshape(-1, 4)
        assert len(times) == len(values)
        self.samplers.append((interpolation, len(self.key_times), len(times), animation))
        self.key_times += list(times)
        self.key_values += list(values)
        return len(self.samplers) - 1

    def channel(self, path, sampler, targets):
        self.channels.append((path, sampler, len(self.targets), len(targets)))
        self.targets += list(targets)

    def joint(self, node, inverse_bind=None):
        j = np.zeros((), S.AnimJoint)
        j["node"] = node
        j["inverseBind"] = inverse_bind if inverse_bind is not None else (np.eye(4) + 0.3 * self.rng.uniform(-1, 1, (4, 4)) * [1, 1, 1, 0]).astype(F)
        self.joints.append(j)

    def tables(self, extra_instances=2):
        """Instance indices are dealt from a permutation, so that the closed range of the composed ones holds static and unlisted records."""
        total = sum(self.instances_of) + extra_instances
        deal = list(np.random.default_rng(99).permutation(total))
        node_instances = []
        nodes = np.array(self.nodes, S.AnimNode) if self.nodes else np.zeros(0, S.AnimNode)
        for k, count in enumerate(self.instances_of):
            nodes["firstInstance"][k], nodes["instanceCount"][k] = len(node_instances), count
            node_instances += [deal.pop() for _ in range(count)]
        tables = dict(samplers=np.array(self.samplers, S.AnimSampler) if self.samplers else np.zeros(0, S.AnimSampler),
                      channels=np.array(self.channels, S.AnimChannel) if self.channels else np.zeros(0, S.AnimChannel), nodes=nodes,
                      joints=np.array(self.joints, S.AnimJoint) if self.joints else np.zeros(0, S.AnimJoint),
                      key_times=np.array(self.key_times, F), key_values=np.array(self.key_values, F).reshape(-1, 4),
                      targets=np.array(self.targets, np.uint32), node_instances=np.array(node_instances, np.uint32),
                      animation_count=self.animation_count, morph_weight_count=self.morph_weight_count)
        return tables, total


def key_values(rng, path, n, unnormalised=False):
    if path == S.ANIM_PATH_ROTATION:
        v = np.array([random_quaternion(rng) for _ in range(n)], F).reshape(n, 4)
        return (v * rng.uniform(0.3, 3.0, (n, 1))).astype(F) if unnormalised else v
    v = rng.uniform(-1.5, 1.5, (n, 4)).astype(F)
    if path == S.ANIM_PATH_SCALE:
        v[:, :3] = rng.uniform(0.5, 1.6, (n, 3))
    return v


KEYS_37 = np.sort(np.random.default_rng(7).uniform(0.5, 4.0, 37)).astype(F)
KEYS_37[11] = KEYS_37[10]                                # two equal key times
KEYS_2 = np.array([0.5, 3.0], F)


def sampler_case():
    """Every interpolation on every path with 0, 1, 2 and 37 keys, each on a node (or weight slot) of its own; times below the first key,
    above the last, on a key (an equal pair among them), between keys, and inside the first and the last segment of the 37-key samplers
    (Catmull-Rom's clamped neighbours). Rotation keys of the 37-key samplers are not normalised."""
    b = Builder(11)
    for interpolation in INTERPOLATIONS:
        for path in PATHS:
            for n in (0, 1, 2, 37):
                times = {0: [], 1: [1.25], 2: KEYS_2, 37: KEYS_37}[n]
                s = b.sampler(interpolation, times, key_values(b.rng, path, n, unnormalised=(n == 37)))
                if path == S.ANIM_PATH_WEIGHTS:
                    b.channel(path, s, [b.morph_weight_count])
                    b.morph_weight_count += 1
                else:
                    b.channel(path, s, [b.node(instances=1 if n == 2 else 0)])
    tables, count = b.tables()
    times = [0.25, 10.0, 0.5, 3.0, float(KEYS_37[5]), float(KEYS_37[10]), 1.7, float((KEYS_37[0] + KEYS_37[1]) / 2), float((KEYS_37[35] + KEYS_37[36]) / 2)]
    return dict(tables=tables, times=[[t] for t in times], instance_count=count)


def slerp_case():
    """Slerp between two keys at alpha 0.3: opposite hemispheres, nearly parallel on both sides of the 0.9995 threshold, nearly opposite,
    orthogonal, equal, and unnormalised keys."""
    b = Builder(12)
    rng = b.rng

    def rotated(q, angle):                                # q turned by `angle` in a random plane of the 3-sphere: dot(q, result) = cos(angle)
        o = rng.standard_normal(4)
        o -= (o @ q) * q
        o /= np.linalg.norm(o)
        return np.cos(angle) * q + np.sin(angle) * o

    threshold = np.arccos(0.9995)
    for angle, scale in [(2.0, 1), (np.pi - 2.0, -1), (threshold * 0.98, 1), (threshold * 1.02, 1), (threshold * 0.98, -1), (threshold * 1.02, -1),
                         (np.pi - 1e-3, 1), (3.0, 1), (np.pi / 2, 1), (0.0, 1), (1e-4, 1), (1.0, 3.7), (1.0, -0.2)]:
        q0 = random_quaternion(rng).astype(np.float64)
        q1 = rotated(q0, angle) * scale
        s = b.sampler(S.ANIM_SLERP, [0.0, 1.0], [q0 * (2.5 if abs(scale) != 1 else 1), q1])
        b.channel(S.ANIM_PATH_ROTATION, s, [b.node(instances=1)])
    tables, count = b.tables()
    return dict(tables=tables, times=[[0.3], [0.5], [0.999]], instance_count=count)


def hierarchy_case(wide=300):
    """One table with every hierarchy and channel rule. `wide`: the children of one animated parent, one depth group (300: more than one
    256-lane workgroup, and more composed nodes than the single-launch compose kernel takes)."""
    b = Builder(13)
    b.animation_count = 3
    rng = b.rng
    lin = lambda path, n, animation=0: b.sampler(S.ANIM_LINEAR, np.linspace(0, 2, n), key_values(rng, path, n), animation)
    # a chain 9 deep under an animated root, one link mirrored, with a second animated joint halfway down
    chain = [b.node(instances=1)]
    for d in range(8):
        chain.append(b.node(chain[-1], trs=b.trs(negative_scale=(d == 3)), instances=1 if d % 2 else 0))
    b.channel(S.ANIM_PATH_ROTATION, lin(S.ANIM_PATH_ROTATION, 5), [chain[0]])
    b.channel(S.ANIM_PATH_TRANSLATION, lin(S.ANIM_PATH_TRANSLATION, 3), [chain[4]])
    # an animated parent with `wide` children: dynamic only through their parent; the parent has three instances, every seventh child one
    parent = b.node(instances=3)
    children = [b.node(parent, instances=1 if k % 7 == 0 else 0) for k in range(wide)]
    b.channel(S.ANIM_PATH_SCALE, lin(S.ANIM_PATH_SCALE, 4), [parent])
    grandchild = b.node(children[5], instances=1)
    # a static parent whose baseWorld is no TRS product, with an animated child and a static one
    static_parent = b.node(base_world=(np.eye(4) + rng.uniform(-0.5, 0.5, (4, 4)) * [1, 1, 1, 0]).astype(F), instances=1)
    animated_child = b.node(static_parent, instances=2)
    static_child = b.node(static_parent, instances=1)
    # one channel with several targets, among them the animated child
    several = [animated_child, b.node(instances=1), b.node(instances=0)]
    b.channel(S.ANIM_PATH_TRANSLATION, lin(S.ANIM_PATH_TRANSLATION, 4), several)
    # an untouched subtree with arbitrary baseWorlds
    root = b.node(base_world=rng.uniform(-2, 2, (4, 4)).astype(F), instances=1)
    b.node(root, base_world=rng.uniform(-2, 2, (4, 4)).astype(F), instances=1)
    # overrides: the same (node, path) written twice in one animation, and by a later animation although its channel comes first
    twice = b.node(instances=1)
    later = lin(S.ANIM_PATH_ROTATION, 3, animation=2)
    b.channel(S.ANIM_PATH_ROTATION, later, [twice, chain[0]])                      # animation 2: wins on both nodes
    b.channel(S.ANIM_PATH_TRANSLATION, lin(S.ANIM_PATH_TRANSLATION, 3, animation=1), [twice])
    b.channel(S.ANIM_PATH_TRANSLATION, lin(S.ANIM_PATH_TRANSLATION, 3, animation=1), [twice, twice])    # same animation, later channel wins
    b.channel(S.ANIM_PATH_ROTATION, lin(S.ANIM_PATH_ROTATION, 3, animation=1), [twice])              # loses to animation 2
    b.channel(S.ANIM_PATH_SCALE, b.sampler(S.ANIM_STEP, [], np.zeros((0, 4)), animation=1), [static_child])   # no keys: static_child stays static
    tables, count = b.tables()
    names = dict(chain=chain, parent=parent, children=children, grandchild=grandchild, static_parent=static_parent, animated_child=animated_child,
                 static_child=static_child, several=several, untouched=[root, root + 1], twice=twice)
    return dict(tables=tables, times=[[0.4, 1.1, 0.7], [1.9, 0.0, 2.5]], instance_count=count, names=names)


def skin_case(joints):
    """A skeleton of `joints` joints (a chain with side branches) under a static armature node, every third joint animated in rotation, the
    root joint in translation, and weight channels into three morph slots (two of them written by one channel; a fourth slot stays 0)."""
    b = Builder(14 + joints)
    rng = b.rng
    b.animation_count, b.morph_weight_count = 2, 4
    armature = b.node()
    nodes = []
    for j in range(joints):
        parent = armature if j == 0 else nodes[max(0, j - 1 - int(rng.integers(0, 3)))]
        nodes.append(b.node(parent))
        b.joint(nodes[-1])
        if j % 3 == 0:
            b.channel(S.ANIM_PATH_ROTATION, b.sampler(S.ANIM_SLERP, [0, 0.7, 1.5], key_values(rng, S.ANIM_PATH_ROTATION, 3)), [nodes[-1]])
    b.channel(S.ANIM_PATH_TRANSLATION, b.sampler(S.ANIM_CATMULLROM, [0, 0.5, 1.0, 1.5], key_values(rng, S.ANIM_PATH_TRANSLATION, 4)), [nodes[0]])
    b.channel(S.ANIM_PATH_WEIGHTS, b.sampler(S.ANIM_LINEAR, [0, 3.0], [[0.1, 9, 9, 9], [0.9, 9, 9, 9]], animation=1), [0, 2])
    b.channel(S.ANIM_PATH_WEIGHTS, b.sampler(S.ANIM_STEP, [0, 1.0, 3.0], [[0.25, 0, 0, 0], [0.5, 0, 0, 0], [0.75, 0, 0, 0]], animation=1), [1])
    tables, count = b.tables(extra_instances=1)
    return dict(tables=tables, times=[[0.3, 2.0], [1.2, 0.5]], instance_count=count)


def clock_case():
    """Two animations of different durations and one whose only key is at 0 (duration 0: its time is never wrapped)."""
    b = Builder(15)
    b.animation_count = 3
    for animation, last in ((0, 2.5), (1, 0.75), (2, 0.0)):
        times = [0.0, last] if last else [0.0]
        s = b.sampler(S.ANIM_LINEAR, times, key_values(b.rng, S.ANIM_PATH_TRANSLATION, len(times)), animation)
        b.channel(S.ANIM_PATH_TRANSLATION, s, [b.node(instances=1)])
    b.sampler(S.ANIM_LINEAR, [0.0, 1.0], key_values(b.rng, S.ANIM_PATH_SCALE, 2), 0)        # a shorter sampler of animation 0: the longest counts
    tables, count = b.tables()
    return dict(tables=tables, times=[[0.1, 0.2, 0.3]], instance_count=count, durations=[2.5, 0.75, 0.0], steps=[0.4, 0.4, 3.1, 0.0, 7.9, 0.016])


def empty_case():
    """No channel at all: nothing is composed, every node keeps baseWorld, the palette is inverseBind . baseWorld."""
    b = Builder(16)
    root = b.node(instances=1)
    b.joint(b.node(root))
    tables, count = b.tables()
    tables["animation_count"] = 0
    return dict(tables=tables, times=[[]], instance_count=count)


_CASES = {}


def cases():
    """name -> case; built once."""
    if not _CASES:
        _CASES.update(samplers=sampler_case(), slerp=slerp_case(), hierarchy=hierarchy_case(), hierarchy_small=hierarchy_case(wide=20), skin5=skin_case(5),
                      skin300=skin_case(300), clock=clock_case(), empty=empty_case())
    return _CASES


def scene_instances(case, seed=3):
    """S.PerInstanceData records for the case's scene: the listed ones at their node's baseWorld, the others at random affine matrices;
    m_PrevWorld is something else everywhere, so that the roll shows."""
    rng = np.random.default_rng(seed)
    inst = np.zeros(case["instance_count"], S.PerInstanceData)
    inst["m_World"] = (np.eye(4) + rng.uniform(-0.5, 0.5, (len(inst), 4, 4)) * [1, 1, 1, 0]).astype(F)
    inst["m_PrevWorld"] = rng.uniform(-1, 1, (len(inst), 4, 4)).astype(F)
    inst["m_Radius"] = 1.5
    tb = case["tables"]
    for n in tb["nodes"]:
        for k in range(n["instanceCount"]):
            inst["m_World"][tb["node_instances"][n["firstInstance"] + k]] = n["baseWorld"]
    return inst
