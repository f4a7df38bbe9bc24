"""Host-side validator of a built acceleration structure (hrpt_selftest_read_bvh / hrpt_selftest_host_build), in plain numpy.

It shares no code with the product: record layouts come from hobbyrenderer_amd/structs.py, the rules from the comments of
csrc/pt_scene_records.h and csrc/bvh_build.h. Everything is level-synchronous and vectorised (one numpy pass per tree level), so a tree over a
million triangles is checked in seconds. validate() returns a Report of NAMED violations with counts and the first offender, e.g.
"leaf_pad: 3 of 4-wide leaf slots, first node 812 slot 2".

What each builder is held to (read from the code, so that the checks can be equalities where the code promises one):
  * boxes. Both builders pad every triangle by the same fp32 expression (bvh_build.cpp:322-328, bvh_build_gpu.hip k_setup) compiled without
    contraction, and every box above is a chain of exact min / max: the host recursion grows `bounds` from the padded primitive boxes
    (bvh_build.cpp Builder::build), the radix tree is fitted by k_fit, PLOC carries pMin / pMax, k_emit2 / k_emit4 / collapse4 copy boxes.
    No builder widens further, a refit recomputes with k_fit. So every stored child box must EQUAL the reference box of its subtree bit for
    bit ("box_not_equal"), and anything that does not even contain it is "box_not_containing" (inner child) / "leaf_pad" (leaf).
  * leaves. The 4-wide collapse only regroups inner nodes: both trees must hold the SAME multiset of leaf references.
  * node order. Both builders number nodes depth first (pre-order), so a child index is always larger than its parent's: a reference that is
    not ("child_back_reference") is a cycle or a broken layout.
  * depths. `maxDepth4` is the depth of the deepest inner 4-wide node (root 0) in both builders; `maxDepth` is the depth of the deepest
    inner 2-wide node for the GPU builder (k_depth) and of the deepest LEAF for the host builder (Builder::build counts the leaf call): one more.
"""
import numpy as np

from hobbyrenderer_amd import structs as S

F = np.float32
EMPTY = S.BVH_EMPTY_CHILD
FAR = F(1e30)


class Report:
    """Named violations: name -> (count, text)."""

    def __init__(self):
        self.violations = {}
        self.stats = {}

    def add(self, name, count, text):
        if count:
            old = self.violations.get(name)
            self.violations[name] = (count + old[0], old[1]) if old else (int(count), text)

    def flag(self, name, mask, what, where=lambda i: f"index {i}"):
        mask = np.asarray(mask)
        n = int(np.count_nonzero(mask))
        if n:
            first = tuple(int(x) for x in np.argwhere(mask)[0])
            self.add(name, n, f"{n} {what}, first {where(*first)}")

    def names(self):
        return set(self.violations)

    def __bool__(self):
        return bool(self.violations)

    def __str__(self):
        return "; ".join(f"{k}: {v[1]}" for k, v in sorted(self.violations.items())) or "valid"


# ------------------------------------------------------------------------------------------------ scene side (the expected triangles)
def transform_points(p, m):
    """mul(float4(p, 1), M).xyz in the row-vector convention, left to right, every operation rounded to binary32 (include/hobbyrt/detmath.h
    contract: no contraction). p: [..., 3] float32, m: [..., 4, 4] float32 broadcastable against p[..., None, :]."""
    p = np.asarray(p, F)
    m = np.asarray(m, F)
    out = np.empty(np.broadcast_shapes(p.shape[:-1], m.shape[:-2]) + (3,), F)
    for k in range(3):
        out[..., k] = ((p[..., 0] * m[..., 0, k] + p[..., 1] * m[..., 1, k]) + p[..., 2] * m[..., 2, k]) + m[..., 3, k]
    return out


def triangle_flags_for_material(mat):
    """bvh_build.h triangle_flags_for_material: bit 0 opaque, bits 1-2 shading class."""
    opaque = (mat["m_AlphaMode"] == S.ALPHA_MODE_OPAQUE).astype(np.uint32)
    transmissive = (mat["m_TransmissionFactor"] > 0) | (mat["m_AlphaMode"] == S.ALPHA_MODE_BLEND)
    cls = np.where(transmissive, 2, np.where(mat["m_TextureFlags"] != 0, 1, 0)).astype(np.uint32)
    return opaque | (cls << 1)


def expected_triangles(scene, two_level=False):
    """Every (owner, primitive) of the scene in (owner, primitive) order with its three vertices and flags. Flat: owner = instance, world-space
    vertices. Two-level: owner = mesh (every mesh some instance uses), object-space vertices, flags 0."""
    md = scene.mesh_data
    tri_count = (md["m_IndexCounts"][:, 0] // 3).astype(np.int64)
    first_index = md["m_IndexOffsets"][:, 0].astype(np.int64)
    if two_level:
        used = np.zeros(len(md), bool)
        used[scene.instances["m_MeshDataIndex"]] = True
        owners = np.flatnonzero(used)
        mesh_of_owner = owners
    else:
        owners = np.arange(len(scene.instances))
        mesh_of_owner = scene.instances["m_MeshDataIndex"].astype(np.int64)
    counts = tri_count[mesh_of_owner]
    base = np.concatenate([[0], np.cumsum(counts)])
    total = int(base[-1])
    owner_slot = np.repeat(np.arange(len(owners)), counts)
    prim = np.arange(total) - base[owner_slot]
    ix = scene.indices[(first_index[mesh_of_owner][owner_slot] + 3 * prim)[:, None] + np.arange(3)]
    pos = scene.vertices["m_Pos"][ix]                                       # [T, 3 vertices, 3]
    if two_level:
        flags = np.zeros(total, np.uint32)
    else:
        pos = transform_points(pos, scene.instances["m_World"][owner_slot][:, None])
        flags = triangle_flags_for_material(scene.materials)[scene.instances["m_MaterialIndex"]][owner_slot]
    owner_base = np.full(int(owners.max()) + 2 if len(owners) else 1, -1, np.int64)
    owner_count = np.zeros_like(owner_base)
    owner_base[owners] = base[:-1]
    owner_count[owners] = counts
    return dict(owner=owners[owner_slot].astype(np.uint32), prim=prim.astype(np.uint32), pos=pos, flags=flags, owner_base=owner_base,
                owner_count=owner_count, total=total)


def padded_triangle_boxes(p0, p1, p2):
    """bvh_build.cpp:322-328 (and triangle_extent above it) in binary32, operation by operation."""
    lo = np.minimum(p0, np.minimum(p1, p2))
    hi = np.maximum(p0, np.maximum(p1, p2))
    ext_pad = F(1e-6) * (hi - lo).max(axis=-1, keepdims=True)
    pad = (F(1e-5) * np.maximum(np.abs(lo), np.abs(hi)) + F(1e-6)) + ext_pad
    return lo - pad, hi + pad, lo, hi


# ------------------------------------------------------------------------------------------------ trees
def tree_arrays2(nodes):
    child = np.stack([nodes["left"], nodes["right"]], 1)
    bmin = np.stack([nodes["lmin"], nodes["rmin"]], 1)
    bmax = np.stack([nodes["lmax"], nodes["rmax"]], 1)
    return child, bmin, bmax


def tree_arrays4(nodes4):
    child = nodes4["child"]
    bmin = np.stack([nodes4["minx"], nodes4["miny"], nodes4["minz"]], 2)        # [N, slot, axis]
    bmax = np.stack([nodes4["maxx"], nodes4["maxy"], nodes4["maxz"]], 2)
    return child, bmin, bmax


def decode_leaf(ref):
    enc = (~ref.astype(np.int64)) & 0xFFFFFFFF
    return enc >> 2, (enc & 3) + 1


def walk(rep, tag, child, roots, lo=0, hi=None, allow_unreached=False):
    """Level-synchronous walk from `roots` over nodes [lo, hi). Returns (depth per node, -1 = unreached; visit counts)."""
    n = len(child)
    hi = n if hi is None else hi
    visits = np.zeros(n, np.int64)
    depth = np.full(n, -1, np.int64)
    roots = np.asarray(roots, np.int64)
    bad_root = (roots < lo) | (roots >= hi)
    rep.flag(f"{tag}root_range", bad_root, "roots outside the node range")
    frontier = np.unique(roots[~bad_root])
    np.add.at(visits, roots[~bad_root], 1)
    d = 0
    while frontier.size and d <= n:
        depth[frontier] = d
        refs = child[frontier]
        inner = (refs >= 0) & (refs != EMPTY)
        oob = inner & ((refs >= hi) | (refs < lo))
        rep.flag(f"{tag}child_range", oob, "inner references outside the node range", lambda i, s: f"node {frontier[i]} slot {s}")
        back = inner & ~oob & (refs <= frontier[:, None])
        rep.flag(f"{tag}child_back_reference", back, "inner references to a node that is not behind its parent (a cycle, or not pre-order)",
                 lambda i, s: f"node {frontier[i]} slot {s}")
        cnt = np.bincount(refs[inner & ~oob], minlength=n)
        new = (cnt > 0) & (visits == 0)
        visits += cnt
        frontier = np.flatnonzero(new)
        d += 1
    rng = np.arange(n)
    in_range = (rng >= lo) & (rng < hi)
    rep.flag(f"{tag}node_reached_twice", visits > 1, "nodes referenced more than once")
    if not allow_unreached:
        rep.flag(f"{tag}node_unreachable", in_range & (visits == 0), "nodes that no walk from the root reaches (count field does not match the tree)")
    return depth, visits


def worst_stack_occupancy(child, depth, pushed_per_node=None):
    """Most entries a traversal that finds EVERY child of every node it visits can have pending: each visited inner node leaves all its used
    slots but the one it descends into (inner_step pushes leaves like inner nodes), so it is the largest sum of (used slots - 1) over the paths
    from the root to an inner node. Computed top-down over the reached nodes, level by level."""
    n, w = child.shape
    own = ((child != EMPTY).sum(1) - 1).clip(min=0)
    occ = np.zeros(n, np.int64)
    for d in range(0, int(depth.max()) + 1):
        idx = np.flatnonzero(depth == d)
        if d == 0:
            occ[idx] = own[idx]
        refs = child[idx]
        inner = (refs >= 0) & (refs != EMPTY) & (refs < n)
        inner &= depth[np.where(inner, refs, 0)] == d + 1
        tgt = refs[inner]
        occ[tgt] = np.repeat(occ[idx], inner.sum(1)) + own[tgt]
    return int(occ[depth >= 0].max())


def leaf_slots(child, depth):
    """(node, slot, ref) of every leaf reference of the reached nodes."""
    reached = depth >= 0
    m = (child < 0) & reached[:, None]
    node, slot = np.nonzero(m)
    return node, slot, child[node, slot]


def check_partition(rep, tag, refs, node, slot, total, max_leaf, what="triangles"):
    first, count = decode_leaf(refs)
    oob = first + count > total
    rep.flag(f"{tag}leaf_range", oob, f"leaves reaching past the {what}", lambda i: f"node {node[i]} slot {slot[i]}")
    rep.flag(f"{tag}leaf_size", count > max_leaf, f"leaves with more than {max_leaf} {what}", lambda i: f"node {node[i]} slot {slot[i]}")
    ok = ~oob
    diff = np.zeros(total + 1, np.int64)
    np.add.at(diff, first[ok], 1)
    np.add.at(diff, (first + count)[ok], -1)
    cover = np.cumsum(diff)[:total]
    rep.flag(f"{tag}triangle_unreferenced", cover == 0, f"{what} that no leaf references", lambda i: f"record {i}")
    rep.flag(f"{tag}triangle_in_two_leaves", cover > 1, f"{what} that more than one leaf references", lambda i: f"record {i}")


def reference_boxes(child, depth, leaf_min, leaf_max):
    """Bottom-up exact unions. leaf_min / leaf_max: callables ref array -> [k, 3] boxes of leaf references. Returns the reference box of every
    child slot ([N, W, 3] x 2; +inf / -inf where the slot is unused or unreached)."""
    n, w = child.shape
    smin = np.full((n, w, 3), np.inf, F)
    smax = np.full((n, w, 3), -np.inf, F)
    nmin = np.full((n, 3), np.inf, F)
    nmax = np.full((n, 3), -np.inf, F)
    for d in range(int(depth.max()), -1, -1):
        idx = np.flatnonzero(depth == d)
        refs = child[idx]
        leaf = refs < 0
        inner = (refs >= 0) & (refs != EMPTY) & (refs < n)
        inner &= depth[np.where(inner, refs, 0)] > d                  # (a back reference has no finished box below it)
        mn = np.full(refs.shape + (3,), np.inf, F)
        mx = np.full(refs.shape + (3,), -np.inf, F)
        mn[leaf] = leaf_min(refs[leaf]); mx[leaf] = leaf_max(refs[leaf])
        mn[inner] = nmin[refs[inner]]; mx[inner] = nmax[refs[inner]]
        smin[idx] = mn; smax[idx] = mx
        nmin[idx] = mn.min(axis=1); nmax[idx] = mx.max(axis=1)
    return smin, smax


def leaf_box_functions(tmin, tmax, total):
    """Union of the padded boxes of a leaf's records (count <= 4)."""
    def gather(refs, arr, fill, red):
        first, count = decode_leaf(refs)
        k = np.arange(4)
        idx = first[:, None] + k
        valid = (k < count[:, None]) & (idx < total)
        vals = np.where(valid[..., None], arr[np.minimum(idx, max(total - 1, 0))], F(fill))
        return red(vals, axis=1)
    return (lambda refs: gather(refs, tmin, np.inf, np.min)), (lambda refs: gather(refs, tmax, -np.inf, np.max))


def area(mn, mx):
    e = np.maximum(mx.astype(np.float64) - mn.astype(np.float64), 0.0)
    return e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 2] * e[..., 0]


def check_boxes(rep, tag, child, depth, bmin, bmax, smin, smax, raw_min=None, raw_max=None):
    """Stored child boxes against the reference boxes of their subtrees."""
    reached = (depth >= 0)[:, None]
    used = (child != EMPTY) & reached & np.isfinite(smin).all(-1)
    leaf = used & (child < 0)
    inner = used & (child >= 0)
    contains = ((bmin <= smin) & (bmax >= smax)).all(-1)
    where = lambda i, s: f"node {i} slot {s}"
    rep.flag(f"{tag}box_not_containing", inner & ~contains, "inner child boxes that do not contain the boxes below them", where)
    rep.flag(f"{tag}leaf_pad", leaf & ~contains, "leaf boxes closer to their triangles than the padding allows", where)
    equal = ((bmin.view(np.uint32) == smin.view(np.uint32)) & (bmax.view(np.uint32) == smax.view(np.uint32))).all(-1)
    rep.flag(f"{tag}box_not_equal", used & contains & ~equal, "child boxes wider than the exact union the builders promise", where)
    unused = (child == EMPTY) & reached
    far = ((bmin == FAR) & (bmax == FAR)).all(-1)
    rep.flag(f"{tag}unused_slot_box", unused & ~far, "unused slots without the far degenerate box", where)
    sa, ra = float(area(bmin[used], bmax[used]).sum()), float(area(smin[used], smax[used]).sum())
    rep.stats[f"{tag}stored_over_reference_area"] = sa / ra if ra > 0 else 1.0


# ------------------------------------------------------------------------------------------------ quantised nodes
def check_quantised(rep, nodes4, nodesq, depth):
    child, bmin, bmax = tree_arrays4(nodes4)
    reached = (depth >= 0)[:, None]
    where = lambda i, s, *a: f"node4 {i} slot {s}" + (f" axis {a[0]}" if a else "")
    rep.flag("q_child_mismatch", (nodesq["child"] != child) & reached, "quantised child references that differ from the fp32 node's", where)
    lo = np.stack([nodesq["lox"], nodesq["loy"], nodesq["loz"]], 1)       # [N, axis] words, byte c = child c
    hi = np.stack([nodesq["hix"], nodesq["hiy"], nodesq["hiz"]], 1)
    sh = (8 * np.arange(4, dtype=np.uint32))[None, :, None]
    qlo = (lo[:, None, :] >> sh) & 255                                      # [N, slot, axis]
    qhi = (hi[:, None, :] >> sh) & 255
    step = np.stack([nodesq["sx"], nodesq["sy"], nodesq["sz"]], 1)
    org = nodesq["o"]
    rep.flag("q_step", ~((step > 0) & np.isfinite(step)) & reached, "steps that are not positive and finite", lambda i, a: f"node4 {i} axis {a}")
    unused = (child == EMPTY) & reached
    rep.flag("q_unused_slot", unused[..., None] & ~((qlo == 255) & (qhi == 0)), "unused slots without lo = 255 > hi = 0", where)
    used = ((child != EMPTY) & reached)[..., None] & np.ones(3, bool)
    o3, s3 = np.broadcast_to(org[:, None, :], qlo.shape), np.broadcast_to(step[:, None, :], qlo.shape)
    dlo = o3 + qlo.astype(F) * s3                                           # separately rounded binary32, as hrpt_selftest_bvh decodes
    dhi = o3 + qhi.astype(F) * s3
    rep.flag("q_plane_inside", used & ~((dlo <= bmin) & (dhi >= bmax)), "decoded planes (separately rounded) inside the fp32 box", where)


def quantise_reference(nodes4):
    """A valid GpuNodeQ array for `nodes4` by the rule of pt_scene_records.h (origin = min corner of the used child boxes, one step per axis, planes
    rounded outward under the separately rounded decode): lets the CPU tests exercise check_quantised on host-built trees."""
    child, bmin, bmax = tree_arrays4(nodes4)
    used = child != EMPTY
    mn = np.where(used[..., None], bmin, F(3e38)).min(1)
    mx = np.where(used[..., None], bmax, F(-3e38)).max(1)
    step = np.maximum(np.maximum((mx - mn) * F(1.0 / 254.0) * F(1.000001), np.maximum(np.abs(mn), np.abs(mx)) * F(2.4e-7)), F(1e-30)).astype(F)
    o, s = mn[:, None, :], step[:, None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        ql = np.clip(np.floor((bmin - o) / s), 0, 255).astype(np.int64)
        qh = np.clip(np.ceil((bmax - o) / s), 0, 255).astype(np.int64)
        for _ in range(4):
            ql = np.where((ql > 0) & ~(o + ql.astype(F) * s <= bmin), ql - 1, ql)
            qh = np.where((qh < 255) & ~(o + qh.astype(F) * s >= bmax), qh + 1, qh)
    ql = np.where(used[..., None], ql, 255).astype(np.uint32)
    qh = np.where(used[..., None], qh, 0).astype(np.uint32)
    sh = (8 * np.arange(4, dtype=np.uint32))[None, :, None]
    q = np.zeros(len(nodes4), S.GpuNodeQ)
    lo, hi = (ql << sh).sum(1).astype(np.uint32), (qh << sh).sum(1).astype(np.uint32)
    q["o"] = mn; q["sx"], q["sy"], q["sz"] = step[:, 0], step[:, 1], step[:, 2]
    q["lox"], q["loy"], q["loz"] = lo[:, 0], lo[:, 1], lo[:, 2]
    q["hix"], q["hiy"], q["hiz"] = hi[:, 0], hi[:, 1], hi[:, 2]
    q["child"] = child
    return q


def fma32(a, b, c):
    """fmaf(a, b, c) for binary32 arrays: the product of two binary32 numbers is exact in binary64; the sum is rounded to binary64 and then to
    binary32 (a double rounding that differs from a true fused operation only when the binary64 sum lands exactly on a binary32 tie)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def folded_decode_intervals(nodes4, nodesq, origin, direction, tmin=0.0, tlim=1e10):
    """What inner_step (pt_traverse.h, the IsQuantised branch) computes for ONE ray at every slot of every node, restated operation by operation in
    binary32: inv = 1 / d capped at +-1e20 (traversal_rcp; the hardware reciprocal may differ from the correctly rounded one used here by an ulp:
    whichever value it is, it is the `inv` of both sides of the comparison below), noi = -(o_ray * inv), ax = s * inv, bx = fma(o_node, inv, noi),
    plane distance = fma(float(q), ax, bx), near / far words by the sign of inv, lo = max(near distances, tmin),
    hi = min(far distances, tlim) * (1 + 4e-6). Next to it the ray's interval with the fp32 box of the same slot, (plane - o_ray) * inv, in
    binary64. Returns (lo_q, hi_q, near_exact, far_exact), each [N, 4]; hi_q carries the kernel's 4e-6 scale, near / far exact are not clamped."""
    child, bmin, bmax = tree_arrays4(nodes4)
    ro, d = np.asarray(origin, F), np.asarray(direction, F)
    with np.errstate(divide="ignore"):
        inv = np.clip(F(1.0) / d, F(-1e20), F(1e20)).astype(F)
    noi = -(ro * inv)
    step = np.stack([nodesq["sx"], nodesq["sy"], nodesq["sz"]], 1)
    a = step * inv                                                          # [N, axis]
    b = fma32(nodesq["o"], np.broadcast_to(inv, step.shape), np.broadcast_to(noi, step.shape))
    lo = np.stack([nodesq["lox"], nodesq["loy"], nodesq["loz"]], 1)
    hi = np.stack([nodesq["hix"], nodesq["hiy"], nodesq["hiz"]], 1)
    neg = inv < 0
    wn, wf = np.where(neg, hi, lo), np.where(neg, lo, hi)                   # near / far plane words of every axis
    sh = (8 * np.arange(4, dtype=np.uint32))[None, :, None]
    qn, qf = ((wn[:, None, :] >> sh) & 255).astype(F), ((wf[:, None, :] >> sh) & 255).astype(F)
    a3, b3 = np.broadcast_to(a[:, None, :], qn.shape), np.broadcast_to(b[:, None, :], qn.shape)
    lo_q = np.maximum(fma32(qn, a3, b3).max(-1), F(tmin))
    hi_q = (np.minimum(fma32(qf, a3, b3).min(-1), F(tlim)) * (F(1.0) + F(4e-6))).astype(F)
    inv64, ro64 = inv.astype(np.float64), ro.astype(np.float64)
    pn, pf = np.where(neg, bmax, bmin).astype(np.float64), np.where(neg, bmin, bmax).astype(np.float64)
    near = ((pn - ro64) * inv64).max(-1)
    far = ((pf - ro64) * inv64).min(-1)
    return lo_q, hi_q, near, far


U = 2.0 ** -24


def check_folded_decode(rep, nodes4, nodesq, depth, rays, tag="q_folded_"):
    """The traversal's own decode (folded_decode_intervals) against the ray's exact interval with the fp32 box, for every ray of `rays` (S.Ray
    records) and every used slot of every reached node.

    A strict bracket (lo_q <= near, hi_q >= far) does NOT hold and cannot: the far end is scaled by 1 + 4e-6, the near end is not widened, and each
    distance goes through four roundings (noi, ax, bx, the final fma). Measured on the host tree of the 101 k-triangle scene, among the slots a ray
    hits: far end below the exact one 0 of 7 694, near end above it 501 of 4 585 (per-triangle rays) and 1 010 of 3 109 (axis-parallel rays), by
    rounding alone; the counts are kept in rep.stats. What is asserted is the bracket up to that rounding, with the bound derived per axis from the
    operations (u = 2^-24): the decoded plane o + q s lies on the right side of the box plane up to u (2 q s + |o|) (it is on the right side under the
    separately rounded decode, check_quantised); noi is off by u |o_ray inv|, q ax by u q s |inv|, bx by u (|o inv| + |o_ray inv|), the result by
    u |t|, the 4e-6 scale and the binary64 emulation of the fma by another u |t|:
        E = u (2 |o_ray inv| + 2 |o inv| + 3 q s |inv| + 2 |t|), the largest over the three axes,
    and: lo_q <= max(near, tmin) + E for every used slot, hi_q >= min(far, tlim) - E for every used slot with far >= 0 (the scale presumes a
    non-negative far end: behind the ray nothing is hit). Independently of E's form, the outcome: a slot whose exact interval is longer than 2 E
    must pass the kernel's own test lo_q <= hi_q. (One quantisation step is of the order of E, so a plane one step inside its box is the business
    of check_quantised, not of this check: this one pins the word / byte selection, the signs and the scale of the folded form.)"""
    child, bmin, bmax = tree_arrays4(nodes4)
    used = (child != EMPTY) & (depth >= 0)[:, None]
    step = np.stack([nodesq["sx"], nodesq["sy"], nodesq["sz"]], 1).astype(np.float64)
    org = np.abs(nodesq["o"].astype(np.float64))
    strict_near = strict_far = hit_slots = 0
    where = lambda i, s: f"node4 {i} slot {s}"
    for k, r in enumerate(rays):
        tmin, tlim = float(r["tmin"]), float(r["tmax"])
        lo_q, hi_q, near, far = folded_decode_intervals(nodes4, nodesq, r["origin"], r["direction"], tmin, tlim)
        with np.errstate(divide="ignore"):
            inv = np.abs(np.clip(F(1.0) / r["direction"], F(-1e20), F(1e20)).astype(np.float64))
        ro = np.abs(r["origin"].astype(np.float64))
        e_axis = U * (2 * ro * inv + 2 * org * inv + 3 * 255 * step * inv)          # [N, axis]
        en, ef = np.maximum(near, tmin), np.minimum(far, tlim)
        e = (e_axis.max(1)[:, None] + 2 * U * np.maximum(np.abs(lo_q), np.abs(hi_q)).astype(np.float64)) * 1.001
        hit = used & (en <= ef)
        hit_slots += int(hit.sum()); strict_near += int((hit & (lo_q > en)).sum()); strict_far += int((hit & (hi_q < ef)).sum())
        rep.flag(f"{tag}near", used & (lo_q > en + e), f"near distances of ray {k} beyond the exact one by more than the rounding bound", where)
        rep.flag(f"{tag}far", used & (far >= 0) & (hi_q < ef - e), f"far distances of ray {k} short of the exact one by more than the rounding bound", where)
        rep.flag(f"{tag}rejects_hit", used & (ef - en > 2 * e) & ~(lo_q <= hi_q), f"slots ray {k} passes through that the folded test rejects", where)
    rep.stats.update({f"{tag}rays": len(rays), f"{tag}hit_slots": hit_slots, f"{tag}strict_near_violations": strict_near, f"{tag}strict_far_violations": strict_far})


# ------------------------------------------------------------------------------------------------ the whole structure
def sah_cost(nodes, root_min, root_max):
    """hobbyrt_pt.h HrptBuildInfo::sahCost in binary64: 1 + sum(area(child) * (inner ? 1 : triangles)) / area(root)."""
    child, bmin, bmax = tree_arrays2(nodes)
    _, count = decode_leaf(child)
    w = np.where(child >= 0, 1.0, count.astype(np.float64))
    total = float((area(bmin, bmax) * w).sum())
    ra = float(area(root_min, root_max))
    return 1.0 + total / ra if ra > 0 else 0.0


def validate_flat(dump, scene, builder="host", max_leaf=None):
    """Checks of a flat structure. builder: "host" or "gpu" (what is promised differs: leaf size, depth convention, sahCost precision)."""
    rep = Report()
    max_leaf = max_leaf or (4 if builder == "host" else 2)
    tris = dump["triangles"]
    total = len(tris)
    exp = expected_triangles(scene)

    # ---- triangle records: every (instance, primitive) once, bit-equal positions, flags
    inst, prim = tris["inst"].astype(np.int64), tris["prim"].astype(np.int64)
    known = inst < len(exp["owner_base"])
    known &= prim < exp["owner_count"][np.where(known, inst, 0)]
    rep.flag("tri_unknown_key", ~known, "triangle records whose (instance, primitive) is not in the scene", lambda i: f"record {i}")
    g = np.where(known, exp["owner_base"][np.where(known, inst, 0)] + prim, 0)
    seen = np.bincount(g[known], minlength=exp["total"])
    rep.flag("tri_key_missing", seen == 0, "(instance, primitive) pairs of the scene without a record", lambda i: f"pair ({exp['owner'][i]}, {exp['prim'][i]})")
    rep.flag("tri_key_duplicate", seen > 1, "(instance, primitive) pairs with more than one record", lambda i: f"pair ({exp['owner'][i]}, {exp['prim'][i]})")
    pos = np.stack([tris["p0"], tris["p1"], tris["p2"]], 1)
    rep.flag("tri_position", known & (pos.view(np.uint32) != exp["pos"][g].view(np.uint32)).any((1, 2)),
             "records whose vertices are not the scene's world-space vertices bit for bit", lambda i: f"record {i} = ({inst[i]}, {prim[i]})")
    rep.flag("tri_flags", known & (tris["flags"] != exp["flags"][g]), "records with the wrong flags", lambda i: f"record {i}")
    attrs = dump["attributes"]
    if attrs is not None and len(attrs) == total:
        mat = scene.instances["m_MaterialIndex"][np.where(known, inst, 0)]
        rep.flag("attr_key", (attrs["inst"] != tris["inst"]) | (attrs["prim"] != tris["prim"]) | (known & (attrs["material"] != mat)),
                 "attribute records that do not belong to the triangle at the same index", lambda i: f"record {i}")
    if total != exp["total"]:
        rep.add("tri_count", 1, f"{total} records for {exp['total']} triangles")

    nodes, nodes4 = dump["nodes"], dump["nodes4"]
    if len(nodes) == 0:                  # a one-leaf scene (or an empty one): rootLeaf
        if len(nodes4):
            rep.add("node4_without_nodes", 1, f"{len(nodes4)} 4-wide nodes but no 2-wide tree")
        if total:
            ref = np.array([dump["rootLeaf"]], np.int32)
            if ref[0] >= 0:
                rep.add("root_leaf", 1, f"rootLeaf {ref[0]} is not a leaf reference")
            else:
                check_partition(rep, "root_", ref, np.zeros(1, int), np.zeros(1, int), total, 4)
        return rep
    if dump["rootLeaf"] != 0:
        rep.add("root_leaf", 1, f"rootLeaf {dump['rootLeaf']} next to a tree")

    tmin, tmax, _, _ = padded_triangle_boxes(tris["p0"], tris["p1"], tris["p2"])
    lmin, lmax = leaf_box_functions(tmin, tmax, total)
    true_depth = {}
    occupancy = {}
    leaves = {}
    root_box = None
    for tag, (child, bmin, bmax), limit in (("n2_", tree_arrays2(nodes), max_leaf), ("n4_", tree_arrays4(nodes4), max_leaf)):
        if len(child) == 0:
            rep.add(f"{tag}empty", 1, "no node")
            continue
        depth, _ = walk(rep, tag, child, [0])
        node, slot, refs = leaf_slots(child, depth)
        check_partition(rep, tag, refs, node, slot, total, limit)
        leaves[tag] = np.sort(refs)
        smin, smax = reference_boxes(child, depth, lmin, lmax)
        check_boxes(rep, tag, child, depth, bmin, bmax, smin, smax)
        true_depth[tag] = int(depth.max())
        occupancy[tag] = worst_stack_occupancy(child, depth)
        if tag == "n2_":
            root_box = (smin[0].min(0), smax[0].max(0))
        else:
            usedn = ((child != EMPTY).sum(1) < 2) & (depth > 0)
            rep.flag("n4_underfull", usedn, "non-root 4-wide nodes with fewer than two children", lambda i: f"node4 {i}")
            if dump["nodesQ"] is not None:
                check_quantised(rep, nodes4, dump["nodesQ"], depth)
    if "n2_" in leaves and "n4_" in leaves and not np.array_equal(leaves["n2_"], leaves["n4_"]):
        diff = np.setxor1d(leaves["n2_"], leaves["n4_"])
        f, c = decode_leaf(diff[:1])
        rep.add("leaf_set_mismatch", len(diff), f"{len(diff)} leaf references in only one of the two trees, first (first {f[0]}, count {c[0]})")

    # ---- depths (see the module docstring for what each builder reports)
    d2, d4 = true_depth.get("n2_", 0), true_depth.get("n4_", 0)
    rep.stats.update(true_depth2=d2, true_depth4=d4, reported_depth2=dump["maxDepth"], reported_depth4=dump["maxDepth4"])
    want2 = d2 + 1 if builder == "host" else d2
    if dump["maxDepth"] < want2:
        rep.add("depth2_too_small", 1, f"maxDepth {dump['maxDepth']} reported, the tree needs {want2}")
    elif dump["maxDepth"] != want2:
        rep.add("depth2_not_exact", 1, f"maxDepth {dump['maxDepth']} reported, {want2} expected")
    # the stacks the launch plan sizes from these depths (pt_wavefront_plan.h: maxDepth + 2 and stack_entries4) against what the dumped trees can make pending
    for tag, bound in (("n2_", dump["maxDepth"] + 2), ("n4_", stack_entries4(dump["maxDepth4"]))):
        if tag in occupancy:
            rep.stats[f"{tag}worst_stack_occupancy"], rep.stats[f"{tag}stack_bound"] = occupancy[tag], bound
            if occupancy[tag] > bound:
                rep.add(f"{tag}stack_bound", 1, f"a traversal can hold {occupancy[tag]} entries, the stack is sized for {bound}")
    if dump["maxDepth4"] < d4:
        rep.add("depth4_too_small", 1, f"maxDepth4 {dump['maxDepth4']} reported, the deepest inner node is at {d4}")
    elif dump["maxDepth4"] != d4:
        rep.add("depth4_not_exact", 1, f"maxDepth4 {dump['maxDepth4']} reported, {d4} expected")

    # ---- sahCost. Host: every extent is a binary32 difference (2^-24 each, two per product), the sum is formed in binary64, the root area in
    # binary32 (extents, 3 products, 2 sums: 7 * 2^-24) and the result is rounded once: 16 * 2^-24 covers it. GPU: about nodeCount / 64 atomic additions of wave sums of positive binary32 terms, each term
    # (3 products, 2 sums, 1 weight product, 1 sum of two) and each addition off by at most 2^-24 relative: every partial sum is at most the
    # total, so the error is at most (terms' 8 + one per addition on a term's way: 6 in the wave + nodeCount / 64 atomics) * 2^-24, and the
    # division by the root area and the final sum add 8 * 2^-24 more.
    if root_box is not None and not rep.names() & {"n2_child_range", "n2_leaf_range"}:
        want = sah_cost(nodes, *root_box)
        bound = (8 + 8) * 2.0 ** -24 if builder == "host" else (8 + 6 + len(nodes) / 64.0 + 8) * 2.0 ** -24
        err = abs(float(dump["sahCost"]) - want) / want if want else abs(float(dump["sahCost"]))
        rep.stats.update(sah_cost=want, sah_rel_error=err, sah_bound=bound)
        if err > bound:
            rep.add("sah_cost", 1, f"sahCost {dump['sahCost']!r} reported, {want!r} recomputed: relative error {err:.3e} above {bound:.3e}")
    return rep


def stack_entries4(depth4):
    """pt_wavefront_plan.h stack_entries4 (tests/test_wavefront_plan.py pins the product's values): the size the plan gives the 4-wide stacks."""
    return 3 * (depth4 + 1)


# ------------------------------------------------------------------------------------------------ two-level structure
def instance_world_boxes(scene, mesh_min, mesh_max, padded=True):
    """bvh_build.cpp rebuild_two_level_instances: the eight corners of the mesh's object box through the flat path's transform, padded like a triangle."""
    m = scene.instances["m_MeshDataIndex"]
    omin, omax = mesh_min[m], mesh_max[m]
    c = np.arange(8)
    corners = np.stack([np.where((c & 1)[None, :] != 0, omax[:, None, 0], omin[:, None, 0]),
                        np.where((c & 2)[None, :] != 0, omax[:, None, 1], omin[:, None, 1]),
                        np.where((c & 4)[None, :] != 0, omax[:, None, 2], omin[:, None, 2])], -1).astype(F)
    w = transform_points(corners, scene.instances["m_World"][:, None])
    lo, hi = w.min(1), w.max(1)
    if not padded:
        return lo, hi
    ext_pad = F(1e-6) * (hi - lo).max(-1, keepdims=True)
    pad = (F(1e-5) * np.maximum(np.abs(lo), np.abs(hi)) + F(1e-6)) + ext_pad
    return lo - pad, hi + pad


def validate_two_level(dump, scene, flat_dump=None, gpu_instance_tree=False):
    """Checks of a two-level structure: the tree over the instances, every mesh tree, the instance records. flat_dump: the flat build of the
    same scene (its world-space vertices must lie inside the instance-leaf boxes). gpu_instance_tree: the instance tree was built on the
    device into a reserved range of instanceCount nodes, of which only the reachable ones are written."""
    rep = Report()
    tris, nodes4, insts = dump["triangles"], dump["nodes4"], dump["instances"]
    total, n_inst, n_tlas = len(tris), len(insts), dump["instanceNodeCount"]
    exp = expected_triangles(scene, two_level=True)
    mesh, prim = tris["inst"].astype(np.int64), tris["prim"].astype(np.int64)
    known = mesh < len(exp["owner_base"])
    known &= prim < exp["owner_count"][np.where(known, mesh, 0)]
    rep.flag("tri_unknown_key", ~known, "triangle records whose (mesh, primitive) is not in the scene", lambda i: f"record {i}")
    g = np.where(known, exp["owner_base"][np.where(known, mesh, 0)] + prim, 0)
    seen = np.bincount(g[known], minlength=exp["total"])
    rep.flag("tri_key_missing", seen == 0, "(mesh, primitive) pairs without a record", lambda i: f"pair ({exp['owner'][i]}, {exp['prim'][i]})")
    rep.flag("tri_key_duplicate", seen > 1, "(mesh, primitive) pairs with more than one record", lambda i: f"pair ({exp['owner'][i]}, {exp['prim'][i]})")
    pos = np.stack([tris["p0"], tris["p1"], tris["p2"]], 1)
    rep.flag("tri_position", known & (pos.view(np.uint32) != exp["pos"][g].view(np.uint32)).any((1, 2)), "records whose vertices are not the mesh's bit for bit",
             lambda i: f"record {i}")
    rep.flag("tri_flags", tris["flags"] != 0, "object-space records with flags", lambda i: f"record {i}")

    # ---- instance records
    si = scene.instances
    if n_inst != len(si):
        rep.add("instance_count", 1, f"{n_inst} records for {len(si)} instances")
        return rep
    rep.flag("inst_mesh", insts["mesh"] != si["m_MeshDataIndex"], "instance records with the wrong mesh")
    rep.flag("inst_material", insts["material"] != si["m_MaterialIndex"], "instance records with the wrong material")
    rep.flag("inst_flags", insts["flags"] != triangle_flags_for_material(scene.materials)[si["m_MaterialIndex"]], "instance records with the wrong flags")
    rep.flag("inst_world", (np.ascontiguousarray(insts["world"]).view(np.uint32) != np.ascontiguousarray(si["m_World"][:, :, :3]).view(np.uint32)).any((1, 2)),
             "instance records whose world rows differ from m_World")
    # inv . world = I against a binary64 inverse. The record is the binary64 inverse rounded once (2^-24 relative per entry); the product
    # world * inv then differs from I by at most 2^-24 * sum |world| |inv| per entry <= 2^-24 * cond_inf(world): 4 x that is asserted
    # (the binary64 inversion's own error, ~cond * 2^-53, is far below).
    a = si["m_World"][:, :3, :3].astype(np.float64)
    t = si["m_World"][:, 3, :3].astype(np.float64)
    inv = insts["inv"].astype(np.float64)
    prod = a @ inv[:, :3, :]
    resid = np.abs(prod - np.eye(3)).max((1, 2))
    tres = np.abs(np.einsum("ij,ijk->ik", t, inv[:, :3, :]) + inv[:, 3, :]).max(1)
    cond = np.abs(a).sum(2).max(1) * np.abs(inv[:, :3, :]).sum(2).max(1)
    tscale = (np.abs(t)[:, :, None] * np.abs(inv[:, :3, :])).sum(1).max(1)
    rep.flag("inst_inverse", (resid > 4 * 2.0 ** -24 * cond) | (tres > 4 * 2.0 ** -24 * np.maximum(tscale, 1e-300)), "instance records whose inverse is not the inverse of the world matrix",
             lambda i: f"instance {i} (residual {resid[i]:.3e}, condition {cond[i]:.3e})")

    # ---- trees: the instance tree [0, n_tlas) and one tree per used mesh behind it
    child, bmin, bmax = tree_arrays4(nodes4)
    tmin, tmax, raw_lo, raw_hi = padded_triangle_boxes(tris["p0"], tris["p1"], tris["p2"])
    n_mesh = len(scene.mesh_data)
    mesh_min = np.full((n_mesh, 3), np.inf, F); mesh_max = np.full((n_mesh, 3), -np.inf, F)
    if total:
        np.minimum.at(mesh_min, tris["inst"], raw_lo); np.maximum.at(mesh_max, tris["inst"], raw_hi)
    roots = insts["blasRoot"].astype(np.int64)
    mesh_of_root = {}
    for m, r in zip(insts["mesh"], roots):
        if mesh_of_root.setdefault(int(m), int(r)) != int(r):
            rep.add("inst_blas_root", 1, f"instances of mesh {m} with different blasRoot")
    empty_mesh = exp["owner_count"][np.minimum(insts["mesh"], len(exp["owner_count"]) - 1)] == 0
    rep.flag("inst_blas_root_empty", empty_mesh != (roots == -0x80000000), "blasRoot is kTraversalDone exactly for meshes without triangles")
    mesh_roots = np.array(sorted({r for r in mesh_of_root.values() if r >= 0}), np.int64)
    leaf_roots = np.array(sorted({r for r in mesh_of_root.values() if r < 0 and r != -0x80000000}), np.int64)
    lmin, lmax = leaf_box_functions(tmin, tmax, total)
    occ_blas = occ_tlas = 0
    if len(nodes4) > n_tlas or len(leaf_roots):
        depth, _ = walk(rep, "blas_", child, mesh_roots, lo=n_tlas)
        node, slot, refs = leaf_slots(child, depth)
        node, slot, refs = np.concatenate([node, np.zeros(len(leaf_roots), int)]), np.concatenate([slot, np.zeros(len(leaf_roots), int)]), \
            np.concatenate([refs, leaf_roots.astype(np.int32)])
        check_partition(rep, "blas_", refs, node, slot, total, 4)
        if len(mesh_roots):
            smin, smax = reference_boxes(child, depth, lmin, lmax)
            check_boxes(rep, "blas_", child, depth, bmin, bmax, smin, smax)
            levels = int(depth.max()) + 1
            occ_blas = worst_stack_occupancy(child, depth)
            rep.flag("blas_underfull", ((child != EMPTY).sum(1) < 2) & (depth > 0), "non-root 4-wide nodes with fewer than two children")
        else:
            levels = 0
        rep.stats.update(true_levels_blas=levels, reported_levels_blas=dump["maxDepth4Blas"])
        if dump["maxDepth4Blas"] < levels:
            rep.add("depth4_blas_too_small", 1, f"maxDepth4Blas {dump['maxDepth4Blas']} reported, the deepest mesh tree has {levels} levels")
        elif dump["maxDepth4Blas"] != levels:
            rep.add("depth4_blas_not_exact", 1, f"maxDepth4Blas {dump['maxDepth4Blas']} reported, {levels} expected")
    imin, imax = instance_world_boxes(scene, mesh_min, mesh_max)
    no_tris = ~np.isfinite(mesh_min[insts["mesh"]]).all(1)
    imin[no_tris] = imax[no_tris] = si["m_World"][no_tris, 3, :3]
    inst_of = lambda refs: ((~refs.astype(np.int64)) & 0xFFFFFFFF) >> 2
    if n_tlas == 0:
        if n_inst:
            r = dump["rootLeaf"]
            if r >= 0 or ((~r) & 3) or n_inst != 1 or ((~r) >> 2) != 0:
                rep.add("tlas_root_leaf", 1, f"rootLeaf {r} for {n_inst} instances without an instance tree")
        levels = 0
    else:
        depth, _ = walk(rep, "tlas_", child, [0], lo=0, hi=n_tlas, allow_unreached=gpu_instance_tree)
        node, slot, refs = leaf_slots(child, depth)
        rep.flag("tlas_leaf_encoding", ((~refs.astype(np.int64)) & 3) != 0, "instance leaves with a count field", lambda i: f"node4 {node[i]} slot {slot[i]}")
        ids = inst_of(refs)
        rep.flag("tlas_leaf_range", ids >= n_inst, "instance leaves past the instance table", lambda i: f"node4 {node[i]} slot {slot[i]}")
        seen = np.bincount(ids[ids < n_inst], minlength=n_inst)
        rep.flag("tlas_instance_unreferenced", seen == 0, "instances that no leaf references", lambda i: f"instance {i}")
        rep.flag("tlas_instance_in_two_leaves", seen > 1, "instances that more than one leaf references", lambda i: f"instance {i}")
        smin, smax = reference_boxes(child[:n_tlas], depth[:n_tlas], lambda r: imin[np.minimum(inst_of(r), n_inst - 1)], lambda r: imax[np.minimum(inst_of(r), n_inst - 1)])
        check_boxes(rep, "tlas_", child[:n_tlas], depth[:n_tlas], bmin[:n_tlas], bmax[:n_tlas], smin, smax)
        rep.flag("tlas_underfull", ((child[:n_tlas] != EMPTY).sum(1) < 2) & (depth[:n_tlas] > 0), "non-root 4-wide nodes with fewer than two children")
        levels = int(depth.max()) + 1
        occ_tlas = worst_stack_occupancy(child[:n_tlas], depth[:n_tlas])
    rep.stats.update(true_levels_tlas=levels, reported_levels_tlas=dump["maxDepth4Tlas"])
    if dump["maxDepth4Tlas"] < levels:
        rep.add("depth4_tlas_too_small", 1, f"maxDepth4Tlas {dump['maxDepth4Tlas']} reported, the instance tree has {levels} levels")
    elif dump["maxDepth4Tlas"] != levels:
        rep.add("depth4_tlas_not_exact", 1, f"maxDepth4Tlas {dump['maxDepth4Tlas']} reported, {levels} expected")
    if dump["maxDepth4"] != dump["maxDepth4Tlas"] + dump["maxDepth4Blas"]:
        rep.add("depth4_sum", 1, "maxDepth4 is not maxDepth4Tlas + maxDepth4Blas")
    # bvh_build.h two_level_stack_need from the reported levels, against what the dumped trees can make pending: the instance tree's siblings,
    # the marker pushed on entering an instance, the mesh tree's siblings
    need = 3 * (dump["maxDepth4Tlas"] + dump["maxDepth4Blas"]) + 3
    rep.stats.update(two_level_worst_stack_occupancy=occ_tlas + 1 + occ_blas, two_level_stack_need=need)
    if occ_tlas + 1 + occ_blas > need:
        rep.add("two_level_stack_need", 1, f"a traversal can hold {occ_tlas + 1 + occ_blas} entries, two_level_stack_need gives {need}")

    # ---- the culling slack of every instance (bvh_build.cpp rebuild_two_level_instances, HostInstance in bvh_build.h): invNorm = largest column sum
    # of |inv|, objMaxAbs = the mesh box's largest |coordinate| * (1 + 1e-5) + 1e-6, boxEps = 8 * 2.4e-7 * max(largest |coordinate| of the unpadded
    # world box, objMax * (largest column sum of |world|) + largest |translation|) * invNorm. Restated in binary64 from the record's own inv and the
    # mesh extents; each is a handful of binary32 operations in the product, so 16 * 2^-24 relative is allowed.
    inv3, w3 = np.abs(insts["inv"][:, :3, :].astype(np.float64)), np.abs(si["m_World"][:, :3, :3].astype(np.float64))
    inv_norm = inv3.sum(1).max(1)
    has_tris = np.isfinite(mesh_min[insts["mesh"]]).all(1)
    om = np.where(has_tris, np.maximum(np.abs(mesh_min[insts["mesh"]]), np.abs(mesh_max[insts["mesh"]])).max(1).astype(np.float64), 0.0)
    wmin, wmax = instance_world_boxes(scene, mesh_min, mesh_max, padded=False)
    max_abs = np.where(has_tris, np.maximum(np.abs(wmin), np.abs(wmax)).max(1).astype(np.float64), 0.0)
    eps = 8.0 * float(F(2.4e-7)) * np.maximum(max_abs, om * w3.sum(1).max(1) + np.abs(si["m_World"][:, 3, :3].astype(np.float64)).max(1)) * inv_norm
    tol = 16 * 2.0 ** -24
    close = lambda got, want: np.abs(got.astype(np.float64) - want) <= tol * np.abs(want)
    rep.flag("inst_inv_norm", ~close(insts["invNorm"], inv_norm), "instance records whose invNorm is not the largest column sum of |inv|", lambda i: f"instance {i}")
    rep.flag("inst_obj_max_abs", ~close(insts["objMaxAbs"], om * (1.0 + 1e-5) + 1e-6), "instance records whose objMaxAbs is not the mesh box's", lambda i: f"instance {i}")
    rep.flag("inst_box_eps", ~close(insts["boxEps"], eps), "instance records whose boxEps is not the documented slack", lambda i: f"instance {i}")

    # ---- each instance-leaf box around the world-space vertices the FLAT build of the same scene stores
    if flat_dump is not None and len(flat_dump["triangles"]):
        ft = flat_dump["triangles"]
        wlo = np.full((n_inst, 3), np.inf, F); whi = np.full((n_inst, 3), -np.inf, F)
        for k in ("p0", "p1", "p2"):
            np.minimum.at(wlo, ft["inst"], ft[k]); np.maximum.at(whi, ft["inst"], ft[k])
        has = np.isfinite(wlo).all(1)
        rep.flag("inst_box_not_containing", has & ~((imin <= wlo) & (imax >= whi)).all(1), "instance boxes that do not contain the instance's world-space vertices",
                 lambda i: f"instance {i}")
    return rep
