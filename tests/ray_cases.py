"""Scenes and rays of the geometric hit tests (tests/test_ray_geometry_cpu.py, tests/test_ray_geometry_gpu.py). All materials opaque.

Everything here is an INPUT: scenes are built with hobbyrenderer_amd.scenes / bvh_scenes, rays are constructed in float64 and rounded once to
the fp32 records the kernels read. No case consults the oracle, a kernel or the reference to choose its rays. A case is
(scene, rays, world triangles); `table(case)` is its reference (ray_reference.RayTable), computed once per process and shared."""
import math

import numpy as np

from hobbyrenderer_amd import scenes, structs as S

import bvh_reference
import bvh_scenes
import ray_reference

f32 = np.float32

SOUP_FRAMES = {"unit": (1.0, 0.0), "milli": (1e-3, 0.0), "kilo": (1e3, 0.0), "offset1e3": (1.0, 1e3), "offset1e5": (1.0, 1e5)}
SOUP_SIZES = {"lds": 400, "global": 3500}           # which side of pick_variant's LDS limit each is on is asserted by the GPU test
SOUP_RAYS = {"lds": 3000, "global": 2400}           # rays x triangles stays below 10^7 per case
EDGE_RAYS = {"lds": 2400, "global": 1500}


class Case:
    def __init__(self, name, scene, rays, kind):
        self.name, self.scene, self.rays, self.kind = name, scene, rays, kind
        self.tris = bvh_reference.expected_triangles(scene)
        self._table = None

    @property
    def table(self):
        if self._table is None:
            self._table = ray_reference.RayTable(self.tris, self.rays)
        return self._table


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _rays(o, d, tmin=0.0, tmax=1e10):
    r = np.zeros(len(o), S.Ray)
    r["origin"] = np.asarray(o, np.float64).astype(f32)
    r["direction"] = np.asarray(d, np.float64).astype(f32)
    r["tmin"] = tmin
    r["tmax"] = tmax
    return r


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _interior(rng, tri, lo=0.0):
    """Random points of triangles [n, 3, 3] (float64) with every barycentric above `lo`."""
    b = rng.dirichlet((1.0, 1.0, 1.0), len(tri)) * (1.0 - 3.0 * lo) + lo
    return (tri * b[:, :, None]).sum(1)


# ---------------------------------------------------------------------------------------------------------------- soups at scale and offset
def soup_triangles(n, scale, offset, seed=11):
    return (bvh_scenes.random_triangles(n, seed).astype(np.float64) * scale + offset).astype(f32)


def soup_scene(luts, size, frame):
    scale, offset = SOUP_FRAMES[frame]
    return cached(("soup", size, frame), lambda: bvh_scenes.triangle_scene(luts, soup_triangles(SOUP_SIZES[size], scale, offset)))


def soup_case(luts, size, frame):
    """Half the rays aimed at random interior points, half random directions; origins in the scene's frame; a third each with unit directions
    and directions scaled by 1e-3 / 1e3 (t scales inversely); 30 % with a finite tmax around the distance of the aimed point (of the scene's
    extent for the unaimed ones), a quarter with tmin > 0 in front of the aimed point."""
    def make():
        sc = soup_scene(luts, size, frame)
        scale, offset = SOUP_FRAMES[frame]
        n = SOUP_RAYS[size]
        rng = np.random.default_rng(101 + n)
        tris = bvh_reference.expected_triangles(sc)["pos"].astype(np.float64)
        o = (offset + scale * rng.uniform(-2.5, 2.5, (n, 3))).astype(f32).astype(np.float64)
        aimed = np.arange(n) % 2 == 0
        target = _interior(rng, tris[rng.integers(0, len(tris), n)])
        to = target - o
        dist = np.linalg.norm(to, axis=1)
        d = np.where(aimed[:, None], to / dist[:, None], _unit(rng, n))
        length = np.array([1.0, 1e-3, 1e3])[(np.arange(n) // 2) % 3]
        d = d * length[:, None]
        t_ref = np.where(aimed, dist, 3.0 * scale) / length
        tmax = np.where(rng.random(n) < 0.7, 1e10, t_ref * rng.uniform(0.5, 1.5, n))
        tmin = np.where(rng.random(n) < 0.75, 0.0, 0.25 * t_ref)
        return Case(f"soup-{size}-{frame}", sc, _rays(o, d, tmin, tmax), "interior")
    return cached(("soup_case", size, frame), make)


def edge_case(luts, size, frame):
    """Rays through fp32-rounded vertices, edge midpoints and random edge points of the same soups (a quarter, a quarter, half), continued to an
    interior point of ANOTHER triangle: the pair with the edge's owner is ambiguous by construction, the triangle behind gives the decided bound."""
    def make():
        sc = soup_scene(luts, size, frame)
        n = EDGE_RAYS[size]
        rng = np.random.default_rng(202 + n)
        tris = bvh_reference.expected_triangles(sc)["pos"].astype(np.float64)
        k = rng.integers(0, len(tris), n)
        e = rng.integers(0, 3, n)
        s = np.where(np.arange(n) % 4 == 0, 0.0, np.where(np.arange(n) % 4 == 1, 0.5, rng.uniform(0.0, 1.0, n)))
        pa, pb = tris[k, e], tris[k, (e + 1) % 3]
        point = (pa * (1.0 - s)[:, None] + pb * s[:, None]).astype(f32).astype(np.float64)
        k2 = (k + rng.integers(1, len(tris), n)) % len(tris)
        q = _interior(rng, tris[k2], lo=0.1)
        alpha = rng.uniform(0.3, 1.0, n)[:, None]
        o = (point - (q - point) * alpha).astype(f32).astype(np.float64)
        d = (point - o) / alpha                               # t = alpha at the edge point, about 1 + alpha behind it
        return Case(f"edges-{size}-{frame}", sc, _rays(o, d), "edges")
    return cached(("edge_case", size, frame), make)


# ---------------------------------------------------------------------------------------------------------------- closed meshes
def _closed_sphere(seed=5, n_lon=12, n_lat=8):
    """scenes.mesh_sphere with vertices jittered to non-dyadic positions and its parametric seam and poles WELDED (equal positions for the
    duplicated grid vertices), so that the surface is closed: every edge is shared by two triangles with bit-identical end points. The
    triangles of the pole rows that collapse to a segment have zero area."""
    verts, idx = scenes.mesh_sphere(n_lon, n_lat, 1.0)
    rng = np.random.default_rng(seed)
    pos = verts["m_Pos"].astype(np.float64).reshape(n_lat + 1, n_lon + 1, 3)
    pos = pos * rng.uniform(0.93, 1.07, pos.shape[:2] + (1,)) + rng.uniform(-0.02, 0.02, pos.shape)
    pos[:, -1] = pos[:, 0]
    pos[0, :] = pos[0, 0]
    pos[-1, :] = pos[-1, 0]
    verts = verts.copy()
    verts["m_Pos"] = pos.reshape(-1, 3).astype(f32)
    return verts, idx


def _rot(ax, ay):
    ry = np.array([[math.cos(ax), 0, -math.sin(ax)], [0, 1, 0], [math.sin(ax), 0, math.cos(ax)]])
    rx = np.array([[1, 0, 0], [0, math.cos(ay), math.sin(ay)], [0, -math.sin(ay), math.cos(ay)]])
    return ry @ rx


def closed_worlds(offset=0.0, moved=False):
    """World matrices of the two instances: rotation + non-uniform scale; mirrored (negative determinant). `moved`: the small motion of the refit."""
    shift = np.array([0.013, -0.007, 0.021]) if moved else np.zeros(3)
    a = scenes._mat((0.9, 1.3, 0.7), _rot(0.7, -0.4), tuple(np.array([-2.0, 0.1, 0.3]) + offset + shift))
    b = scenes._mat((-1.1, 0.8, 1.2), _rot(-1.1, 0.25), tuple(np.array([2.0, -0.2, 0.1]) + offset - shift))
    return [a, b]


def closed_scene(luts, offset=0.0, moved=False):
    def make():
        b = scenes.SceneBuilder()
        mesh = b.add_mesh(*_closed_sphere())
        mat = b.add_material()
        for w in closed_worlds(offset, moved):
            b.add_instance(mesh, mat, w)
        return b.finalize(luts)
    return cached(("closed", offset, moved), make)


def closed_case(luts, offset=0.0, moved=False, random_dirs=300, per_edge=8):
    """From origins within 0.25 of each instance's centre (the surface is more than 0.4 away): rays at every vertex, every edge midpoint,
    `per_edge` random points of every edge and random directions. Directions are target - origin (t = 1 at the target), random ones unit."""
    def make():
        sc = closed_scene(luts, offset, moved)
        tris = bvh_reference.expected_triangles(sc)
        rng = np.random.default_rng(303)
        os_, ds = [], []
        for inst, w in enumerate(closed_worlds(offset, moved)):
            p = tris["pos"][tris["owner"] == inst].astype(np.float64)
            centre = np.asarray(w)[3, :3]
            vert = np.unique(p.reshape(-1, 3), axis=0)
            edges = np.concatenate([np.stack([p[:, i], p[:, (i + 1) % 3]], 1) for i in range(3)])
            edges = edges[(edges[:, 0] != edges[:, 1]).any(1)]
            flip = np.array([tuple(a) > tuple(b) for a, b in edges])
            edges[flip] = edges[flip][:, ::-1]
            edges = np.unique(edges.reshape(-1, 6), axis=0).reshape(-1, 2, 3)
            s = np.concatenate([np.full((len(edges), 1), 0.5), rng.uniform(0.0, 1.0, (len(edges), per_edge))], 1)
            on_edge = (edges[:, None, 0] * (1.0 - s)[..., None] + edges[:, None, 1] * s[..., None]).reshape(-1, 3)
            target = np.concatenate([vert, on_edge]).astype(f32).astype(np.float64)
            ball = _unit(rng, len(target) + random_dirs) * (0.25 * rng.random((len(target) + random_dirs, 1)) ** (1 / 3))
            o = (centre + ball).astype(f32).astype(np.float64)
            d = np.concatenate([target - o[:len(target)], _unit(rng, random_dirs)])
            os_.append(o); ds.append(d)
        return Case(f"closed-{offset:g}{'-moved' if moved else ''}", sc, _rays(np.concatenate(os_), np.concatenate(ds)), "closed")
    return cached(("closed_case", offset, moved, random_dirs, per_edge), make)


def gbuffer_case(luts, width=64, height=36):
    """The camera inside the first closed mesh: (scene, constants, case) with the primary rays of gbuffer_reference as the case's rays."""
    def make():
        import gbuffer_reference as G
        sc = closed_scene(luts)
        centre = np.asarray(closed_worlds()[0])[3, :3]
        view, pos = scenes.planar_view(width, height, position=tuple(centre + [0.05, -0.03, 0.02]), yaw=0.6, pitch=0.2, fov_y=math.radians(75.0))
        cb = scenes.fill_constants(view, pos, sc, 2, 1)
        o, d, _ = G.primary_rays(cb, width, height)
        rays = np.zeros(width * height, S.Ray)
        rays["origin"] = o
        rays["direction"] = d.reshape(-1, 3)
        rays["tmax"] = G.MISS_T
        return sc, cb, Case("gbuffer-closed", sc, rays, "closed")
    return cached(("gbuffer", width, height), make)


# ---------------------------------------------------------------------------------------------------------------- degenerate directions
def axis_case(luts):
    """The 400-triangle unit soup under directions with one and two zero components (+0.0 and -0.0), denormal components (1e-40), through
    vertices (the origin's other coordinates EQUAL the vertex's) and through interior points."""
    def make():
        sc = soup_scene(luts, "lds", "unit")
        tris = bvh_reference.expected_triangles(sc)["pos"]
        rng = np.random.default_rng(404)
        o, d = [], []
        for i in range(900):
            k = int(rng.integers(0, len(tris)))
            at_vertex = i % 2 == 0
            p = tris[k, i % 3].astype(np.float64) if at_vertex else _interior(rng, tris[k:k + 1].astype(np.float64), 0.1)[0].astype(f32).astype(np.float64)
            a = (i // 2) % 3
            sign = 1.0 if (i // 6) % 2 else -1.0
            style = (i // 12) % 4
            dirn = np.zeros(3)
            dirn[a] = -sign
            if style == 1:
                dirn[(a + 1) % 3] = -0.0; dirn[(a + 2) % 3] = -0.0
            elif style == 2:
                dirn[(a + 1) % 3] = 1e-40; dirn[(a + 2) % 3] = -1e-40 if i % 5 else 0.0
            elif style == 3:                                  # one zero component: the ray stays in the plane of coordinate a + 2
                dirn[(a + 1) % 3] = rng.uniform(-1.0, 1.0)
            org = p - dirn * 2.0                             # exact for the zero components: those coordinates stay the point's
            o.append(org); d.append(dirn)
        return Case("axis-directions", sc, _rays(np.array(o), np.array(d)), "axis")
    return cached("axis_case", make)


def degenerate_case(luts, which):
    """`planar`: the 64 overlapping triangles in the plane y = 0.25 under rays exactly in that plane and rays parallel to it: all misses. (Rays
    ACROSS the plane are left out on purpose: the triangles overlap, every one a ray crosses has the same float64 t, their fp32 t differ by
    rounding, and the tie rule of the verdict presumes exact ties as on dyadic inputs.) `zero_area`: rays at the
    end points and at points of the collapsed triangles, and at interior points of the proper ones."""
    def make():
        t = bvh_scenes.degenerate_sets()[which]
        sc = bvh_scenes.triangle_scene(luts, t)
        tris = bvh_reference.expected_triangles(sc)["pos"].astype(np.float64)
        rng = np.random.default_rng(505)
        n = 600
        k = rng.integers(0, len(tris), n)
        s = rng.uniform(0, 1, (n, 1))
        if which == "planar":
            target = _interior(rng, tris[k])
            ang = rng.uniform(0, 2 * math.pi, n)
            in_plane = np.arange(n) % 2 == 0
            d = np.stack([np.cos(ang), np.where(np.arange(n) % 4 == 0, 0.0, -0.0), np.sin(ang)], 1)
            o = target - d * rng.uniform(0.5, 3.0, (n, 1))
            o[:, 1] = np.where(in_plane, 0.25, 0.25 + rng.choice([-0.5, 0.0078125, 2.0], n))      # in the plane / parallel to it, off it
        else:
            collapsed = np.arange(n) % 2 == 0
            kk = np.where(collapsed, (k // 3) * 3 + (np.arange(n) // 2) % 2, k) % len(tris)
            target = np.where(collapsed[:, None], tris[kk, 0] * (1 - s) + tris[kk, 1] * s, _interior(rng, tris[kk]))
            target = target.astype(f32).astype(np.float64)
            o = (rng.uniform(-2.5, 2.5, (n, 3))).astype(f32).astype(np.float64)
            d = target - o
        return Case(f"degenerate-{which}", sc, _rays(o, d), "degenerate")
    return cached(("degenerate", which), make)


# ---------------------------------------------------------------------------------------------------------------- interval ends, exact
def interval_scene(luts):
    """One dyadic triangle per axis in the plane coordinate = 2 (for an origin at the origin), oriented both ways."""
    base = np.array([[-1.0, -1.0, 2.0], [3.0, -1.0, 2.0], [-1.0, 3.0, 2.0]])
    tris = []
    for a in range(3):
        perm = [(a + 1) % 3, (a + 2) % 3, a]
        t = np.zeros((3, 3)); t[:, perm] = base
        tris.append(t + 16.0 * a)                             # apart from each other; still dyadic
        tris.append((t + 16.0 * a)[::-1] * [1, 1, 1])
    return cached("interval_scene", lambda: bvh_scenes.triangle_scene(luts, np.array(tris, f32)))


def interval_rays():
    """(rays, expected hit flags, labels): axis-parallel rays whose hit is at t == 2.0 EXACTLY in fp32 (edge functions -8, -4, -4 or 8, 4, 4 in
    some order: det = +-16, T = +-32; origins shifted by dyadic amounts keep every operation exact), under the interval ends of the issue."""
    two = f32(2.0)
    ends = [("tmax=2", 0.0, two, False), ("tmax=next(2)", 0.0, np.nextafter(two, f32(np.inf)), True), ("tmin=2", two, 1e10, False),
            ("tmin=prev(2)", np.nextafter(two, f32(0)), 1e10, True), ("tmin=tmax", f32(1.5), f32(1.5), False), ("tmin>tmax", f32(3.0), f32(1.0), False),
            ("tmax=inf", 0.0, np.inf, True), ("plain", 0.0, 1e10, True)]
    o, d, lo, hi, want, label = [], [], [], [], [], []
    for a in range(3):
        for sign in (1.0, -1.0):
            for shift in ((0.0, 0.0), (0.25, 0.5)):
                for name, t0, t1, hit in ends:
                    org = np.full(3, 16.0 * a)
                    org[(a + 1) % 3] += shift[0]; org[(a + 2) % 3] += shift[1]
                    dirn = np.zeros(3); dirn[a] = sign
                    if sign < 0:
                        org[a] += 4.0                         # from the other side: the plane is again 2 away
                    o.append(org); d.append(dirn); lo.append(t0); hi.append(t1); want.append(hit); label.append(f"axis {a} sign {sign:+.0f} shift {shift} {name}")
    return _rays(np.array(o), np.array(d), np.array(lo, f32), np.array(hi, f32)), np.array(want), label


# ---------------------------------------------------------------------------------------------------------------- non-finite and zero rays
def nonfinite_rays(frame_offset=0.0):
    """NaN in origin or direction, +-inf components, direction (0, 0, 0): each must give a miss (hit == 0) and visibility 1."""
    nan, inf = np.nan, np.inf
    good_o, good_d = (0.1, 0.2, -2.5), (0.05, -0.1, 1.0)
    cases = [((nan, 0, 0), good_d), ((0, nan, 0), good_d), ((0, 0, nan), good_d), (good_o, (nan, 0, 1)), (good_o, (0, nan, 1)), (good_o, (0, 1, nan)),
             (good_o, (inf, 0, 0)), (good_o, (-inf, 0, 0)), (good_o, (0, inf, 1)), (good_o, (1, 1, -inf)), (good_o, (inf, inf, 1)), (good_o, (inf, -inf, inf)),
             ((inf, 0, 0), good_d), ((0, -inf, 0), good_d), ((inf, inf, inf), good_d), ((0, 0, inf), (0, 0, 1)), ((0, 0, -inf), (0, 0, -1)),
             (good_o, (0, 0, 0)), (good_o, (0, -0.0, 0)), ((0, 0, 0), (0, 0, 0))]
    r = _rays(np.array([c[0] for c in cases], np.float64) + frame_offset, np.array([c[1] for c in cases], np.float64))
    return r
