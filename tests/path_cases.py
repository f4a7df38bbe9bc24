"""Small scenes in which every branch of the path tracer's loop is reached -- TEST INFRASTRUCTURE.

Built with scenes.SceneBuilder from the unit quad and the unit cube (vertex positions +-0.5, axis-aligned normals) under scales and
translations that are small dyadic rationals, so the quantised geometry is the intended geometry and every world vertex is exact in
binary32. At most a few dozen triangles and 6 bounces per case.

  A  closed box, coloured diffuse walls, emissive ceiling patch, a metal, a half-metallic and a rough dielectric block; the sun (occluded
     everywhere, its draws still consumed where the cull passes), a point light whose range cuts off part of the box, a spot light
  B  the box lit by the patch alone (and the occluded sun): a thick smooth and a thick rough absorbing glass slab, a thin transmissive
     BLEND pane, a thin BLEND pane without transmission (the stochastic candidate commit of TraceRayStandard)
  C  open sky, sun only: a floor, a block and two mirrors in a courtyard whose walls are higher than every camera; probe 2 is a long lens
     into the sun, probe 3 a long lens whose two specular bounces leave towards the sun
  D  A with 1 x 1 albedo (sRGB), roughness-metallic and emissive textures bound to every material, and the sun first in the light list
  E  filtered shadows: a point light above a BLEND pane and a strongly absorbing slab with part of the floor seeing it directly, and a
     second point light inside the slab (the open medium segment up to TMax)

Per case: one pinhole camera at 40 x 23 at two accumulation indices and six 8 x 8 probe cameras at an interior point; camera (first index)
plus probes are the 1 304 rays of `batch`, which crosses a 1 024-sample segment; `free_rays` adds 1 061 rays no camera makes."""
import math

import numpy as np

from hobbyrenderer_amd import scenes, structs as S
import gbuffer_reference as G

NAMES = ("A", "B", "C", "D", "E")
W, H = 40, 23
INDICES = (0, 3)
PROBE_N, PROBE_INDEX = 8, 2
FREE_RAYS = 1061
FACES = [(math.pi / 2, 0.0), (-math.pi / 2, 0.0), (0.0, -math.pi / 2), (0.0, math.pi / 2), (0.0, 0.0), (math.pi, 0.0)]      # (yaw, pitch): +x -x +y -y +z -z
BLEND = S.ALPHA_MODE_BLEND
_mat, _ROT = scenes._mat, scenes._ROT_TO


class Case:
    def __init__(self, name, scene, bounces, camera, probe, free_box, solids, lenses=None):
        self.name, self.scene, self.bounces, self.camera, self.probe, self.free_box, self.solids = name, scene, bounces, camera, probe, free_box, solids
        self.lenses = lenses or {}              # probe k -> planar_view arguments that replace the 90-degree face

    def views(self):
        """[(label, constants, width, height)]: the camera at both indices, then the six probes."""
        out = []
        for index in INDICES:
            view, pos = scenes.planar_view(W, H, **self.camera)
            out.append((f"camera@{index}", scenes.fill_constants(view, pos, self.scene, index, self.bounces), W, H))
        for k, (yaw, pitch) in enumerate(FACES):
            kw = dict(position=self.probe, yaw=yaw, pitch=pitch, fov_y=math.pi / 2, aspect=1.0)
            kw.update(self.lenses.get(k, {}))
            view, pos = scenes.planar_view(PROBE_N, PROBE_N, **kw)
            out.append((f"probe{k}", scenes.fill_constants(view, pos, self.scene, PROBE_INDEX, self.bounces), PROBE_N, PROBE_N))
        return out

    def constants(self):
        return self.views()[0][1]

    def batch(self):
        """The 1 304 rays: camera at the first index, then the probes, as S.Ray records."""
        v = self.views()
        return np.concatenate([rays_of(cb, w, h) for _, cb, w, h in [v[0]] + v[len(INDICES):]])

    def free_rays(self, n=FREE_RAYS, seed=11):
        """Rays no camera makes: origins in free space (outside every block and slab), unit directions, tmin in {0, 1e-4}, random states."""
        rng = np.random.default_rng(seed)
        lo, hi = (np.asarray(a, np.float64) for a in self.free_box)
        o = np.zeros((0, 3))
        while len(o) < n:
            p = lo + rng.random((4 * n, 3)) * (hi - lo)
            inside = np.zeros(len(p), bool)
            for c, half in self.solids:
                inside |= (np.abs(p - np.asarray(c)) <= np.asarray(half) + 0.05).all(1)
            o = np.concatenate([o, p[~inside]])
        r = np.zeros(n, S.Ray)
        r["origin"] = o[:n].astype(np.float32)
        d = rng.normal(size=(n, 3))
        r["direction"] = (d / np.sqrt((d ** 2).sum(1, keepdims=True))).astype(np.float32)
        r["tmin"] = np.where(rng.random(n) < 0.5, 0.0, 1e-4).astype(np.float32)
        r["tmax"] = np.float32(1e10)
        r["rng"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        return r


def rays_of(cb, w, h):
    """The primary rays of every pixel for `cb` as S.Ray records, row-major."""
    o, d, seed = G.primary_rays(cb, w, h)
    rays = np.zeros(w * h, S.Ray)
    rays["origin"] = o; rays["direction"] = d.reshape(-1, 3); rays["tmin"] = 0.0; rays["tmax"] = np.float32(1e10); rays["rng"] = seed.reshape(-1)
    return rays


# ---------------------------------------------------------------------------------------------------------------- materials
class _Materials:
    """add(...) makes a material from constants, or, textured, from 1 x 1 textures that hold them (the factors then are 1)."""

    def __init__(self, builder, textured):
        self.b, self.textured = builder, textured

    def add(self, color=(1, 1, 1), alpha=1.0, rough=1.0, metal=0.0, emissive=(0, 0, 0), **kw):
        if not self.textured:
            return self.b.add_material(m_BaseColor=(*color, alpha), m_RoughnessMetallic=(rough, metal), m_EmissiveFactor=(*emissive, 1), **kw)
        byte = lambda x: int(round(255 * x))
        scale = max(max(emissive), 1.0)
        albedo = S.Texture(np.array([[[byte(c) for c in color] + [255]]], np.uint8), 1, 1, S.TEXTURE_FORMAT_RGBA8_SRGB)
        rm = np.array([[[0, byte(rough), byte(metal), 255]]], np.uint8)
        em = np.array([[[byte(e / scale) for e in emissive] + [255]]], np.uint8)
        ta, tr, te = self.b.add_texture(albedo), self.b.add_texture(rm), self.b.add_texture(em)
        return self.b.add_material(m_BaseColor=(1, 1, 1, alpha), m_RoughnessMetallic=(1, 0), m_EmissiveFactor=(scale, scale, scale, 1),
                                   m_TextureFlags=S.TEXFLAG_ALBEDO | S.TEXFLAG_ROUGHNESS_METALLIC | S.TEXFLAG_EMISSIVE,
                                   m_AlbedoTextureIndex=ta, m_RoughnessMetallicTextureIndex=tr, m_EmissiveTextureIndex=te, **kw)


def _box(b, m, patch=(17, 12, 4)):
    """The closed room x [-1, 1], y [0, 2], z [-2, 2] with an emissive patch under the ceiling. Returns (quad mesh, cube mesh)."""
    quad, cube = b.add_mesh(*scenes.generate_floor_quad()), b.add_mesh(*scenes.generate_default_cube())
    white, red, green = m.add((0.73, 0.73, 0.73)), m.add((0.65, 0.05, 0.05)), m.add((0.12, 0.45, 0.15))
    blue, light = m.add((0.2, 0.3, 0.7), rough=0.8), m.add((0.78, 0.78, 0.78), emissive=patch)
    b.add_instance(quad, white, _mat((2, 1, 4), _ROT["+y"], (0, 0, 0)))
    b.add_instance(quad, white, _mat((2, 1, 4), _ROT["-y"], (0, 2, 0)))
    b.add_instance(quad, red, _mat((2, 1, 4), _ROT["+x"], (-1, 1, 0)))
    b.add_instance(quad, green, _mat((2, 1, 4), _ROT["-x"], (1, 1, 0)))
    b.add_instance(quad, blue, _mat((2, 1, 2), _ROT["-z"], (0, 1, 2)))
    b.add_instance(quad, white, _mat((2, 1, 2), _ROT["+z"], (0, 1, -2)))
    b.add_instance(quad, light, _mat((0.75, 1, 0.75), _ROT["-y"], (0, 1.984375, 0.25)))
    # a roof above the room: a sun shadow ray that starts within its 0.01 bias of the ceiling skips the ceiling, and ends here
    b.add_instance(quad, white, _mat((16, 1, 16), _ROT["-y"], (0, 2.25, 0)))
    return quad, cube


BLOCKS = [((-0.5, 0.375, 0.75), (0.25, 0.375, 0.25)), ((0.4375, 0.25, 0.25), (0.3125, 0.25, 0.25)), ((0.0, 0.125, -0.5), (0.25, 0.125, 0.25))]


def _blocks(b, m, cube):
    metal = m.add((0.9, 0.7, 0.4), rough=0.3, metal=1.0)
    half = m.add((0.6, 0.6, 0.8), rough=0.45, metal=0.5)
    rough = m.add((0.8, 0.5, 0.3), rough=0.6)
    for mat, (c, h) in zip((metal, half, rough), BLOCKS):
        b.add_instance(cube, mat, _mat(tuple(2 * x for x in h), None, c))


_SUN = np.array([0.3, 0.8, -0.52]) / math.sqrt(0.3 ** 2 + 0.8 ** 2 + 0.52 ** 2)      # oblique to every wall: no dot(N, sun) is exactly 0


def _finish(b, luts, sun_first=False):
    sc = b.finalize(luts)
    sc.sun_direction = _SUN.astype(np.float32)
    if sun_first:                                  # g_Lights[0] is the sun (finalize orders spot, point, directional)
        sc.lights = np.ascontiguousarray(np.concatenate([sc.lights[-1:], sc.lights[:-1]]))
    return sc


ROOM_BOX = ((-0.9, 0.1, -1.9), (0.9, 1.9, 1.9))
ROOM_CAMERA = dict(position=(0.0625, 1.0, -1.875), pitch=math.radians(8.0), fov_y=math.radians(62.0))


def _case_a(luts, textured=False):
    b = scenes.SceneBuilder()
    m = _Materials(b, textured)
    quad, cube = _box(b, m)
    _blocks(b, m, cube)
    b.add_light(S.LIGHT_POINT, position=(0.5, 1.5, -0.5), color=(1.0, 0.9, 0.8), intensity=4.0, radius=0.03125, range_=1.75)
    b.add_light(S.LIGHT_SPOT, position=(-0.5, 1.75, -0.8125), direction=(0.25, -1.0, 0.5), color=(0.6, 0.7, 1.0), intensity=8.0, radius=0.015625,
                inner=0.3, outer=0.55)
    # A keeps finalize's order, so g_Lights[0] -- whose intensity scales the sun and the sky -- is the spot light; D puts the sun first
    return Case("D" if textured else "A", _finish(b, luts, sun_first=textured), 5, ROOM_CAMERA, (0.125, 1.0, -0.75), ROOM_BOX, BLOCKS)


def _case_b(luts):
    b = scenes.SceneBuilder()
    m = _Materials(b, False)
    quad, cube = _box(b, m, patch=(34, 24, 8))
    glass = m.add((0.95, 0.97, 1.0), rough=0.05, m_AlphaMode=BLEND, m_TransmissionFactor=1.0, m_IOR=1.5, m_SigmaA=(2.0, 1.0, 0.5))
    frosted = m.add((1.0, 0.95, 0.9), rough=0.3, m_AlphaMode=BLEND, m_TransmissionFactor=1.0, m_IOR=1.5, m_SigmaA=(0.5, 1.0, 2.0))
    pane = m.add((0.8, 0.9, 1.0), alpha=0.5, rough=0.05, m_AlphaMode=BLEND, m_TransmissionFactor=0.75, m_IOR=1.5, m_IsThinSurface=1)
    veil = m.add((0.9, 0.6, 0.6), alpha=0.5, rough=0.5, m_AlphaMode=BLEND, m_IOR=1.5, m_IsThinSurface=1)
    solids = [((-0.4375, 0.625, 0.5), (0.375, 0.375, 0.1875)), ((0.5, 0.5, 0.0), (0.25, 0.375, 0.3125))]
    b.add_instance(cube, glass, _mat(tuple(2 * x for x in solids[0][1]), None, solids[0][0]))
    b.add_instance(cube, frosted, _mat(tuple(2 * x for x in solids[1][1]), None, solids[1][0]))
    b.add_instance(quad, pane, _mat((0.75, 1, 0.75), _ROT["-z"], (-0.375, 1.25, -0.5)))
    b.add_instance(quad, veil, _mat((0.75, 1, 1.0), _ROT["-z"], (0.5, 0.5, -0.75)))
    return Case("B", _finish(b, luts), 6, ROOM_CAMERA, (0.0625, 0.75, -1.25), ROOM_BOX, solids)


def _case_c(luts):
    b = scenes.SceneBuilder()
    m = _Materials(b, False)
    quad, cube = b.add_mesh(*scenes.generate_floor_quad()), b.add_mesh(*scenes.generate_default_cube())
    b.add_instance(quad, m.add((0.6, 0.55, 0.5), rough=0.7), _mat((8, 1, 8), None, (0, 0, 0)))
    # a courtyard: walls higher than every camera and surface, so that no ray reaches the ground below the horizon, where the sky lookup
    # of a camera one metre above it is ill-conditioned in binary32 (atmosphere_reference.py: "rays grazing the ground are the worst")
    wall = m.add((0.5, 0.5, 0.55), rough=0.9)
    for side, at in (("+x", (-4, 1, 0)), ("-x", (4, 1, 0)), ("+z", (0, 1, -4)), ("-z", (0, 1, 4))):
        b.add_instance(quad, wall, _mat((2, 1, 8) if side[1] == "x" else (8, 1, 2), _ROT[side], at))
    solids = [((0.0, 0.5, 1.0), (0.5, 0.5, 0.5))]
    b.add_instance(cube, m.add((0.7, 0.7, 0.9), rough=0.35, metal=0.5), _mat((1, 1, 1), None, solids[0][0]))
    # Two mirrors (roughness 0.05) and two long lenses (0.37 degrees across). Probe 2 looks into the sun, whose disk (radius 0.27 degrees)
    # fills its 8 x 8 pixels. Probe 3 looks at the upright mirror along the sun's direction mirrored in x and y; its specular bounces go on
    # to the flat mirror and leave it towards the disk: misses after bounce 0 that would show a sun disk added there. Two mirrors, because
    # the specular direct light of the sun in a mirror that reflects the eye into it -- D_GGX at its peak, 1 - NdotH^2 ~ alpha^2 ~ 6e-6
    # -- is wrong by several per cent in binary32, and specular direct light is kept at bounce 0 only.
    shiny = m.add((0.95, 0.95, 0.95), rough=0.05, metal=1.0)
    upright, flat = np.array([-3.0, 1.0, 0.0]), np.array([-2.625, 0.0625, -0.625])
    b.add_instance(quad, shiny, _mat((1, 1, 1), _ROT["+x"], tuple(upright)))
    b.add_instance(quad, shiny, _mat((1, 1, 1), None, tuple(flat)))
    camera = dict(position=(0.75, 1.25, -3.0), yaw=math.radians(-10.0), pitch=math.radians(12.0), fov_y=math.radians(60.0))
    d1 = np.array([_SUN[0], -_SUN[1], _SUN[2]])                        # upright mirror -> flat mirror
    at = flat - d1 * ((upright[0] - flat[0]) / -d1[0])                  # where that line meets the upright mirror's plane
    d0 = np.array([-_SUN[0], -_SUN[1], _SUN[2]])                       # lens -> upright mirror
    lenses = {2: dict(yaw=math.atan2(_SUN[0], _SUN[2]), pitch=-math.asin(_SUN[1]), fov_y=0.0064),
              3: dict(position=tuple(at - 1.0 * d0), yaw=math.atan2(d0[0], d0[2]), pitch=-math.asin(d0[1]), fov_y=0.0064)}
    return Case("C", _finish(b, luts), 4, camera, (0.25, 1.5, -0.5), ((-3.0, 0.1, -3.0), (3.0, 1.9, 3.0)), solids, lenses)


def _case_e(luts):
    b = scenes.SceneBuilder()
    m = _Materials(b, False)
    quad, cube = _box(b, m, patch=(4, 3, 1))
    _blocks(b, m, cube)
    veil = m.add((0.9, 0.9, 0.6), alpha=0.5, rough=0.5, m_AlphaMode=BLEND, m_IOR=1.5, m_IsThinSurface=1)
    dark = m.add((1.0, 1.0, 1.0), rough=0.05, m_AlphaMode=BLEND, m_TransmissionFactor=1.0, m_IOR=1.5, m_SigmaA=(20.0, 24.0, 28.0))
    slab = ((0.5, 1.0, 0.0), (0.375, 0.125, 0.5))
    b.add_instance(quad, veil, _mat((1.0, 1, 1.5), _ROT["+y"], (-0.125, 1.25, 0.0)))
    b.add_instance(cube, dark, _mat(tuple(2 * x for x in slab[1]), None, slab[0]))
    b.add_light(S.LIGHT_POINT, position=(0.3125, 1.5, 0.0625), color=(1.0, 0.9, 0.8), intensity=6.0, radius=0.03125, range_=2.5)
    b.add_light(S.LIGHT_POINT, position=slab[0], color=(0.8, 0.9, 1.0), intensity=300.0, radius=0.015625)
    return Case("E", _finish(b, luts), 4, ROOM_CAMERA, (-0.25, 0.625, -0.75), ROOM_BOX, BLOCKS + [slab])


_BUILDERS = {"A": _case_a, "B": _case_b, "C": _case_c, "D": lambda luts: _case_a(luts, True), "E": _case_e}
_CACHE = {}


def case(name, luts):
    if name not in _CACHE:
        _CACHE[name] = _BUILDERS[name](luts)
    return _CACHE[name]
