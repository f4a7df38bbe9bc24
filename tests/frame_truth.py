"""Geometric ground truth for a pair of frames -- TEST INFRASTRUCTURE.

NumPy float64. What a frame IS comes from what the caller chose and from nothing a stage computed: the camera from position, yaw, pitch,
fov_y, aspect, size and jitter (never from the matrices, scale or bias of a view record); the geometry from the frame's own SceneArrays
(object-space vertices and m_World of THAT frame; m_PrevWorld is never read); hits by the brute force of path_reference /
surface_reference (every ray against every world triangle); texels by texture_reference through surface_reference; the sky of a miss by
atmosphere_reference. Nothing is taken from motion_reference, temporal_reference, upscale_reference or gbuffer_reference.

Conventions, as the caller's choices mean them (left-handed, x right, y up, window y down, pixel p covers [p, p + 1), the primary ray of
pixel p passes through the window position p + 0.5 + jitter):

    forward = (sin yaw cos pitch, -sin pitch, cos yaw cos pitch), right = normalize(cross((0, 1, 0), forward)), up = cross(forward, right)
    window(X) = ((1 + x / (z tx)) W / 2, (1 - y / (z ty)) H / 2) with (x, y, z) = (X - position) . (right, up, forward),
    ty = tan(fov_y / 2), tx = ty * aspect; z is the view depth.

For frame k, its predecessor and every pixel, pair_truth gives the hit of the primary ray (instance, primitive, u, v, with the margin of
path_reference), the world point X on the frame-k vertices, the previous world point X' (the same (u, v) on the previous frame's
vertices under the previous frame's world matrix), the previous window position w' (projected, then verified by casting: the ray through w'
must meet X' to 1e-9 of the scene's size, and the ray through window(X) must meet X and land on p + 0.5 + jitter), the true motion
w' - w and view-depth difference, and whether X' was visible in frame k - 1 (a brute-force segment test from the previous camera against
the previous frame's world triangles) with a margin: the least of the relative distance |t - dist| / dist to every other triangle the
segment's line crosses and of the clearance |c| of every other triangle's nearest edge in front of X'."""
import math

import numpy as np

import atmosphere_reference as A
import path_reference as R

F = np.float64
INF = np.inf
LOOP = 1e-9                      # closed loops hold to this share of the scene's size
FAR = F(np.float32(1e10))        # the primary ray's tmax, and the depth plane's value on a miss


class Camera:
    def __init__(self, width, height, position, yaw=0.0, pitch=0.0, fov_y=math.pi / 4, aspect=None, jitter=(0.0, 0.0)):
        self.width, self.height = int(width), int(height)
        self.position = np.asarray(position, F)
        self.yaw, self.pitch, self.fov_y = float(yaw), float(pitch), float(fov_y)
        self.aspect = self.width / self.height if aspect is None else float(aspect)
        self.jitter = (float(jitter[0]), float(jitter[1]))
        cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
        self.forward = np.array([sy * cp, -sp, cy * cp])
        right = np.cross([0.0, 1.0, 0.0], self.forward)
        self.right = right / math.sqrt(right @ right)
        self.up = np.cross(self.forward, self.right)
        self.ty = math.tan(self.fov_y / 2)
        self.tx = self.ty * self.aspect

    def with_jitter(self, jitter):
        return Camera(self.width, self.height, self.position, self.yaw, self.pitch, self.fov_y, self.aspect, jitter)

    def planar_view_arguments(self):
        return dict(position=tuple(self.position), yaw=self.yaw, pitch=self.pitch, fov_y=self.fov_y, aspect=self.aspect)

    def samples(self):
        """The window position of every pixel's primary ray, row-major [H * W, 2]."""
        x, y = np.meshgrid(np.arange(self.width, dtype=F), np.arange(self.height, dtype=F))
        return np.stack([x.ravel() + 0.5 + self.jitter[0], y.ravel() + 0.5 + self.jitter[1]], 1)

    def rays(self, window):
        window = np.asarray(window, F).reshape(-1, 2)
        x = (2.0 * window[:, 0] / self.width - 1.0) * self.tx
        y = (1.0 - 2.0 * window[:, 1] / self.height) * self.ty
        d = self.forward[None] + self.right[None] * x[:, None] + self.up[None] * y[:, None]
        return np.broadcast_to(self.position, d.shape).copy(), d / np.sqrt((d * d).sum(1, keepdims=True))

    def project(self, X):
        """(window [n, 2], view depth [n]); the window position of a point at or behind the camera's plane is NaN."""
        v = np.asarray(X, F) - self.position
        x, y, z = v @ self.right, v @ self.up, v @ self.forward
        with np.errstate(all="ignore"):
            w = np.stack([(1.0 + x / (z * self.tx)) * self.width / 2, (1.0 - y / (z * self.ty)) * self.height / 2], 1)
        return np.where((z > 0)[:, None], w, np.nan), z


class Frame:
    """One frame: `scene` is the SceneArrays as it stands in that frame (its vertices, its m_World), `camera` the frame's Camera."""

    def __init__(self, scene, camera):
        self.scene, self.camera = scene, camera
        self.ps = R.PathScene(scene)
        self.size = float(max(np.abs(self.ps.P).max(), np.abs(camera.position).max()))

    def cast(self, o, d):
        """hit, triangle, t, u, v, margin of the rays (o, d): TraceRayStandard over an opaque scene, by path_reference's brute force."""
        n = len(o)
        margin = np.full(n, INF)
        took = {b: np.zeros(n, bool) for b in R.BRANCHES + R.SURFACE_BRANCHES}
        with np.errstate(all="ignore"):
            hit, tri, t, u, v = self.ps.trace_standard(o, d, np.zeros(n), R.Rng(np.zeros(n, np.uint32)), np.ones(n, bool), margin, took)
        return hit, tri, t, u, v, margin

    def point(self, tri, u, v):
        P = self.ps.P[tri]
        return P[:, 0] * (1.0 - u - v)[:, None] + P[:, 1] * u[:, None] + P[:, 2] * v[:, None]

    def first_hits(self, window=None):
        """dict per window position (default: every pixel's sample): hit, tri, inst, prim, u, v, t, X, depth, normal (the shading normal,
        turned towards the eye), emission, margin."""
        window = self.camera.samples() if window is None else np.asarray(window, F).reshape(-1, 2)
        o, d = self.camera.rays(window)
        hit, tri, t, u, v, margin = self.cast(o, d)
        X = self.point(tri, u, v)
        with np.errstate(all="ignore"):
            attr = self.ps.surf.attributes(tri, u, v)
            pbr = self.ps.surf.pbr(self.ps.mat_of[tri], attr)
        normal = pbr["normal"]
        facing = (normal * -d).sum(1)
        normal = np.where((facing < 0)[:, None], -normal, normal)
        margin = np.minimum(margin, np.where(hit, np.minimum(np.abs(facing), pbr["margin"]), INF))
        return dict(window=window, o=o, d=d, hit=hit, tri=tri, inst=np.where(hit, self.ps.inst_of[tri], -1), prim=self.ps.prim_of[tri], u=u, v=v,
                    t=t, X=X, depth=(X - self.camera.position) @ self.camera.forward, normal=normal, emission=pbr["emissive"], margin=margin)

    def radiance(self, window, hits=None):
        """G at continuous window positions: the first hit's emission (factor times texture, through the material's sampler), the sky with
        the sun's disk on a miss -- what a path of one bounce returns in a scene without lights and with base colour 0."""
        h = self.first_hits(window) if hits is None else hits
        out = np.where(h["hit"][:, None], h["emission"], 0.0)
        miss = ~h["hit"]
        if miss.any():
            sun = np.asarray(self.scene.sun_direction, F).reshape(1, 3)
            out[miss] = A.rt_sky_radiance(self.ps.t16, self.ps.s16, h["o"][miss], h["d"][miss], sun, F(self.scene.lights[0]["m_Intensity"]), True)
        return out

    def planes(self, hits):
        """The true depth plane (t, view depth, u, v; 1e10 twice on a miss) and normal plane of `hits`, [H, W, 4] float64."""
        H, W = self.camera.height, self.camera.width
        hit = hits["hit"]
        depth = np.where(hit[:, None], np.stack([hits["t"], hits["depth"], hits["u"], hits["v"]], 1), np.array([FAR, FAR, 0.0, 0.0]))
        normal = np.where(hit[:, None], np.concatenate([hits["normal"], np.zeros((len(hit), 1))], 1), 0.0)
        return depth.reshape(H, W, 4), normal.reshape(H, W, 4)


def pair_truth(cur, prev, hits=None):
    """The truth of frame `cur` against its predecessor `prev` at every pixel of `cur` (or at `hits` = cur.first_hits(...)); see the
    module's docstring. Adds to the hits: Xp, wp, prev_depth, motion, depth_difference, visible, visibility_margin, w."""
    h = dict(cur.first_hits() if hits is None else hits)
    assert cur.ps.P.shape == prev.ps.P.shape and np.array_equal(cur.ps.inst_of, prev.ps.inst_of), "the two frames must share their topology"
    hit, tri, u, v, X = h["hit"], h["tri"], h["u"], h["v"], h["X"]
    n = len(hit)
    size = max(cur.size, prev.size)
    # the closed loop of frame k: X projects onto the sample position, and the ray through that position meets X
    w, depth = cur.camera.project(X)
    assert np.abs(w - h["window"])[hit].max() <= LOOP * max(cur.camera.width, cur.camera.height), "window(X) is not p + 0.5 + jitter"
    o, d = cur.camera.rays(w[hit])
    reach = ((X[hit] - o) * d).sum(1)
    assert np.abs(o + d * reach[:, None] - X[hit]).max() <= LOOP * size
    # the previous point and its window position, verified by casting
    Xp = prev.point(tri, u, v)
    wp, prev_depth = prev.camera.project(Xp)
    front = hit & (prev_depth > 0)
    o, d = prev.camera.rays(wp[front])
    dist = np.sqrt(((Xp[front] - o) ** 2).sum(1))
    assert np.abs(o + d * dist[:, None] - Xp[front]).max() <= LOOP * size, "the ray through w' does not meet X'"
    # visibility of X' in the previous frame
    visible, vmargin = np.zeros(n, bool), np.zeros(n)
    if front.any():
        with np.errstate(all="ignore"):
            t, _, _, c = prev.ps.pairs(o, d, np.zeros(len(o)), np.full(len(o), INF))
        other = np.arange(t.shape[1])[None, :] != tri[front][:, None]
        rel = (t - dist[:, None]) / dist[:, None]
        crossed = other & (c > 0)
        occluded = (crossed & (rel < 0)).any(1)
        near = np.where(crossed, np.abs(rel), INF).min(1)
        edge = np.where(other & (rel < 0) & np.isfinite(c), np.abs(c), INF).min(1)
        visible[front], vmargin[front] = ~occluded, np.minimum(near, edge)
    h.update(w=w, Xp=Xp, wp=wp, prev_depth=prev_depth, in_front=front, motion=np.where(front[:, None], wp - w, 0.0),
             depth_difference=np.where(front, prev_depth - depth, 0.0), visible=visible, visibility_margin=vmargin)
    return h


def same_instance_around(inst_map, centre, lo, hi, inst):
    """Every texel of the footprint [floor(centre) + lo, floor(centre) + hi]^2 (clamped to the image) of `inst_map` [H, W] shows `inst`."""
    H, W = inst_map.shape
    with np.errstate(all="ignore"):
        base = np.floor(np.nan_to_num(centre, nan=-1e6)).astype(np.int64)
    ok = np.ones(len(inst), bool)
    for dy in range(lo, hi + 1):
        for dx in range(lo, hi + 1):
            ok &= inst_map[np.clip(base[:, 1] + dy, 0, H - 1), np.clip(base[:, 0] + dx, 0, W - 1)] == inst
    return ok


def safe_pixels(truth, cur_maps, prev_maps, prev_size, margin_bar, visibility_bar=1e-3):
    """Safe: p is hit with margin, X' is visible with margin, w' lies at least 2 px inside the previous image, every texel of the 4 x 4
    Catmull-Rom footprint around w' shows p's instance in every map of `prev_maps` (instance ids of frame k - 1, [H, W]), and every texel
    of the 3 x 3 neighbourhood of p does in every map of `cur_maps`. Disoccluded: p is hit with margin and X' is hidden with margin."""
    W, H = prev_size
    t = truth
    hit = t["hit"] & (t["margin"] >= margin_bar)
    wp = t["wp"]
    with np.errstate(invalid="ignore"):
        inside = t["in_front"] & (wp[:, 0] >= 2) & (wp[:, 0] <= W - 2) & (wp[:, 1] >= 2) & (wp[:, 1] <= H - 2)
    safe = hit & inside & t["visible"] & (t["visibility_margin"] >= visibility_bar)
    for m in prev_maps:
        safe &= same_instance_around(m, wp - 0.5, -1, 2, t["inst"])
    pixel = np.stack([np.arange(len(hit)) % cur_maps[0].shape[1], np.arange(len(hit)) // cur_maps[0].shape[1]], 1).astype(F)
    for m in cur_maps:
        safe &= same_instance_around(m, pixel, -1, 1, t["inst"])
    disoccluded = hit & t["in_front"] & ~t["visible"] & (t["visibility_margin"] >= visibility_bar)
    return safe, disoccluded


def hull_violation(out, colour, history, wp, widen=1e-9, floor=0.0):
    """How far `out` [n, 3] lies outside the per-channel hull of colour [n, 3] and of the history [H, W, >= 3] at the 2 x 2 texels that
    enclose the window position wp [n, 2] (texel q has its centre at q + 0.5), beyond a widening of `widen` relative to
    max(|hull|, floor). 0 where it lies inside."""
    H, W = history.shape[:2]
    base = np.floor(np.nan_to_num(wp, nan=0.0) - 0.5).astype(np.int64)
    lo, hi = colour.copy(), colour.copy()
    for dy in (0, 1):
        for dx in (0, 1):
            t = history[np.clip(base[:, 1] + dy, 0, H - 1), np.clip(base[:, 0] + dx, 0, W - 1), :3]
            lo, hi = np.minimum(lo, t), np.maximum(hi, t)
    slack = widen * np.maximum(np.maximum(np.abs(lo), np.abs(hi)), floor)
    return np.maximum(np.maximum(lo - slack - out, out - hi - slack), 0.0).max(1)
