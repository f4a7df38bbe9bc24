"""The hash-grid radiance cache on the GPU. The four table kernels equal the NumPy statement of
tests/rcache_reference.py on every case of the CPU suite, as maps (the slot a key lands in depends on the order of the CAS winners) and bit
for bit in what a query returns, with the wave-local combine on and off; the surface query equals the G-buffer planes and hrpt_trace_rays;
a fresh cache changes nothing of hrpt_indirect_lighting's diffuse plane; the two frame calls equal their composition from the public stage
calls and host executors on a second context; a closed emissive box stores and returns exactly its emission; RESET, resize, isolation and
the refusal of a broken table."""
import math

import numpy as np
import pytest

import rcache_cases as RC
import rcache_reference as R
from hobbyrenderer_amd import native, scenes, structs as S
from test_deferred_gpu import _camera, _context, _moved, _scene, same_bytes

pytestmark = pytest.mark.gpu

FOUR = (S.GB_ALBEDO, S.GB_NORMAL, S.GB_GEO_NORMAL, S.GB_DEPTH)
FOUR_MASK = sum(1 << p for p in FOUR)
MISS = np.float32(1e10)
UNTRACED = np.zeros((), S.Ray)
UNTRACED["origin"] = np.uint32(0x7FC00000).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to("cuda:0")


class DeviceTable:
    """A table in caller-owned device memory, driven through the _device stage calls."""

    def __init__(self, ctx, d, table=None):
        import torch
        self.ctx, self.d, self.stream = ctx, d, torch.cuda.current_stream()
        keys, accum, resolved = table if table is not None else native.rcache_table(d)
        self.keys, self.accum, self.resolved, self.drops = _dev(keys), _dev(accum), _dev(resolved), _dev(np.zeros(2, np.uint64))

    def insert(self, s, flags=0):
        ds = _dev(s)
        self.ctx.rcache_insert_device(self.d, RC.CAM, self.keys.data_ptr(), self.accum.data_ptr(), self.drops.data_ptr(), ds.data_ptr() if len(s) else 0, len(s), flags,
                                      self.stream.cuda_stream)
        self.stream.synchronize()

    def resolve(self, flags=0):
        self.ctx.rcache_resolve_device(self.d, self.keys.data_ptr(), self.accum.data_ptr(), self.resolved.data_ptr(), flags, self.stream.cuda_stream)
        self.stream.synchronize()

    def query(self, pts):
        import torch
        dp, out, voxel = _dev(pts), torch.full((len(pts), 4), float("nan"), device="cuda:0"), torch.full((len(pts),), float("nan"), device="cuda:0")
        self.ctx.rcache_query_device(self.d, RC.CAM, self.keys.data_ptr(), self.resolved.data_ptr(), dp.data_ptr(), out.data_ptr(), voxel.data_ptr(), len(pts), self.stream.cuda_stream)
        self.stream.synchronize()
        return out.cpu().numpy(), voxel.cpu().numpy()

    def host(self):
        return (self.keys.cpu().numpy().view(np.uint64), self.accum.cpu().numpy().view(S.RcacheAccum), self.resolved.cpu().numpy().view(S.RcacheEntry))

    def dropped(self):
        return int(self.drops.cpu().numpy().view(np.uint64)[0])


def assert_same_table(d, got, want, what):
    assert R.invariant_faults(d, *got) == [], what
    assert R.as_map(*got) == R.as_map(*want), what


@pytest.fixture(scope="module")
def bare():
    ctx = native.PathTracerContext(0)                # no scene: the table kernels need none
    yield ctx
    ctx.close()


# ---------------------------------------------------------------- 1. the table kernels == the statement
@pytest.mark.parametrize("name", sorted(RC.insert_cases()))
@pytest.mark.parametrize("flags", [0, S.RCACHE_NO_WAVE_COMBINE], ids=["combine", "per-sample"])
def test_insert_resolve_and_query_equal_the_statement(bare, name, flags):
    d, s, after_insert, drops = RC.insert_cases()[name]
    assert drops == 0                                # the condition of the map comparison
    t = DeviceTable(bare, d)
    t.insert(s, flags)
    assert t.dropped() == 0
    assert_same_table(d, t.host(), after_insert, "after the insert")
    ref = tuple(a.copy() for a in after_insert)
    R.resolve(d, *ref)
    t.resolve()
    assert_same_table(d, t.host(), ref, "after the resolve")
    # a second frame on top: half of the samples again, the other entries age
    half = s[::2]
    t.insert(half, flags); t.resolve()
    assert R.insert(d, RC.CAM, ref[0], ref[1], half) == 0
    R.resolve(d, *ref)
    assert_same_table(d, t.host(), ref, "after the second frame")
    pts = RC.points(np.concatenate([s["position"], s["position"][:8] + np.float32(7.0)]), np.concatenate([s["normal"], s["normal"][:8]]))
    got, want = t.query(pts), R.query(d, RC.CAM, ref[0], ref[2], pts)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))


def test_keys_at_boundaries_wraps_and_octants_equal_the_statement(bare):
    """The key points of the CPU suite (level boundaries and voxel faces one binary32 step at a time, negative coordinates, the 17-bit wrap,
    every octant with -0.0) through the insert and query kernels: the same keys and, bit for bit, the same voxel sizes."""
    pos, nrm = RC.key_points()
    d = RC.desc(12)
    t = DeviceTable(bare, d)
    plain = [i for i in range(len(pos)) if RC.key_camera(i) is RC.CAM]
    assert len(plain) == len(pos) - 2
    s = RC.samples(pos[plain], nrm[plain], (1.0, 0.5, 0.25))
    for flags in (0, S.RCACHE_NO_WAVE_COMBINE):
        t.insert(s, flags)
    keys, accum, resolved = native.rcache_table(d)
    assert R.insert(d, RC.CAM, keys, accum, np.concatenate([s, s])) == 0
    assert t.dropped() == 0
    assert_same_table(d, t.host(), (keys, accum, resolved), "the key points")
    t.resolve()
    R.resolve(d, keys, accum, resolved)
    pts = RC.points(pos[plain], nrm[plain])
    got, want = t.query(pts), R.query(d, RC.CAM, keys, resolved, pts)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])) and got[0][:, 3].all()
    for i in set(range(len(pos))) - set(plain):                      # the wrap points have a camera of their own
        w = DeviceTable(bare, d)
        cam, w_s = RC.key_camera(i), RC.samples(pos[i], nrm[i], (1, 1, 1))
        bare.rcache_insert_device(d, cam, w.keys.data_ptr(), w.accum.data_ptr(), w.drops.data_ptr(), _dev(w_s).data_ptr(), 1, 0, w.stream.cuda_stream)
        w.stream.synchronize()
        k = w.host()[0]
        assert [int(x) for x in k[k != 0]] == [R.key_of(d, pos[i], nrm[i], cam)[0]]


@pytest.mark.parametrize("flags", [0, S.RCACHE_NO_WAVE_COMBINE], ids=["combine", "per-sample"])
def test_overflow_keeps_32_of_40_keys_and_counts_8_drops(bare, flags):
    d, s, all_keys = RC.overflow_case()
    t = DeviceTable(bare, d)
    t.insert(s, flags)
    keys, accum, _ = t.host()
    stored = [int(k) for k in keys[keys != 0]]
    assert len(stored) == 32 == len(set(stored)) and set(stored) <= set(all_keys)
    assert t.dropped() == 8 and int(accum["count"].sum()) + 8 == len(s)
    assert R.invariant_faults(d, *t.host()) == []


def test_ageing_eviction_compaction_in_order_and_reset(bare):
    d0, s, all_keys = RC.overflow_case()
    d = RC.desc(10, stale_frames_max=0)
    keys, accum, resolved = native.rcache_table(d)
    keys, accum, _ = native.rcache_insert_host(d, RC.CAM, keys, accum, s[:32], nthreads=1)      # a full bucket in a known order
    table = native.rcache_resolve_host(d, keys, accum, resolved)
    base = R.bucket_base(all_keys[0], 10)
    t = DeviceTable(bare, d, table)
    feed = np.delete(s[:32], [0, 5, 31])
    t.insert(feed); t.resolve()
    ref = tuple(a.copy() for a in table)
    assert R.insert(d, RC.CAM, ref[0], ref[1], feed) == 0
    R.resolve(d, *ref)
    got = t.host()
    assert [int(k) for k in got[0][base:base + 32]] == [k for i, k in enumerate(all_keys[:32]) if i not in (0, 5, 31)] + [0, 0, 0]
    assert np.array_equal(got[0], ref[0]) and got[2].tobytes() == ref[2].tobytes() and not got[1].view(np.uint8).any()
    # re-insert after the eviction: no duplicate key
    t.insert(s[:32]); t.resolve()
    got = t.host()
    assert sorted(int(k) for k in got[0][got[0] != 0]) == sorted(all_keys[:32]) and R.invariant_faults(d, *got) == []
    # ageing to eviction at staleFramesMax + 1
    d2 = RC.desc(10, stale_frames_max=2)
    t = DeviceTable(bare, d2)
    t.insert(s[:20]); t.resolve()
    for age in (1, 2):
        t.resolve()
        k, _, r = t.host()
        assert (k != 0).sum() == 20 and set(r["meta"][k != 0] >> 16) == {age}
    t.resolve()
    assert not any(a.view(np.uint8).any() for a in t.host())
    t.insert(s[:20]); t.resolve(S.RCACHE_RESET)
    assert not any(a.view(np.uint8).any() for a in t.host())


# ---------------------------------------------------------------- 2. where rays land
def _primary(cb, W, H):
    import gbuffer_reference as G
    o, d, seed = G.primary_rays(cb, W, H)
    rays = np.zeros(H * W, S.Ray)
    rays["origin"], rays["direction"], rays["tmax"], rays["rng"] = o, d.reshape(-1, 3), 1e10, seed.reshape(-1)
    return rays


def _surfaces(ctx, rays):
    import torch
    dr, out = _dev(rays), torch.full((len(rays) * 12,), float("nan"), device="cuda:0")
    stream = torch.cuda.current_stream()
    ctx.rcache_surfaces_device(dr.data_ptr(), out.data_ptr(), len(rays), stream.cuda_stream)
    stream.synchronize()
    return out.cpu().numpy().view(S.RcacheSurface)


@pytest.mark.parametrize("name,structure", [("cube", None), ("cornell", None), ("soup", None), ("cornell", S.ACCEL_TWO_LEVEL), ("soup", S.ACCEL_TWO_LEVEL)],
                         ids=["cube", "cornell", "soup", "cornell-two-level", "soup-two-level"])
def test_surfaces_equal_the_gbuffer_planes_and_trace_rays(luts, name, structure):
    W, H = 40, 24
    sc = _scene(luts, name)
    view, pos = _camera(name, W, H)
    cb = scenes.fill_constants(view, pos, sc, 3, 1)
    cb["m_Jitter"] = (0.25, -0.125)
    ctx = _context(sc, structure, W, H)
    try:
        ctx.render_gbuffer(cb, planes=1 << S.GB_DEPTH | 1 << S.GB_GEO_NORMAL)
        depth, geo = ctx.read_gbuffer(S.GB_DEPTH).reshape(-1, 4), ctx.read_gbuffer(S.GB_GEO_NORMAL).reshape(-1, 4)
        rays = _primary(cb, W, H)
        rays[5]["origin"][1] = np.nan                                 # a ray that is not finite: a miss that keeps its rng
        surf = _surfaces(ctx, rays)
        hits = ctx.trace_rays(rays, thread_per_ray=True)
        assert hits.tobytes() == ctx.trace_rays(rays).tobytes()
        hit = hits["hit"] == 1
        assert hit.any() and (name != "cube" or (~hit).any())
        assert np.array_equal(surf["hit"], hits["hit"]) and np.array_equal(surf["rng"], hits["rng"]) and np.array_equal(bits(surf["t"]), bits(hits["t"]))
        assert not surf["pad"].any() and not surf["position"][~hit].any() and not surf["normal"][~hit].any() and surf["hit"][5] == 0
        ok = hit.copy(); ok[5] = False
        assert np.array_equal(bits(surf["t"][ok]), bits(depth[ok, 0])) and (depth[~hit & (np.arange(W * H) != 5), 0] == MISS).all()
        o, d, t = rays["origin"], rays["direction"], surf["t"]
        X = np.stack([o[:, k] + d[:, k] * t for k in range(3)], -1).astype(np.float32)
        assert np.array_equal(bits(surf["position"][hit]), bits(X[hit]))
        Ng = geo[:, :3]
        facing = (Ng[:, 0] * d[:, 0] + Ng[:, 1] * d[:, 1]) + Ng[:, 2] * d[:, 2]
        want = np.where((facing > 0)[:, None], -Ng, Ng)
        assert np.array_equal(bits(surf["normal"][ok]), bits(want[ok]))
    finally:
        ctx.close()


# ---------------------------------------------------------------- 3. an empty cache changes nothing
@pytest.mark.parametrize("name,size", [("cornell", (40, 24)), ("cube", (64, 48))], ids=["cornell-40x24", "cube-64x48"])
def test_an_empty_cache_changes_nothing(luts, name, size):
    W, H = size
    sc = _scene(luts, name)
    view, pos = _camera(name, W, H)
    cb = scenes.fill_constants(view, pos, sc, 3, 3)
    ctx = _context(sc, None, W, H)
    cache = native.RadianceCache(ctx, RC.desc(12))
    try:
        ctx.render_gbuffer(cb, planes=FOUR_MASK)
        ctx.indirect_lighting(cb, S.IndirectParams(S.INDIRECT_DIFFUSE | S.INDIRECT_SPECULAR, 77))
        want, spec = ctx.read_indirect(0), ctx.read_indirect(1)
        assert (want[..., :3] > 0).any()
        cache.indirect(cb, S.RcacheParams(0, 77))
        same_bytes(ctx.read_indirect(0), want, "the diffuse plane through an empty cache")
        same_bytes(ctx.read_indirect(1), spec, "the specular plane is left as it is")
        assert not ctx.read_rcache_served().any()
        cache.indirect(cb, S.RcacheParams(S.RCACHE_NO_FALLBACK, 77))
        assert not ctx.read_indirect(0).any() and not ctx.read_rcache_served().any()
    finally:
        cache.close(); ctx.close()


# ---------------------------------------------------------------- 4. the frame calls == their composition from the public calls
def _update_records(d, planes, cb, W, H, frame):
    """The records of one hrpt_rcache_update: the picked pixels' diffuse records of the indirect stage, untraced below the roughness threshold."""
    full = native.indirect_rays_host(*planes, cb, S.IndirectParams(S.INDIRECT_DIFFUSE, frame))[0]
    rough = planes[1][..., 3]
    picks = R.block_pixels(W, H, int(d["sparseBlock"]), frame)
    rays = np.full(len(picks), UNTRACED, S.Ray)
    for i, p in enumerate(picks):
        if p is not None and not rough[p[1], p[0]] < np.float32(d["roughnessThreshold"]):
            rays[i] = full[p[1], p[0]]
    return rays


def _compose_update(d, other, table, planes, cb, W, H, frame, cam):
    rays = _update_records(d, planes, cb, W, H, frame)
    surf = _surfaces(other, rays)
    rad = other.trace_radiance(rays, cb, secondary=True)
    s = RC.samples(surf["position"], surf["normal"], rad[:, :3], ((surf["hit"] != 0) & (rad[:, 3] == 1)).astype(np.float32))
    keys, accum, drops = native.rcache_insert_host(d, cam, table[0], table[1], s)
    assert drops == 0
    return native.rcache_resolve_host(d, keys, accum, table[2]), int((s["valid"] == 1).sum())


def _compose_indirect(d, other, table, planes, cb, W, H, seed, cam, fallback=True):
    p = S.IndirectParams(S.INDIRECT_DIFFUSE, seed)
    rays = native.indirect_rays_host(*planes, cb, p).reshape(-1)
    surf = _surfaces(other, rays)
    cached, voxel = native.rcache_query_host(d, cam, table[0], table[2], RC.points(surf["position"], surf["normal"]))
    served = (surf["hit"] != 0) & (cached[:, 3] == 1) & (surf["t"] >= voxel)
    rays = rays.copy()
    rays[served] = UNTRACED
    rad = other.trace_radiance(rays, cb, secondary=True) if fallback else np.zeros((len(rays), 4), np.float32)
    dif = native.indirect_resolve_host(*planes, cb, rad.reshape(1, H, W, 4), p)[0].reshape(-1, 4)
    plane = np.where(served[:, None], np.concatenate([cached[:, :3], np.ones((len(rays), 1), np.float32)], 1), np.float32(0)).astype(np.float32)
    dif[served] = plane[served]
    return dif.reshape(H, W, 4), plane.reshape(H, W, 4), served


@pytest.mark.parametrize("name,size,structure,move", [("cornell", (40, 24), None, False), ("cornell", (64, 48), None, False), ("soup", (40, 24), S.ACCEL_TWO_LEVEL, True)],
                         ids=["cornell-40x24", "cornell-64x48", "soup-two-level-moved"])
def test_frame_calls_equal_the_composition_of_the_public_calls(luts, name, size, structure, move):
    W, H = size
    sc = _scene(luts, name)
    view, pos = _camera(name, W, H)
    cb = scenes.fill_constants(view, pos, sc, 3, 3)
    cam = np.asarray(cb["m_CameraPos"], np.float32).reshape(-1)[:3]
    d = RC.desc(12, scene_scale=8.0)
    ctx, other = _context(sc, structure, W, H), _context(sc, structure)
    cache = native.RadianceCache(ctx, d)
    try:
        if move:                                                              # hrpt_update_instances before the frames
            sc = _moved(sc, len(sc.instances) - 1)
            for c in (ctx, other):
                c.update_instances(sc.instances[-1:], len(sc.instances) - 1)
        ctx.render_gbuffer(cb, planes=FOUR_MASK)
        planes = [ctx.read_gbuffer(p) for p in FOUR]
        table, fed = native.rcache_table(d), 0
        for frame in range(3):
            cache.update(cb, frame, S.RCACHE_NO_WAVE_COMBINE if frame == 1 else 0)
            table, n = _compose_update(d, other, table, planes, cb, W, H, frame, cam)
            fed += n
            got = cache.read()
            assert got[3] == 0
            assert_same_table(d, got[:3], table, f"{name}: the table after update {frame}")
        assert fed > 0 and (table[0] != 0).any()
        for flags in (0, S.RCACHE_NO_FALLBACK):
            cache.indirect(cb, S.RcacheParams(flags, 77))
            dif, plane, served = _compose_indirect(d, other, table, planes, cb, W, H, 77, cam, fallback=not flags)
            same_bytes(ctx.read_indirect(0), dif, f"{name}: the diffuse plane, flags {flags}")
            same_bytes(ctx.read_rcache_served(), plane, f"{name}: the served plane, flags {flags}")
        print(f"{name} {W}x{H}: {int(served.sum())} of {W * H} pixels served after 3 updates")
        assert served.any()
    finally:
        cache.close(); ctx.close(); other.close()


# ---------------------------------------------------------------- 5. a closed emissive box stores and returns its emission
def test_closed_emissive_box_stores_and_returns_its_emission(luts):
    LE = (2.0, 1.5, 0.5)                              # LE * radianceScale (1e3) are integers: every quantised sample is exact
    b = scenes.SceneBuilder()
    quad = b.add_mesh(*scenes.generate_floor_quad())
    wall = b.add_material(m_BaseColor=(0, 0, 0, 1), m_EmissiveFactor=LE + (1,))
    for rot, at, scale in (("+y", (0, 0, -1.5), (3, 1, 6)), ("-y", (0, 2, -1.5), (3, 1, 6)), ("+x", (-1, 1, -1.5), (3, 1, 6)), ("-x", (1, 1, -1.5), (3, 1, 6)),
                           ("-z", (0, 1, 1), (3, 1, 3)), ("+z", (0, 1, -4), (3, 1, 3))):
        b.add_instance(quad, wall, scenes._mat(scale, scenes._ROT_TO[rot], at))
    sc = b.finalize(luts)
    W, H = 64, 48
    view, pos = scenes.planar_view(W, H, position=(0.1, 0.9, -3.0), yaw=0.3, pitch=0.1, fov_y=math.radians(70.0))
    cb = scenes.fill_constants(view, pos, sc, 0, 2)   # m_MaxBounces = 2: the traced segment is the path's last (test_indirect_gpu.py)
    # voxels of 2^level / 4 with level 1 or 2 in a 2 x 2 x 5 box: a few dozen voxels, so one sparse update fills many of those the pixels' rays
    # land in (served), while rays that end within one voxel of their origin, in the corners, are not served
    d = RC.desc(12, scene_scale=4.0)
    ctx = _context(sc, None, W, H)
    cache = native.RadianceCache(ctx, d)
    try:
        ctx.render_gbuffer(cb, planes=FOUR_MASK)
        assert (ctx.read_gbuffer(S.GB_DEPTH)[..., 0] != MISS).all()
        cache.update(cb, 0)
        keys, accum, resolved, drops = cache.read()
        stored = resolved[keys != 0]
        assert drops == 0 and len(stored) > 0 and not accum.view(np.uint8).any()
        for ch, le in zip("rgb", LE):
            assert (stored[ch] == np.float32(le)).all()
        assert ((stored["meta"] & 0xFFFF) > 0).all()
        rays = native.indirect_rays_host(*[ctx.read_gbuffer(p) for p in FOUR], cb, S.IndirectParams(S.INDIRECT_DIFFUSE, 77))[0]
        traced = np.isfinite(rays["origin"]).all(-1)
        want = np.where(traced[..., None], np.float32(LE + (1.0,)), np.float32(0)).astype(np.float32)
        cache.indirect(cb, S.RcacheParams(0, 77))
        same_bytes(ctx.read_indirect(0), want, "the diffuse plane")
        served = ctx.read_rcache_served()[..., 3] == 1
        print(f"furnace: {int(served.sum())} served, {int((traced & ~served).sum())} traced and not served, {len(stored)} entries")
        assert served.any() and (traced & ~served).any() and not (served & ~traced).any()
        same_bytes(ctx.read_rcache_served()[served], want[served], "the served plane")
    finally:
        cache.close(); ctx.close()


# ---------------------------------------------------------------- 6. the one statistical case
# Voxel bias makes the difference underivable, and the stage is deterministic for fixed seeds: the figure below was measured against the
# existing stage (never against the cache itself) and the test asserts it times 1.5.
MEASURED_REL_DIFF = 0.03133        # cache mean 0.349972 against 0.339339 traced; served fraction 0.7855
MEASURED_ON = "2026-10-21, one MI355X"


def test_cornell_mean_against_the_traced_diffuse_lobe(luts):
    W, H = 64, 48
    sc = _scene(luts, "cornell")                      # three lights
    view, pos = _camera("cornell", W, H)
    cb = scenes.fill_constants(view, pos, sc, 3, 3)
    ctx = _context(sc, None, W, H)
    cache = native.RadianceCache(ctx, RC.desc(12, scene_scale=8.0))
    try:
        ctx.render_gbuffer(cb, planes=FOUR_MASK)
        for frame in range(32):
            cache.update(cb, frame)
        cache.indirect(cb, S.RcacheParams(0, 1000))
        got = float(ctx.read_indirect(0)[..., :3].astype(np.float64).mean())
        served = float((ctx.read_rcache_served()[..., 3] == 1).mean())
        acc = np.zeros((H, W, 3), np.float64)
        for seed in range(256):
            ctx.indirect_lighting(cb, S.IndirectParams(S.INDIRECT_DIFFUSE, seed))
            acc += ctx.read_indirect(0)[..., :3]
        want = float((acc / 256).mean())
        rel = abs(got - want) / want
        print(f"cornell 64x48 after 32 updates: cache mean {got:.6f}, traced mean over 256 seeds {want:.6f}, relative difference {rel:.5f}, served {served:.4f}, "
              f"drops {cache.read()[3]}")
        assert rel <= MEASURED_REL_DIFF * 1.5
    finally:
        cache.close(); ctx.close()


# ---------------------------------------------------------------- 7. reset, resize, isolation, a broken table, destruction
def test_reset_resize_isolation_write_and_destroy(luts):
    lib = native.lib
    W, H = 40, 24
    sc = _scene(luts, "cornell")
    view, pos = _camera("cornell", W, H)
    cb = scenes.fill_constants(view, pos, sc, 3, 3)
    d = RC.desc(10, scene_scale=8.0)
    ctx = _context(sc, None, W, H)
    cache = native.RadianceCache(ctx, d)
    err = lambda: lib.hrpt_last_error(ctx._h).decode()       # noqa: E731
    try:
        assert lib.hrpt_rcache_update(cache._h, cb.ctypes.data, 0, 0) == -1 and "HRPT_GB_ALBEDO" in err()
        ctx.render(cb, accum_count=2)
        ctx.render_gbuffer(cb, planes=FOUR_MASK)
        before = [ctx.read_accumulation(), ctx.read_output()] + [ctx.read_gbuffer(p) for p in FOUR]
        stats = ctx.stats()
        cache.update(cb, 0); cache.update(cb, 1)
        cache.indirect(cb, S.RcacheParams(0, 5))
        after = [ctx.read_accumulation(), ctx.read_output()] + [ctx.read_gbuffer(p) for p in FOUR]
        for k, (a, b) in enumerate(zip(before, after)):
            same_bytes(b, a, f"image {k} after the cache's calls")
        for field, _ in S.Stats._fields_:
            assert getattr(stats, field) == getattr(ctx.stats(), field), field
        table = cache.read()
        assert (table[0] != 0).any()
        # errors leave the table as it was
        assert lib.hrpt_rcache_update(cache._h, cb.ctypes.data, 2, 8) == -1 and "unknown flags" in err()
        deep = cb.copy(); deep["m_MaxBounces"] = 65
        assert lib.hrpt_rcache_update(cache._h, np.ascontiguousarray(deep).ctypes.data, 2, 0) == -1 and "m_MaxBounces" in err()
        bad = S.RcacheParams(4, 0)
        assert lib.hrpt_rcache_indirect(cache._h, cb.ctypes.data, bad) == -1 and "unknown flag bits" in err()
        assert R.as_map(*cache.read()[:3]) == R.as_map(*table[:3])
        # a table that breaks the invariant is refused; a sound one is installed
        holed = table[0].copy()
        first = np.flatnonzero(holed)[0]
        bucket = first - first % 32
        if holed[bucket + 1] == 0:
            holed[bucket + 1], holed[bucket] = holed[bucket], 0
        else:
            holed[bucket] = 0
        with pytest.raises(native.HrptError, match="hrpt_rcache_write"):
            cache.write(holed, table[1], table[2])
        moved = table[0].copy()
        moved[(bucket + 32) % 1024 + 31] = table[0][first]
        with pytest.raises(native.HrptError, match="hrpt_rcache_write"):
            cache.write(moved, table[1], table[2])
        assert R.as_map(*cache.read()[:3]) == R.as_map(*table[:3])
        cache.write(*table[:3])
        # hrpt_resize drops the planes, not the table
        ctx.resize(33, 9)
        assert lib.hrpt_read_rcache_served(ctx._h, None, 0) == -1 and "hrpt_rcache_indirect writes it" in err()
        assert R.as_map(*cache.read()[:3]) == R.as_map(*table[:3])
        # RESET and clear
        ctx.render_gbuffer(scenes.fill_constants(*_camera("cornell", 33, 9), sc, 3, 3), planes=FOUR_MASK)
        cb2 = scenes.fill_constants(*_camera("cornell", 33, 9), sc, 3, 3)
        cache.update(cb2, 9, S.RCACHE_RESET)
        fresh = native.RadianceCache(ctx, d)
        fresh.update(cb2, 9)
        assert R.as_map(*cache.read()[:3]) == R.as_map(*fresh.read()[:3]) != {}
        fresh.close()
        cache.clear()
        assert not any(a.view(np.uint8).any() for a in cache.read()[:3])
    finally:
        cache.close(); ctx.close()               # the cache goes before its context
