"""Inputs of the radiance-cache tests, shared by tests/test_rcache_cpu.py and tests/test_rcache_gpu.py: descs,
sample and point records, and the named insert cases. Every case that is compared as a map carries the drop count of the NumPy statement,
asserted to be 0 where the case is made; the overflow case is searched for with the NumPy hash."""
import functools

import numpy as np

import rcache_reference as R
from hobbyrenderer_amd import native, structs as S

CAM = np.array([0.25, -0.5, 1.0], np.float32)
COUNTS = (0, 1, 63, 64, 65, 4096)


def desc(capacity_log2=10, **kw):
    kw.setdefault("max_samples", 60)
    return native.rcache_desc(capacity_log2=capacity_log2, **kw)


def samples(position, normal, radiance, valid=1.0):
    position = np.asarray(position, np.float32).reshape(-1, 3)
    s = np.zeros(len(position), S.RcacheSample)
    s["position"], s["normal"], s["radiance"], s["valid"] = position, normal, radiance, valid
    return s


def points(position, normal):
    position = np.asarray(position, np.float32).reshape(-1, 3)
    p = np.zeros(len(position), S.RcachePoint)
    p["position"], p["normal"] = position, normal
    return p


def _steps(x, n=2):
    """x and its n binary32 neighbours on each side."""
    out, lo, hi = [np.float32(x)], np.float32(x), np.float32(x)
    for _ in range(n):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return out


@functools.lru_cache(maxsize=None)
def key_points():
    """(positions [n, 3], normals [n, 3]) for the camera CAM: both sides of level boundaries (|p - c| = 2^k) and of voxel faces one binary32
    step at a time, negative coordinates, grid coordinates beyond the 17-bit wrap, every normal octant with -0.0 components."""
    pos, nrm = [], []
    for k in (-1, 0, 1, 2, 5):                                   # level boundaries along +x and -y from the camera
        for d in _steps(2.0 ** k):
            pos += [CAM + np.array([d, 0, 0], np.float32), CAM - np.array([0, d, 0], np.float32)]
    d = desc()
    for level in (1, 2, 4):                                      # voxel faces: multiples of the voxel size, both signs
        voxel = R.voxel_of(d, level)
        for m in (-3, -1, 0, 1, 2, 7):
            for x in _steps(np.float32(m) * voxel):
                pos.append(np.array([x, CAM[1] + np.float32(2.0 ** level * 1.2), x], np.float32))
    far = np.float32(0.04 * 70000.0)                             # level 1 next to the camera, grid coordinate above 2^16: the wrap
    pos += [np.array([far, -far, 2 * far], np.float32), np.array([-far, far, -3 * far], np.float32)]
    nrm = [np.array([0.0, 1.0, 0.0], np.float32)] * len(pos)
    for sx in (1.0, -1.0, 0.0, -0.0):                            # octants, with zero and negative-zero components
        for sy in (0.5, -0.5, -0.0):
            for sz in (1.0, -1.0, 0.0):
                pos.append(np.array([1.0, 2.0, 3.0], np.float32))
                nrm.append(np.array([sx, sy, sz], np.float32))
    return np.array(pos, np.float32), np.array(nrm, np.float32)


def _wrap_cameras():
    far = np.float32(0.04 * 70000.0)
    return {len(key_points()[0]) - 36 - 2: np.array([far, -far, 2 * far], np.float32) + np.float32(0.01),
            len(key_points()[0]) - 36 - 1: np.array([-far, far, -3 * far], np.float32) + np.float32(0.01)}


def key_camera(i):
    """The camera of key point i: CAM, or a camera next to the point for the two wrap points."""
    return _wrap_cameras().get(i, CAM)


def scattered(n, keys, seed, spread=3.0):
    """n samples over `keys` distinct surface points near the camera (several samples per point when n > keys), radiance in [0, 4)."""
    rng = np.random.default_rng(seed)
    sites = (rng.random((max(keys, 1), 3), np.float32) - np.float32(0.5)) * np.float32(spread) + CAM
    normals = rng.standard_normal((max(keys, 1), 3)).astype(np.float32)
    pick = rng.integers(0, max(keys, 1), n)
    return samples(sites[pick], normals[pick], rng.random((n, 3), np.float32) * np.float32(4.0))


@functools.lru_cache(maxsize=None)
def insert_cases():
    """{name: (desc, samples, the NumPy statement's table after them, its drop count)}; every one has drop count 0."""
    cases = {}
    for n in COUNTS:
        cases[f"scattered_{n}"] = (desc(10), scattered(n, 40, 100 + n))
    one = samples(np.tile(np.array([[1.0, 2.0, 3.0]], np.float32), (4096, 1)), (0, 0, 1), np.random.default_rng(7).random((4096, 3), np.float32) * np.float32(9.0))
    cases["one_key_4096"] = (desc(10), one)
    cases["700_keys_4096"] = (desc(12), scattered(4096, 700, 9, spread=6.0))
    hostile = scattered(65, 20, 11)
    hostile["radiance"][::5, 0] = np.nan
    hostile["radiance"][1::5, 1] = -3.0
    hostile["radiance"][2::5, 2] = 1e9                          # above the channel clamp at radianceScale 1e3
    hostile["radiance"][3::7, 1] = np.inf
    hostile["position"][4::9, 1] = np.inf                       # skipped, not counted
    hostile["normal"][5::11, 2] = np.nan
    hostile["valid"][6::13] = 0.0
    cases["hostile_65"] = (desc(10), hostile)
    out = {}
    for name, (d, s) in cases.items():
        keys, accum, resolved = native.rcache_table(d)
        drops = R.insert(d, CAM, keys, accum, s)
        assert drops == 0, f"{name}: the map comparison needs a case without overflow"
        out[name] = (d, s, (keys, accum, resolved), drops)
    return out


@functools.lru_cache(maxsize=None)
def overflow_case():
    """(desc, 40 samples with 40 distinct keys of ONE home bucket at capacity 2^10, their keys), found with the NumPy hash."""
    d = desc(10)
    found, keys, target, i = [], [], None, 0
    while len(found) < 40:
        p = CAM + np.array([0.3 + 0.045 * (i % 97), 0.2 + 0.045 * (i // 97 % 89), 0.1 + 0.045 * (i // (97 * 89))], np.float32)
        i += 1
        key, _ = R.key_of(d, p, (0, 1, 0), CAM)
        base = R.bucket_base(key, 10)
        if target is None:
            target = base
        if base == target and key not in keys:
            found.append(p)
            keys.append(key)
    return d, samples(np.array(found), (0, 1, 0), (1.0, 2.0, 3.0)), keys
