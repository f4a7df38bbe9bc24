"""The radiance cache's host executors (hrpt_rcache_insert_host / _resolve_host / _query_host, csrc/pt_rcache.h) against the NumPy statement
of tests/rcache_reference.py, which shares nothing with the C source. No GPU. Tables are compared as maps -- the set of keys, and the
accumulation and resolved record of every key bit for bit -- plus the invariants; query results are compared bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rcache_cases as RC
import rcache_reference as R
from hobbyrenderer_amd import native, structs as S

lib = native.lib
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hobbyrenderer_amd", "csrc")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_table(d, got, want):
    assert R.invariant_faults(d, *got) == []
    assert R.as_map(*got) == R.as_map(*want)


# ---------------------------------------------------------------- keys
def test_keys_and_voxel_sizes_at_boundaries_wraps_and_octants():
    pos, nrm = RC.key_points()
    d = RC.desc(10)
    levels = set()
    for i, (p, n) in enumerate(zip(pos, nrm)):
        cam = RC.key_camera(i)
        key, voxel = R.key_of(d, p, n, cam)
        levels.add(key >> 51 & 0x3FF)
        keys, accum, _ = native.rcache_table(d)
        keys, accum, drops = native.rcache_insert_host(d, cam, keys, accum, RC.samples(p, n, (1, 1, 1)))
        assert drops == 0 and [int(k) for k in keys[keys != 0]] == [key], (i, p, n)
        assert np.flatnonzero(keys)[0] == R.bucket_base(key, 10)
        _, v = native.rcache_query_host(d, cam, keys, np.zeros(1024, S.RcacheEntry), RC.points(p, n))
        assert bits(v)[0] == bits(np.float32(voxel)), (i, p)
    assert levels == {1, 2, 4, 5}                                # both sides of the boundaries at |p - c| = 4 and 32
    # the wrap points hold grid coordinates past 17 bits, the octant points all eight octants
    wrapped = R.key_of(d, pos[140], nrm[140], RC.key_camera(140))[0]
    assert np.floor(pos[140][2] / np.float32(0.04)) > 2 ** 17 > (wrapped >> 34 & 0x1FFFF)
    assert {R.key_of(d, p, n, RC.CAM)[0] >> 61 for p, n in zip(pos[-36:], nrm[-36:])} == set(range(8))
    assert R.key_of(d, pos[-1], np.float32([-0.0, -0.0, -0.0]), RC.CAM)[0] >> 61 == 7          # -0.0 >= 0


def test_grid_arithmetic_of_a_1920_x_1080_frame():
    """Block count and the picked pixels of block size 5 at full size: one pick per block, inside its block, the last row ragged."""
    picks = R.block_pixels(1920, 1080, 5, 3)
    assert len(picks) == 384 * 216 and all(p is not None for p in picks)
    for i in (0, 383, 384, len(picks) - 1):
        assert (picks[i][0] // 5, picks[i][1] // 5) == (i % 384, i // 384)
    ragged = R.block_pixels(64, 48, 5, 1)
    assert len(ragged) == 13 * 10 and any(p is None for p in ragged) and all(p is None or (p[0] < 64 and p[1] < 48) for p in ragged)


# ---------------------------------------------------------------- insert
@pytest.mark.parametrize("name", sorted(RC.insert_cases()))
@pytest.mark.parametrize("nthreads", [1, 3, 16])
def test_insert_equals_the_statement_as_a_map(name, nthreads):
    d, s, want, drops = RC.insert_cases()[name]
    assert drops == 0                                            # the condition of the map comparison
    keys, accum, resolved = native.rcache_table(d)
    keys, accum, got_drops = native.rcache_insert_host(d, RC.CAM, keys, accum, s, nthreads=nthreads)
    assert got_drops == 0
    assert_same_table(d, (keys, accum, resolved), want)


def test_one_key_sums_and_the_channel_rules():
    d, s, (keys, accum, _), _ = RC.insert_cases()["one_key_4096"]
    assert (keys != 0).sum() == 1 and accum[keys != 0]["count"][0] == 4096
    d, s, (keys, accum, _), _ = RC.insert_cases()["hostile_65"]
    used = (s["valid"] == 1) & np.isfinite(s["position"]).all(1) & np.isfinite(s["normal"]).all(1)
    assert accum["count"].sum() == used.sum() < 65
    k2, a2, _ = native.rcache_insert_host(d, RC.CAM, *native.rcache_table(d)[:2], RC.samples((1, 2, 3), (0, 0, 1), (np.nan, -5.0, 1e9)))
    a = a2[k2 != 0][0]
    assert (int(a["r"]), int(a["g"]), int(a["b"]), int(a["count"])) == (0, 0, 4294967040, 1)


def test_overflow_keeps_32_of_40_keys_and_counts_8_drops():
    d, s, all_keys = RC.overflow_case()
    assert len(set(all_keys)) == 40 and len({R.bucket_base(k, 10) for k in all_keys}) == 1
    for nthreads in (1, 16):
        keys, accum, drops = native.rcache_insert_host(d, RC.CAM, *native.rcache_table(d)[:2], s, nthreads=nthreads)
        stored = [int(k) for k in keys[keys != 0]]
        assert len(stored) == 32 == len(set(stored)) and set(stored) <= set(all_keys)
        assert drops == 8 and int(accum["count"].sum()) + drops == len(s)
    keys, accum, _ = native.rcache_table(d)
    assert R.insert(d, RC.CAM, keys, accum, s) == 8


# ---------------------------------------------------------------- resolve
def _both(d, table, s=None):
    """One frame on both sides from one table: (host table, statement table)."""
    keys, accum, resolved = (a.copy() for a in table)
    hk, ha = keys, accum
    if s is not None:
        hk, ha, drops = native.rcache_insert_host(d, RC.CAM, keys, accum, s, nthreads=3)
        assert drops == 0 and R.insert(d, RC.CAM, keys, accum, s) == 0
    host = native.rcache_resolve_host(d, hk, ha, resolved, nthreads=3)
    R.resolve(d, keys, accum, resolved)
    return host, (keys, accum, resolved)


def test_first_fill_running_mean_and_the_window():
    d = RC.desc(10, max_samples=5)
    host = ref = native.rcache_table(d)
    for frame in range(4):
        s = RC.scattered(200, 30, 50)                                # the same 30 surface points every frame, new radiance
        s["radiance"] = np.random.default_rng(60 + frame).random((200, 3), np.float32) * np.float32(4.0)
        host, ref_next = _both(d, host, s)
        ref = ref_next
        assert_same_table(d, host, ref)
        assert (host[1].view(np.uint8) == 0).all()                   # the accumulation is zeroed
    samples = host[2]["meta"][host[0] != 0] & 0xFFFF
    assert samples.max() == 5 and (host[2]["meta"][host[0] != 0] >> 16).max() == 0
    # the first fill of one key is the plain mean
    d1 = RC.desc(10)
    (k, a, r), _ = _both(d1, native.rcache_table(d1), RC.samples([(1, 2, 3)] * 2, (0, 0, 1), [(1.0, 2.0, 4.0), (2.0, 2.0, 0.0)]))
    e = r[k != 0][0]
    assert (e["r"], e["g"], e["b"], e["meta"]) == (1.5, 2.0, 2.0, 2)


def test_ageing_evicts_at_stale_frames_max_plus_one_and_reinsert_makes_no_duplicate():
    d = RC.desc(10, stale_frames_max=2)
    s = RC.scattered(64, 10, 3)
    table, ref = _both(d, native.rcache_table(d), s)
    n = (table[0] != 0).sum()
    for age in (1, 2):
        table, ref = _both(d, table)
        assert_same_table(d, table, ref)
        assert (table[0] != 0).sum() == n and set(table[2]["meta"][table[0] != 0] >> 16) == {age}
    table, ref = _both(d, table)
    assert (table[0] == 0).all() and R.invariant_faults(d, *table) == [] and R.as_map(*ref) == {}
    table, ref = _both(d, table, s)
    assert_same_table(d, table, ref)
    assert (table[0] != 0).sum() == n and len(set(table[0][table[0] != 0])) == n


def test_compaction_keeps_the_order_of_the_survivors():
    d, s, all_keys = RC.overflow_case()
    d = RC.desc(10, stale_frames_max=0)
    keys, accum, resolved = native.rcache_table(d)
    keys, accum, _ = native.rcache_insert_host(d, RC.CAM, keys, accum, s[:32], nthreads=1)
    keys, accum, resolved = native.rcache_resolve_host(d, keys, accum, resolved)
    base = R.bucket_base(all_keys[0], 10)
    before = [int(k) for k in keys[base:base + 32]]
    assert before == all_keys[:32]                                   # one thread: arrival order
    feed = np.delete(s[:32], [0, 5, 31])                             # slots 0, 5 and 31 get no sample: evicted at stale 1 > 0
    table = (keys, accum, resolved)
    host, ref = _both(d, table, feed)
    assert [int(k) for k in host[0][base:base + 32]] == [k for i, k in enumerate(before) if i not in (0, 5, 31)] + [0, 0, 0]
    assert_same_table(d, host, ref)
    assert np.array_equal(host[0], ref[0]) and host[2].tobytes() == ref[2].tobytes()     # same order on both sides: equal as arrays too


def test_reset_empties_the_table():
    d, s, want, _ = RC.insert_cases()["scattered_4096"]
    keys, accum, resolved = native.rcache_resolve_host(d, *want, flags=S.RCACHE_RESET)
    assert not keys.any() and not accum.view(np.uint8).any() and not resolved.view(np.uint8).any()


# ---------------------------------------------------------------- query
def test_query_present_absent_unresolved_and_the_walk_stops_at_an_empty_slot():
    d, s, all_keys = RC.overflow_case()
    keys, accum, resolved = native.rcache_table(d)
    keys, accum, _ = native.rcache_insert_host(d, RC.CAM, keys, accum, s[:6], nthreads=1)
    pts = RC.points(s["position"][:8], s["normal"][:8])
    for k, r in ((keys, resolved), native.rcache_resolve_host(d, keys, accum, resolved)[::2]):
        got, want = native.rcache_query_host(d, RC.CAM, k, r, pts, nthreads=3), R.query(d, RC.CAM, k, r, pts)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    assert not native.rcache_query_host(d, RC.CAM, keys, resolved, pts)[0].any()                    # present with samples == 0
    keys, accum, resolved = native.rcache_resolve_host(d, keys, accum, resolved)
    out, voxel = native.rcache_query_host(d, RC.CAM, keys, resolved, pts)
    assert (out[:6] == np.float32([1, 2, 3, 1])).all() and not out[6:].any() and (voxel > 0).all()   # present / absent
    base = R.bucket_base(all_keys[0], 10)
    holed = keys.copy()
    holed[base + 2] = 0                                                                             # breaks the invariant on purpose: the walk ends there
    out, _ = native.rcache_query_host(d, RC.CAM, holed, resolved, pts)
    assert out[:2, 3].all() and not out[2:].any()
    bad = RC.points([(np.nan, 0, 0), (1, 2, 3)], [(0, 0, 1), (np.inf, 0, 0)])
    out, voxel = native.rcache_query_host(d, RC.CAM, keys, resolved, bad)
    assert not out.any() and not voxel.any()


@pytest.mark.parametrize("nthreads", [1, 3, 16])
def test_thread_count_invariance(nthreads):
    d, s, want, _ = RC.insert_cases()["700_keys_4096"]
    keys, accum, resolved = native.rcache_table(d)
    keys, accum, _ = native.rcache_insert_host(d, RC.CAM, keys, accum, s, nthreads=nthreads)
    host = native.rcache_resolve_host(d, keys, accum, resolved, nthreads=nthreads)
    ref = tuple(a.copy() for a in want)
    R.resolve(d, *ref)
    assert_same_table(d, host, ref)
    pts = RC.points(s["position"][::7], s["normal"][::7])
    got, want_q = native.rcache_query_host(d, RC.CAM, host[0], host[2], pts, nthreads=nthreads), R.query(d, RC.CAM, ref[0], ref[2], pts)
    assert np.array_equal(bits(got[0]), bits(want_q[0])) and np.array_equal(bits(got[1]), bits(want_q[1])) and got[0][:, 3].all()


# ---------------------------------------------------------------- arguments
def test_argument_errors():
    def err():
        return lib.hrpt_last_error(None).decode()
    d = RC.desc(10)
    keys, accum, resolved = native.rcache_table(d)
    drops, s, out = np.zeros(1, np.uint64), RC.samples((1, 2, 3), (0, 0, 1), (1, 1, 1)), np.zeros(4, np.float32)
    p = lambda a: a.ctypes.data       # noqa: E731
    assert lib.hrpt_rcache_insert_host(None, p(RC.CAM), p(keys), p(accum), p(drops), p(s), 1, 1) == -1 and err() == "hrpt_rcache_insert_host: null desc"
    for field, value in (("capacityLog2", 9), ("capacityLog2", 27), ("sceneScale", 0.0), ("radianceScale", np.inf), ("maxSamples", 0), ("maxSamples", 65536),
                         ("staleFramesMax", 65535), ("sparseBlock", 0), ("sparseBlock", 17), ("levelBias", np.nan), ("roughnessThreshold", np.nan)):
        bad = d.copy()
        bad[field] = value
        assert lib.hrpt_rcache_insert_host(p(bad), p(RC.CAM), p(keys), p(accum), p(drops), p(s), 1, 1) == -1 and err().startswith("hrpt_rcache_insert_host: capacityLog2 10..26"), field
        assert lib.hrpt_rcache_resolve_host(p(bad), p(keys), p(accum), p(resolved), 0, 1) == -1
    nan_cam = np.float32([0, np.nan, 0])
    assert lib.hrpt_rcache_insert_host(p(d), p(nan_cam), p(keys), p(accum), p(drops), p(s), 1, 1) == -1 and err() == "hrpt_rcache_insert_host: the camera position is not finite"
    assert lib.hrpt_rcache_insert_host(p(d), None, p(keys), p(accum), p(drops), p(s), 1, 1) == -1 and err() == "hrpt_rcache_insert_host: null cameraPos"
    assert lib.hrpt_rcache_insert_host(p(d), p(RC.CAM), None, p(accum), p(drops), p(s), 1, 1) == -1 and err() == "hrpt_rcache_insert_host: null array"
    assert lib.hrpt_rcache_insert_host(p(d), p(RC.CAM), p(keys), p(accum), p(drops), None, 1, 1) == -1
    assert lib.hrpt_rcache_insert_host(p(d), p(RC.CAM), p(keys), p(accum), p(drops), None, 0, 1) == 0
    assert lib.hrpt_rcache_resolve_host(p(d), p(keys), None, p(resolved), 0, 1) == -1 and err() == "hrpt_rcache_resolve_host: null array"
    assert lib.hrpt_rcache_resolve_host(p(d), p(keys), p(accum), p(resolved), 2, 1) == -1 and err() == "hrpt_rcache_resolve_host: unknown flags"
    pts = RC.points((1, 2, 3), (0, 0, 1))
    assert lib.hrpt_rcache_query_host(p(d), p(RC.CAM), p(keys), p(resolved), p(pts), None, None, 1, 1) == -1 and err() == "hrpt_rcache_query_host: null array"
    assert lib.hrpt_rcache_query_host(p(d), p(RC.CAM), p(keys), p(resolved), p(pts), p(out), None, 1, 1) == 0
    # an error changes nothing
    assert not keys.any() and not accum.view(np.uint8).any() and not drops.any()
    # the context calls on NULL
    assert lib.hrpt_rcache_create(None, p(d), None) == -1 and lib.hrpt_rcache_update(None, None, 0, 0) == -1
    assert lib.hrpt_rcache_indirect(None, None, None) == -1 and lib.hrpt_rcache_read(None, None, None, None, 0, None) == -1
    assert lib.hrpt_rcache_surfaces_device(None, None, None, 0, None) == -1 and lib.hrpt_read_rcache_served(None, None, 0) == -1
    lib.hrpt_rcache_destroy(None)


@pytest.mark.parametrize("seed", [5, 6])
def test_host_side_is_clean_under_the_sanitizers(seed):
    """pt_rcache.h + the host executors + a driver with its own main, built with AddressSanitizer and UBSan (`make rcache_asan`), chained as
    the update chains them: insert from several threads, resolve, query, over tables of 2^10 and 2^12 entries, full buckets and hostile
    samples, points, radiance and resolved records on exactly sized heap arrays. Nothing is loaded into Python."""
    subprocess.check_call(["make", "-C", CSRC, "rcache_asan"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(CSRC, "build", "rcache_asan"), str(seed)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "no report" in r.stdout
