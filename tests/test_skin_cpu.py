"""The vertex producer without a GPU (hrpt_skin_vertices_host): csrc/pt_skin.h on host threads against its NumPy
statement (tests/skin_reference.py), as bytes, with and without joints and targets, over counts and thread counts and on the edge rows
of the definition; the statement against a float64 formulation that shares nothing with it; skinning followed by the quantiser; the ABI
of the new calls and their argument errors; and the sanitizer build of the host side (`make skin_asan`, a stand-alone program). The
reference renderer has no skinning: parity unpinned by the reference."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hobbyrenderer_amd import native, scenes, structs as S
import skin_cases as K
import skin_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hobbyrenderer_amd", "csrc")
COUNTS = [1, 63, 64, 65, 257, 1025, 4096]
COMBINATIONS = {"skin": (True, False), "morph": (False, True), "both": (True, True), "neither": (False, False)}


@pytest.fixture(scope="module")
def case():
    return K.random_case()


@pytest.fixture(scope="module")
def statement(case):
    """The NumPy statement of every combination over all 4 096 vertices, with NumPy's floating-point warnings as errors: the statement
    stays defined on the random rows. A vertex depends on nothing but itself, so a shorter count is a prefix."""
    with np.errstate(invalid="raise", divide="raise", over="raise"):
        return {k: R.skin(**K.select(case, skin=s, morph=m)) for k, (s, m) in COMBINATIONS.items()}


def _first_difference(got, want):
    bad = np.nonzero((got.view(np.uint32).reshape(-1, 12) != want.view(np.uint32).reshape(-1, 12)).any(1))[0]
    return (len(bad), int(bad[0]), got[bad[0]], want[bad[0]]) if len(bad) else None


@pytest.mark.parametrize("combination", list(COMBINATIONS))
@pytest.mark.parametrize("count", COUNTS)
def test_host_executor_equals_the_numpy_statement(case, statement, combination, count):
    s, m = COMBINATIONS[combination]
    want = statement[combination][:count]
    for nthreads in (1, 3, 16):
        got = native.skin_vertices_host(**K.select(case, count, skin=s, morph=m), nthreads=nthreads)
        assert len(got) == count and got.tobytes() == want.tobytes(), (nthreads, _first_difference(got, want))


def test_edge_rows():
    e = K.edge_case()
    want = R.skin(**e)
    got = native.skin_vertices_host(**e, nthreads=3)
    assert got.tobytes() == want.tobytes(), _first_difference(got, want)
    assert np.isfinite(got["pos"]).all() and np.isfinite(got["normal"]).all() and np.isfinite(got["tangent"]).all()     # the inf target was skipped
    rows = [(i, s, z) for i in K.EDGE_INFLUENCES for s in K.EDGE_SIGNS for z in (False, True)]
    morphed = R.skin(e["base"], deltas=e["deltas"], morph_weights=e["morph_weights"])
    for k, ((joints, _), sign, zero) in enumerate(rows):
        length = np.linalg.norm(got["normal"][k].astype(np.float64))
        if joints == (0, 0, 0, 0):                                       # identity: the morphed vertex, normalised
            assert got[k].tobytes() == morphed[k].tobytes()
        if joints == (1, 1, 1, 1):                                       # singular: zero vectors are kept, not divided
            assert not got["normal"][k].any() and not got["tangent"][k, :3].any()
            assert got["pos"][k].tolist() == e["joint_matrices"][1, :, 3].tolist()
        elif zero:
            assert length == 0
        else:
            assert abs(length - 1) < 3e-7
        flipped = joints in ((2, 0, 0, 0), (2, 3, 2, 3))                 # determinant < 0
        assert got["tangent"][k, 3].tobytes() == np.float32(-sign if flipped else sign).tobytes(), (k, joints, sign)
        if joints == (2, 0, 0, 0) and not zero:                          # the mirror in x of the morphed vertex
            assert np.allclose(got["normal"][k], morphed["normal"][k] * (-1, 1, 1), atol=3e-7)
    assert {0x00000000, 0x80000000, 0x3F800000, 0xBF800000} == set(got["tangent"][:, 3].view(np.uint32).tolist())


def test_statement_against_float64(case, statement):
    """Allowance: four times the deviations measured when the stage was defined (7.9e-7 per normal component, 1.1e-6 relative per
    position), over all 4 096 vertices with none excluded. Measured on this generator: 7.9e-7 per normal component, 1.1e-6 relative
    position, 7.6e-7 per tangent component, which is held to the normal's allowance: a blend that nearly cancels shortens B t as it
    shortens the cofactors' product, and the normalisation magnifies the rounding of either by the same condition number. Blended
    3 x 3 condition numbers reach 6.4e3; unit lengths deviate by at most 1.1e-7."""
    got = statement["both"]
    p, n, t, s, cond = R.skin_float64(**case)
    normal = np.abs(got["normal"] - n).max()
    tangent = np.abs(got["tangent"][:, :3] - t).max()
    position = (np.abs(got["pos"] - p).max(1) / np.abs(p).max(1)).max()
    unit = np.abs(np.linalg.norm(got["normal"].astype(np.float64), axis=1) - 1).max()
    print(f"normal {normal:.3e} tangent {tangent:.3e} position {position:.3e} unit {unit:.3e} cond max {cond.max():.1f}")
    assert normal <= 4 * 7.9e-7 and tangent <= 4 * 7.9e-7 and position <= 4 * 1.1e-6
    assert unit <= 3e-7                                                  # two roundings of a unit vector's components
    assert got["tangent"][:, 3].tolist() == s.tolist() and (got["tangent"][:, 3] != case["base"]["tangent"][:, 3]).any()
    assert got["uv"].tobytes() == case["base"]["uv"].tobytes()
    for k, (sk, mo) in COMBINATIONS.items():                             # the other combinations, against the same formulation
        p, n, t, s, _ = R.skin_float64(**K.select(case, skin=sk, morph=mo))
        g = statement[k]
        assert np.abs(g["normal"] - n).max() <= 4 * 7.9e-7 and (np.abs(g["pos"] - p).max(1) / np.abs(p).max(1)).max() <= 4 * 1.1e-6, k


def test_skin_then_quantise(case, statement):
    v = statement["both"]
    want = scenes.quantize_vertices(v["pos"], v["normal"], v["uv"], v["tangent"][:, :3], v["tangent"][:, 3])
    got = native.quantize_vertices_host(native.skin_vertices_host(**case))
    assert got.tobytes() == want.tobytes()
    assert ((got["m_Normal"] >> 30) & 1).any() and not ((got["m_Normal"] >> 30) & 1).all()


def test_abi():
    assert C.sizeof(S.SkinArgs) == 64 and S.ABI_VERSION == 3 and S.SkinMorphDelta.itemsize == 36      # that the C header says the same: test_binding_contract.py
    for name in ("hrpt_skin_vertices_host", "hrpt_skin_vertices_device", "hrpt_update_vertices_skinned"):
        assert name in native.EXPORTS and getattr(native.lib, name)


def _call(arrays, out, count=None, joint_count=None, target_count=None, reserved=0, offsets=None):
    """hrpt_skin_vertices_host on raw addresses: arrays = (base, joints, weights, matrices, deltas, morph weights), None = NULL."""
    addresses = [None if a is None else a.ctypes.data + (offsets or {}).get(k, 0) for k, a in enumerate(arrays)]
    args = S.SkinArgs(*addresses, count, joint_count, target_count, reserved)
    return native.lib.hrpt_skin_vertices_host(C.byref(args), None if out is None else out.ctypes.data, 1)


def test_argument_errors(case):
    small = K.select(case, 8)
    arrays, n, jc, tc = native.skin_arrays(**small)
    arrays = [native._aligned_copy(a) for a in arrays]
    out = native._aligned_copy(np.zeros(n, S.VertexFloat))
    assert _call(arrays, out, n, jc, tc) == 0
    assert out.tobytes() == native.skin_vertices_host(**small).tobytes()
    assert native.lib.hrpt_skin_vertices_host(None, out.ctypes.data, 1) == -1                    # NULL args
    assert _call(arrays, out, n, jc, tc, reserved=1) == -1
    assert _call(arrays, None, n, jc, tc) == -1                                                   # NULL out
    for k, step in enumerate((8, 4, 8, 8, 2, 2)):                                                 # each pointer off its alignment
        assert _call(arrays, out, n, jc, tc, offsets={k: step}) == -1, k
    base, joints, weights, matrices, deltas, mw = arrays
    assert _call([None, joints, weights, matrices, deltas, mw], out, n, jc, tc) == -1             # NULL base with count > 0
    assert _call([base, joints, None, matrices, deltas, mw], out, n, jc, tc) == -1                # joints without weights
    assert _call([base, joints, weights, None, deltas, mw], out, n, jc, tc) == -1                 # ... without matrices
    assert _call(arrays, out, n, 0, tc) == -1                                                     # ... with jointCount == 0
    assert _call([base, joints, weights, matrices, None, mw], out, n, jc, tc) == -1               # targets without deltas
    assert _call([base, joints, weights, matrices, deltas, None], out, n, jc, tc) == -1           # ... without weights
    assert _call([base, None, None, None, None, None], out, n, 0, 0) == 0                         # neither: normalisation alone
    assert _call([None] * 6, None, 0, 0, 0) == 0 and _call(arrays, out, 0, jc, tc) == 0           # count 0
    for name in ("hrpt_skin_vertices_device", "hrpt_update_vertices_skinned"):                    # no context: an error, not a crash
        fn = getattr(native.lib, name)
        assert fn(*[0 if t is C.c_uint32 else None for t in fn.argtypes]) == -1, name


def test_joint_index_out_of_range_writes_nothing(case):
    small = K.select(case, 1030, morph=False)
    arrays, n, jc, tc = native.skin_arrays(**small)
    arrays = [None if a is None else native._aligned_copy(a) for a in arrays]
    arrays[1][1027, 3] = jc                                              # in the second chunk of the executor
    out = native._aligned_copy(np.full(n * 12, 7.5, np.float32).view(S.VertexFloat))
    assert _call(arrays, out, n, jc, 0) == -1
    assert (out.view(np.float32) == 7.5).all()
    with pytest.raises(native.HrptError) as e:
        native.skin_vertices_host(small["base"], arrays[1], small["weights"], small["joint_matrices"])
    assert e.value.code == -1 and "joint index out of range" in str(e.value)


@pytest.mark.parametrize("seed", [5, 6])
def test_host_side_is_clean_under_the_sanitizers(seed):
    """pt_skin.h + the host executor + a driver with its own main, built with AddressSanitizer and UBSan (`make skin_asan`): random, edge and
    hostile inputs over exactly sized arrays, 1, 3 and 16 threads, unaligned tail counts, and a joint index out of range, which the
    executor refuses and the shared function clamps. Nothing is loaded into Python."""
    subprocess.check_call(["make", "-C", CSRC, "skin_asan"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(CSRC, "build", "skin_asan"), str(seed)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "no report" in r.stdout
