"""The vertex quantiser without a GPU (hrpt_quantize_vertices_host): csrc/pt_deform.h on host threads against the
NumPy statement of QuantizeVertex (scenes.quantize_vertices), as bytes; the rows that statement leaves undefined; counts and thread counts;
the ABI of the new calls; and the sanitizer build of the host side (`make deform_asan`, a stand-alone program).
(libhobbyrt_scene's C++ QuantizeVertex has no Python binding, so it is not compared here.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hobbyrenderer_amd import native, structs as S
import deform_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hobbyrenderer_amd", "csrc")


@pytest.fixture(scope="module")
def inputs():
    v = D.float_vertices()
    return v, D.numpy_quantised(v)


def test_quantiser_bits_equal_the_numpy_statement(inputs):
    v, ref = inputs
    got = native.quantize_vertices_host(v, nthreads=1)
    bad = np.nonzero(got.view(np.uint32).reshape(-1, 6) != ref.view(np.uint32).reshape(-1, 6))[0]
    assert got.tobytes() == ref.tobytes(), (len(bad), v[bad[0]], got[bad[0]], ref[bad[0]])
    # the edge rows did what they are there for: both ends of every field, the flushed and the saturated half, the empty tangent
    n = got["m_Normal"][:1152]
    assert (n & 1023).min() == 0 and (n & 1023).max() == 1022 and ((n >> 30) & 1).any() and not (n >> 31).any()
    assert {0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0x7BFF} <= set((got["m_Uv"][:1152] & 0xFFFF).tolist()) | set((got["m_Uv"][:1152] >> 16).tolist())
    assert (got["m_Tangent"][:1152] == 0).any() and (got["m_Tangent"] >> 16 == 0).all()


@pytest.mark.parametrize("count", [0, 1, D.COUNT])
def test_counts_and_thread_counts(inputs, count):
    v, ref = inputs
    for nthreads in (1, 3, 64):
        got = native.quantize_vertices_host(v[:count], nthreads=nthreads)
        assert len(got) == count and got.tobytes() == ref[:count].tobytes(), nthreads


def test_nan_counts_as_zero():
    rows, zeroed, words = D.nan_vertices()
    got, want = native.quantize_vertices_host(rows), native.quantize_vertices_host(zeroed)
    normal_rows = words < 0
    assert got[normal_rows].tobytes() == want[normal_rows].tobytes()
    assert got[normal_rows].tobytes() == D.numpy_quantised(zeroed[normal_rows]).tobytes()
    assert got["m_Tangent"][~normal_rows].tolist() == words[~normal_rows].tolist()
    for f in ("m_Pos", "m_Normal", "m_Uv"):                      # an infinite tangent touches the tangent word alone
        assert got[f][~normal_rows].tobytes() == D.numpy_quantised(_finite_tangent(rows[~normal_rows]))[f].tobytes()


def _finite_tangent(v):
    v = v.copy()
    v["tangent"][:, :3] = (1, 0, 0)
    return v


def test_abi_and_argument_errors():
    assert S.VertexFloat.itemsize == 48 and S.ABI_VERSION == 3      # that the C header says the same: test_binding_contract.py
    one_in, one_out = np.zeros(1, S.VertexFloat), np.zeros(1, S.VertexQuantized)
    assert native.lib.hrpt_quantize_vertices_host(None, 1, one_out.ctypes.data, 1) == -1
    assert native.lib.hrpt_quantize_vertices_host(one_in.ctypes.data, 1, None, 1) == -1
    assert native.lib.hrpt_quantize_vertices_host(None, 0, None, 1) == 0
    for name in ("hrpt_update_vertices", "hrpt_update_vertices_device", "hrpt_quantize_vertices_device"):      # no context: an error, not a crash
        fn = getattr(native.lib, name)
        assert fn(*[None if t is C.c_void_p else 0 for t in fn.argtypes]) == -1, name


@pytest.mark.parametrize("seed", [5, 6])
def test_host_side_is_clean_under_the_sanitizers(seed):
    """pt_deform.h + the host executor + a driver with its own main, built with AddressSanitizer and UBSan (`make deform_asan`), over random
    and hostile vertices (NaN, inf, huge and denormal values in every field), counts 0 and 1, more threads than vertices. Nothing is loaded
    into Python."""
    subprocess.check_call(["make", "-C", CSRC, "deform_asan"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([os.path.join(CSRC, "build", "deform_asan"), str(seed)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "no report" in r.stdout
