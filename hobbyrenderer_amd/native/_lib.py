"""The loaded library, the one place an entry point's signature is declared, and the argument converters every wrapper shares."""
import ctypes as C
import os

import numpy as np

from .. import structs as S

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # hobbyrenderer_amd/: the libraries, .cache/ and csrc/ live here
LIB_PATH = os.environ.get("HRPT_LIBRARY") or os.path.join(_PKG, "libhobbyrt_pt.so")   # HRPT_LIBRARY: A/B another build of the same ABI

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build it with `make -C hobbyrenderer_amd/csrc` (or __graft_entry__.build()). "
        "The HIP library is the only backend of this package.")

# One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 / libhsa-runtime64 (soname libamdhip64.so.7)
# and RCCL is linked against it. If libhobbyrt_pt.so were loaded first it would pull /opt/rocm's copy in as a SECOND
# runtime, and whichever initialises the GPU second then finds no device. Importing torch first makes the dynamic
# loader satisfy our DT_NEEDED libamdhip64.so.7 with the already loaded copy. Without torch the ROCm copy is used.
try:
    import torch  # noqa: F401
except ImportError:  # pure-ctypes use (no multi-GPU): /opt/rocm's runtime through the library's RUNPATH
    torch = None

lib = C.CDLL(LIB_PATH)
EXPORTS = []        # every entry point declare() has seen, in declaration order


def declare(name, argtypes, restype=C.c_int):
    """The one declaration of entry point `name` (its prototype in include/hobbyrt_pt.h; tests/test_binding_contract.py compares the two)."""
    fn = getattr(lib, name)
    fn.argtypes, fn.restype = argtypes, restype
    EXPORTS.append(name)


class HrptError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"hrpt error {code}: {message}")
        self.code = code


declare("hrpt_last_error", [C.c_void_p], restype=C.c_char_p)


def _check_rc(rc):
    """A call without a context: its message is the library's process-wide one."""
    if rc != 0:
        raise HrptError(rc, lib.hrpt_last_error(None).decode())


def address(p):
    """A device address or a stream handle (an int, any NumPy integer, 0 or None) as a c_void_p argument; 0 and None are both NULL."""
    return int(p) if p else None


def records(a, name):
    """`a` as a C-contiguous array of the structs record `name`; an array of another dtype is refused rather than reinterpreted."""
    dtype = getattr(S, name)
    if isinstance(a, np.ndarray) and a.dtype != dtype:
        raise ValueError(f"{name} records expected, got an array of dtype {a.dtype}")
    return np.ascontiguousarray(a, dtype)


def or_default(params, cls, *args):
    """The caller's parameter record, or a default-constructed one."""
    return params if params is not None else cls(*args)


def _ptr(a):
    return None if a is None else a.ctypes.data


_COUNT_WORDS = {1: "one", 2: "two", 4: "four", 5: "five"}


def _same_shape_images(name, required, **optional):
    """The image arguments of a host wrapper as contiguous float32 arrays: `required` all [H, W, 4] of one shape, each optional one None or
    of that shape. Returns (required, optional in the order given, shape)."""
    imgs = [np.ascontiguousarray(a, np.float32) for a in required]
    shape = imgs[0].shape
    if len(shape) != 3 or shape[2] != 4 or any(a.shape != shape for a in imgs):
        raise ValueError(f"{name}: {_COUNT_WORDS[len(imgs)]} float32 [H, W, 4] images of one size expected")
    opt = []
    for key, a in optional.items():
        a = None if a is None else np.ascontiguousarray(a, np.float32)
        if a is not None and a.shape != shape:
            raise ValueError(f"{name}: {key} must have the images' shape")
        opt.append(a)
    return imgs, opt, shape


def _frame_params(constants, accum_count, tile, flags, stripes):
    p = np.zeros((), S.FrameParams)
    p["stripeCount"], p["stripeIndex"] = stripes
    p["constants"] = constants
    p["accumCount"] = accum_count
    p["tileX0"], p["tileY0"], p["tileX1"], p["tileY1"] = tile
    p["flags"] = flags
    return p
