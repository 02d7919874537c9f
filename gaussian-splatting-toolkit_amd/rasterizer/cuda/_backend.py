"""Loader of the native library behind ``rasterizer.cuda``.

Counterpart of the reference's ``rasterizer/cuda/_backend.py`` (prebuilt
extension first, nvcc JIT otherwise).  Here there is exactly one backend: the
HIP library ``libgsraster.so`` (C ABI in ``include/gsraster.h``) built in-tree
for gfx950 by ``csrc/Makefile``.  There is no CPU or eager-PyTorch fallback: if
the library is missing the first native call raises.
"""
import ctypes as C
import os
import subprocess

from torch import Tensor

from ._prototypes import PROTOTYPES

PATH = os.path.dirname(os.path.abspath(__file__))
# (GSR_LIBRARY: another build of the same library, for A/B measurements of compile-time variants -- tools/r05/)
LIB_PATH = os.environ.get("GSR_LIBRARY") or os.path.join(PATH, "libgsraster.so")
CSRC = os.path.normpath(os.path.join(PATH, "..", "..", "csrc"))

# every entry include/gsraster.h declares, with its prototype (generated: tools/gen_prototypes.py)
SYMBOLS = tuple(PROTOTYPES)


class Pointer(C.c_void_p):
    """What the typed handle takes for a pointer parameter (any ``T *``, ``void *``, ``gsr_stream_t``): a tensor
    (its ``data_ptr()``, whatever the device and dtype), None (NULL), an int (an address or a stream handle) or what
    ``c_void_p`` itself converts -- a ``c_void_p``, ``byref(struct)``, a ctypes array.  Anything else, a float or a
    str for instance, is a ``ctypes.ArgumentError`` at the call."""

    @classmethod
    def from_param(cls, value):
        if isinstance(value, Tensor):
            # (c_void_p's own converter on the address: ~60 ns less per pointer than building a c_void_p, which on
            #  the host-bound 480 x 270 step is what keeps this path no slower than hand-wrapped arguments)
            return _void_p_from_param(value.data_ptr())
        if isinstance(value, (str, bytes)):  # (c_void_p would pass the characters' address)
            raise TypeError("tensor, None, address or ctypes pointer expected")
        return _void_p_from_param(value)


_void_p_from_param = C.c_void_p.from_param
_KINDS = {"p": Pointer, "i": C.c_int, "I": C.c_uint, "f": C.c_float, "d": C.c_double, "z": C.c_size_t,
          "q": C.c_longlong, "Q": C.c_ulonglong, "s": C.c_char_p}


def build(verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j8"]
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


def _load(typed: bool):
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"rasterizer: native library {LIB_PATH} not found. Build it with "
            f"`make -C {CSRC}` (needs hipcc); there is no fallback implementation."
        )
    lib = C.CDLL(LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    if missing:
        raise ImportError(f"rasterizer: {LIB_PATH} lacks symbols {missing}")
    for name, (ret, params) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = _KINDS[ret]
        if typed:
            fn.argtypes = [_KINDS[k] for k in params]
    return lib


_lib = _typed = None


def lib():
    """The raw handle: return types only.  A call through it marshals every argument itself and nothing checks it."""
    global _lib
    if _lib is None:
        _lib = _load(typed=False)
    return _lib


def typed():
    """The handle the package calls through: a second ``CDLL`` of the same file (the same loaded library and
    thread-local ``gsr_last_error``, its own function objects) on which every entry has the header's ``argtypes``.
    Call sites pass tensors, None, ints and floats; a wrong count is a ``TypeError``, a wrong kind a
    ``ctypes.ArgumentError``, before anything reaches the library."""
    global _typed
    if _typed is None:
        _typed = _load(typed=True)
    return _typed


__all__ = ["lib", "typed", "build", "LIB_PATH", "SYMBOLS", "PROTOTYPES", "Pointer"]
