"""ctypes binding of libgm_hip.so (C-ABI declared in include/gm_hip.h).

There is NO fallback: if the HIP library is missing or a call fails, this raises.  The product
path never routes through torch eager kernels or the CPU oracle for the ops bound here."""
import ctypes
import os

from ._abi import *  # noqa: F401,F403  (the C-ABI's structs, constants and tables stay reachable as _lib.X)
from ._abi import _SIGNATURES

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GM_LIB_PATH") or os.path.join(HERE, "libgm_hip.so")

_lib = None


class GMError(RuntimeError):
    pass


def check_int(v, name, error=GMError):
    """int(v) of an integer (Python's or numpy's, no bool); else `error`: the models' argument validator, raised as
    the calling module's own error class."""
    import numpy as np
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise error("%s must be an integer, got %r" % (name, v))
    return int(v)


def check_real(v, name, error=GMError):
    """float(v) of a finite number (Python's or numpy's, no bool); else `error`."""
    import math
    import numpy as np
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise error("%s must be a number, got %r" % (name, v))
    v = float(v)
    if not math.isfinite(v):
        raise error("%s must be finite, got %r" % (name, v))
    return v


def check_seed(seed, name="seed", error=GMError):
    """A counter-generator seed: an integer in [0, 2^64); else `error`."""
    seed = check_int(seed, name, error)
    if not 0 <= seed < 1 << 64:
        raise error("%s must lie in [0, 2^64), got %d" % (name, seed))
    return seed


def load():
    """Load libgm_hip.so; raise loudly if it is not there (build with __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise GMError("HIP extension %s is missing -- run `python __graft_entry__.py build` "
                      "(hipcc --offload-arch=gfx950); there is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().gm_last_error()
        raise GMError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else "?"))


def call(name, *args):
    check(getattr(load(), name)(*args), name)
