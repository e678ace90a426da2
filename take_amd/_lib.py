"""Loading libtake_hip.so: the one place that knows where the library is and gives every entry point its prototype.

There is no fallback: if the shared object is missing or no HIP device is visible every call raises `TakeError`.
"""
import ctypes as C
import os
import subprocess

from . import cdefs as D

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TAKE_HIP_LIB") or os.path.join(_PKG, "libtake_hip.so")  # TAKE_HIP_LIB: tuning builds
_LIB = None

EXPORTS = sorted(D.PROTOTYPES)


class TakeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"take_hip error {code}: {msg}")
        self.code = code


def build(force=False):
    """Compile libtake_hip.so for gfx950 with hipcc (take_amd/csrc/Makefile).  Cross-compiles without a GPU."""
    src = os.path.join(_PKG, "csrc")
    args = ["make", "-C", src]
    if force:
        args.append("-B")
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libtake_hip.so failed:\n" + r.stdout[-4000:])
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise TakeError(-3, f"{LIB_PATH} not built (run __graft_entry__.build() / make -C take_amd/csrc)")
        L = C.CDLL(LIB_PATH)
        for name, argtypes in D.PROTOTYPES.items():
            f = getattr(L, name)
            f.argtypes = argtypes
            if name in D.RESTYPES:
                f.restype = D.RESTYPES[name]
        _LIB = L
    return _LIB


def _check(rc):
    if rc < 0:
        raise TakeError(rc, lib().take_hip_last_error().decode())
    return rc


def device_count():
    return _check(lib().take_hip_device_count())
