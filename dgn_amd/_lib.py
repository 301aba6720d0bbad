"""ctypes binding of libdgn_hip.so (C ABI in include/dgn_hip.h).

There is NO fallback: if the shared library is missing or cannot be loaded, every
entry point raises -- the product path never computes on the CPU or through torch ops.
Build it with ``python -c "import __graft_entry__ as g; g.build()"`` or
``dgn_amd/csrc/build.sh`` (hipcc, --offload-arch=gfx950).
"""
from __future__ import annotations

import ctypes as C
import os
import threading

from . import _cabi


class DgnError(RuntimeError):
    pass


_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DGN_HIP_LIB") or os.path.join(_PKG, "libdgn_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "dgn_hip.h")


def read_abi(path: str) -> _cabi.Header:
    try:
        with open(path) as f:
            return _cabi.parse(f.read())
    except OSError as e:
        raise DgnError(f"{path}: cannot read the C ABI header the binding is derived from ({e}); there is no fallback") from e


# Everything the header declares, under the header's names: the DGN_* constants and the Dgn* structs as module attributes (once, at import)
_abi = read_abi(HEADER_PATH)
globals().update(_abi.constants)
globals().update(_abi.structs)
ABI_VERSION = _abi.constants["DGN_ABI_VERSION"]
EXPORTS = tuple(_abi.prototypes)      # every declared function, in header order (checked by tests/test_abi.py without a GPU)

_lib = None
_lock = threading.Lock()


def load() -> C.CDLL:
    """Load the shared library once; raise loudly if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise DgnError(f"{LIB_PATH} not found: the HIP extension is not built (run __graft_entry__.build() "
                           "or dgn_amd/csrc/build.sh). dgn_amd has no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in _abi.prototypes.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        if lib.dgn_abi_version() != ABI_VERSION:
            raise DgnError(f"libdgn_hip.so ABI {lib.dgn_abi_version()} != binding {ABI_VERSION}: rebuild")
        _lib = lib
    return _lib


class _Options:
    """The library's process-wide options as attributes (``dgn_set_option`` / ``dgn_get_option`` of the C ABI): ``options.blk_min_nodes = 0``.
    ``monkeypatch.setattr(_lib.options, name, value)`` switches one for a test and restores it."""

    def __getattr__(self, name):
        v = load().dgn_get_option(name.encode())
        if v == -2 ** 63:
            raise AttributeError(f"unknown libdgn_hip option '{name}'")
        return v

    def __setattr__(self, name, value):
        check(load().dgn_set_option(name.encode(), int(value)), "dgn_set_option")


options = _Options()


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise DgnError(f"{what} failed (rc={rc}): {load().dgn_last_error().decode()}")


def stream_ptr(device) -> int:
    """Raw handle of torch's current stream on ``device`` (what every entry point takes as its ``stream`` argument).
    ``torch.cuda.current_stream(d).cuda_stream`` builds a Stream object per call (~7 us of an eager step that is launch-bound)."""
    import torch
    idx = device.index if getattr(device, "index", None) is not None else torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(idx)
