"""ctypes binding of the C ABI in ``include/mi355r.h`` (``libmi355r.so``).

The library is the product: there is no CPU or PyTorch fallback. If the shared
object is missing or fails to load, importing a GPU entry point raises
``RuntimeError`` (build it with ``python -m torch_renderer_amd._build`` or
``__graft_entry__.build()``).

Nothing of the ABI is restated here: the ``MR_*`` constants, the struct classes (``MrView``,
``MrRasterSettings``, ``MrShadeParams``, ``MrOpencvPoses``, ``MrPoses``, ``MrMesh``) and every function's
``restype`` / ``argtypes`` are read from the header, once, at import (``_abi.read_header``).
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch  # noqa: F401  -- must be imported first: the .so shares torch's HIP runtime

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmi355r.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "mi355r.h")


def read_header(path: str = HEADER_PATH) -> _abi.Abi:
    if not os.path.exists(path):
        raise RuntimeError(f"mi355r: C ABI header not found at {path}. The binding is read from it: "
                           "keep include/mi355r.h beside the package.")
    with open(path) as fh:
        return _abi.read_header(fh.read())


ABI = read_header()
globals().update(ABI.constants)  # MR_OK, MR_OUT_DEPTH, ...
globals().update(ABI.structs)  # MrView, MrRasterSettings, MrShadeParams, MrOpencvPoses, MrPoses, MrMesh
EXPORTED_SYMBOLS = [name for name, _, _ in ABI.prototypes]

_lib = None
_lock = threading.Lock()


def load(path: str | None = None) -> ctypes.CDLL:
    """Load (once) and return the library. Raises RuntimeError if it is missing."""
    global _lib
    with _lock:
        if _lib is not None and path is None:
            return _lib
        p = path or os.environ.get("MI355R_LIB") or LIB_PATH  # override: experiment builds
        if not os.path.exists(p):
            raise RuntimeError(
                f"mi355r: native library not found at {p}. Build it first "
                "(python -m torch_renderer_amd._build). There is no CPU fallback.")
        lib = ctypes.CDLL(p)
        for name, res, args in ABI.prototypes:
            fn = getattr(lib, name, None)
            if fn is None and path is None and not os.environ.get("MI355R_LIB"):
                raise RuntimeError(f"mi355r: {p} does not export {name} (stale build?)")
            if fn is None:  # an experiment build older than the current ABI
                continue
            fn.restype = res
            fn.argtypes = args
        if path is None:
            _lib = lib
        return lib


_EXT = None


def torch_ext():
    """The fused render's autograd node in C++ (``_mr_torch.so``, csrc/mr_torch.cpp), bound to the C ABI
    functions of the library ``load()`` returned. Raises RuntimeError if it is missing (no fallback)."""
    global _EXT
    with _lock:
        if _EXT is not None:
            return _EXT
    path = os.path.join(_HERE, "_mr_torch.so")
    if not os.path.exists(path):
        raise RuntimeError(f"mi355r: {path} not found. Build it first (python -m torch_renderer_amd._build).")
    import importlib.util

    spec = importlib.util.spec_from_file_location("_mr_torch", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import torch

    built = getattr(mod, "built_with_torch", "unknown")
    abi = getattr(mod, "built_with_cxx11_abi", None)
    if built != torch.__version__ or (abi is not None and bool(abi) != bool(torch._C._GLIBCXX_USE_CXX11_ABI)):
        raise RuntimeError(f"mi355r: {path} was built against torch {built} (cxx11 ABI {abi}), this process runs "
                           f"torch {torch.__version__} (cxx11 ABI {torch._C._GLIBCXX_USE_CXX11_ABI}): rebuild it "
                           "(python -m torch_renderer_amd._build)")
    lib = load()
    # (abi_functions: the entry points the node calls, as mr_torch.cpp lists them)
    mod.init({name: ctypes.cast(getattr(lib, name), ctypes.c_void_p).value for name in mod.abi_functions})
    with _lock:
        _EXT = mod
    return mod


def check(rc: int) -> None:
    if rc != 0:
        msg = load().mr_last_error().decode(errors="replace")
        if rc == ABI.constants["MR_EUNSUPPORTED"]:
            raise NotImplementedError(f"mi355r: {msg}")
        raise RuntimeError(f"mi355r error {rc}: {msg}")


def ptr(t):
    """Device (or host) pointer of a contiguous tensor, or None."""
    if t is None:
        return None
    assert t.is_contiguous(), "mi355r: tensors passed across the C ABI must be contiguous"
    return ctypes.c_void_p(t.data_ptr())


def strided_ptr(t):
    """Pointer of a tensor whose layout the callee takes as explicit strides (e.g. a broadcast
    view with batch stride 0)."""
    return ctypes.c_void_p(t.data_ptr())


def stream_handle(device=None):
    """The current HIP stream of `device` (torch.device, index or None: the current device) as a handle:
    the raw stream pointer, without building a torch Stream object per launch."""
    if isinstance(device, torch.device):
        idx = device.index if device.index is not None else torch.cuda.current_device()
    elif isinstance(device, int):
        idx = device
    else:
        idx = torch.cuda.current_device()
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(idx))


def timing_enable(on: bool = True) -> None:
    check(load().mr_timing_enable(1 if on else 0))


def timing_read() -> dict:
    """{kernel name: (launches, total_ms)} for launches recorded since timing_enable(True)."""
    L = load()
    n = L.mr_timing_kernel_count()
    launches = (ctypes.c_int32 * n)()
    total = (ctypes.c_double * n)()
    check(L.mr_timing_read(ctypes.cast(launches, ctypes.c_void_p), ctypes.cast(total, ctypes.c_void_p), n))
    return {L.mr_timing_kernel_name(k).decode(): (launches[k], total[k]) for k in range(n) if launches[k]}
