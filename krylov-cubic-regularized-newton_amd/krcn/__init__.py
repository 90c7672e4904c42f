"""krcn — MI355X-native Krylov cubic-regularized-Newton hot path.

The native library (lib/libkrcn.so, sources in csrc/, ABI in include/krcn.h)
holds the HIP kernels; this package is its Python face: the device matrix
handle, the deterministic synthetic problem generator, and multi-GPU sharding.
"""
from . import synth  # noqa: F401
from ._lib import (KRCN_FORMAT_AUTO, KRCN_FORMAT_SORTED, KRCN_FORMAT_WAVE,  # noqa: F401
                   KRCN_FORMAT_JAG, KRCN_FORMAT_WINDOW, KrcnError, load)
from .device import DeviceCSR  # noqa: F401


def gram_geometry(d, n, split=0):
    """How DeviceCSR.hessian_gram cuts its work for a d-column, n-row matrix
    (krcn_gram_geometry; host arithmetic, no device): {'T': tile edge, 'KS':
    summed entries per slab, 'nt': tiles per side, 'tiles': upper-triangle
    tiles, 'slabs', 'split': workgroups per tile (split=0 asks the rule),
    'grid', 'ws_bytes': bytes of the split partials}."""
    import ctypes

    from . import _lib
    out = (ctypes.c_int64 * 8)()
    _lib.call("krcn_gram_geometry", int(d), int(n), int(split), out)
    return dict(zip(("T", "KS", "nt", "tiles", "slabs", "split", "grid", "ws_bytes"), (int(v) for v in out)))


__all__ = ["DeviceCSR", "KrcnError", "gram_geometry", "load", "synth"]
