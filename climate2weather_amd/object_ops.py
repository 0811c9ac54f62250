"""ctypes wrappers of the event-object entry points of libc2w_hip.so (include/c2w_hip.h: c2w_object_tables), in the style of
``spell_ops.py``; the host side that calls them is ``objects.py``."""
from __future__ import annotations

from . import _lib
from .ops import _accepted, _p, _stream


def supported(H: int, W: int, K: int, connectivity: int, max_objects: int) -> bool:
    return bool(_lib.load().c2w_objects_supported(H, W, K, connectivity, max_objects))


def object_tables(x, y, thr, direction, plane, area_hist, objects, invalid, M, T, F, H, W, K, connectivity, max_objects) -> bool:
    """The objects of the ``D T F K`` planes of x (M, T, F, H W) and y (T, F, H W) or None, dense fp32, 16-byte aligned; ``D = M + 1``
    with a truth, else ``M``; thr (F, K) fp32 and direction (F, K) int32, 1 for ``x >= thr`` and 0 for ``x <= thr``.  ``plane
    (D, T, F, K, 6)`` int64, ``objects (D, T, F, K, max_objects, 8)`` int32 (None at ``max_objects = 0``) and ``invalid (D, T, F)`` int64
    are WRITTEN, every entry; ``area_hist (D, F, K, B)`` int64, ``B = floor(log2(H W)) + 1``, is ADDED to: the caller zeroed it when
    it made it (include/c2w_hip.h::c2w_object_tables).  False if H, W, K, connectivity or max_objects is not supported -- nothing is
    written and the caller takes the general definition."""
    rc = _lib.load().c2w_object_tables(_p(x), _p(y), _p(thr), _p(direction), _p(plane), _p(area_hist), _p(objects), _p(invalid), M, T, F, H, W, K,
                                       connectivity, max_objects, _stream())
    return _accepted(rc, "c2w_object_tables")
