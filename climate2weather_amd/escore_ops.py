"""ctypes wrappers of the energy-score and variogram-score entry points of libc2w_hip.so (include/c2w_hip.h: c2w_escore_*,
c2w_vario_*), in the style of ``ops.py``; the host side that calls them is ``multivariate.py``."""
from __future__ import annotations

from . import _lib
from .ops import _accepted, _nbytes, _p, _stream


def escore_supported(hw: int, M: int) -> bool:
    return bool(_lib.load().c2w_escore_supported(hw, M))


def escore_scratch_bytes(planes: int, hw: int, M: int) -> int:
    """bytes of scratch ``escore_pairs`` needs (0 while a plane is one chunk of 256 cells)"""
    return int(_lib.load().c2w_escore_scratch_bytes(planes, hw, M))


def escore_pairs(x, y, d2, scratch, M, planes, hw) -> bool:
    """d2 (planes, M (M + 1) / 2) float64 = the squared distances of every pair of the rows y, x_1 .. x_M of every plane, from x
    (M, planes, hw) and y (planes, hw) -- dense fp32, 16-byte aligned (include/c2w_hip.h::c2w_escore_pairs: the definition, the pair
    order, the fixed summation order).  scratch: a float64 device tensor of at least ``escore_scratch_bytes`` bytes, or None where that
    is 0.  False if hw or M is not supported -- nothing is written and the caller takes the general definition."""
    return _accepted(_lib.load().c2w_escore_pairs(_p(x), _p(y), _p(d2), _p(scratch), _nbytes(scratch), M, planes, hw, _stream()), "c2w_escore_pairs")


def vario_supported(H: int, W: int, R: int, M: int, order2: int) -> bool:
    return bool(_lib.load().c2w_vario_supported(H, W, R, M, order2))


def vario_scratch_bytes(planes: int, H: int, W: int, R: int) -> int:
    """bytes of scratch ``vario_terms`` needs (0 while a plane is one tile of 8 x 32 cells)"""
    return int(_lib.load().c2w_vario_scratch_bytes(planes, H, W, R))


def vario_terms(x, y, V, scratch, M, planes, H, W, R, order2) -> bool:
    """V (planes, O, 3) float64 = per offset of the half-plane stencil of radius R the sums over its cell pairs of
    ``((g_y - g_x)^2, g_y, g_x)`` at the order ``order2 / 2``, from x (M, planes, H, W) and y (planes, H, W), dense fp32
    (include/c2w_hip.h::c2w_vario_terms).  scratch as for ``escore_pairs``.  False if the shape, R, M or the order is not supported --
    nothing is written and the caller takes the general definition."""
    rc = _lib.load().c2w_vario_terms(_p(x), _p(y), _p(V), _p(scratch), _nbytes(scratch), M, planes, H, W, R, order2, _stream())
    return _accepted(rc, "c2w_vario_terms")
