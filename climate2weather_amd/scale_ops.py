"""ctypes wrappers of the block-moment entry points of libc2w_hip.so (include/c2w_hip.h: c2w_block_moments), in the style of
``dependence_ops.py``; the host side that calls them is ``scalesplit.py``."""
from __future__ import annotations

from . import _lib
from .ops import _accepted, _p, _stream


def supported(H: int, W: int, s: int) -> bool:
    return bool(_lib.load().c2w_block_moments_supported(H, W, s))


def block_moments(x, y, n, pivot, sums, M, T, F, H, W, s) -> bool:
    """The tables of one call: ``n`` int32 and ``pivot`` fp32 ``(D, T, F, h, w)`` and ``sums (D, T, F, NS, h, w)`` float64 are
    written, every element.  x (M, T, F, H, W) and y (T, F, H, W) or None dense fp32, 16-byte aligned; ``D = M + 1`` and ``NS = 3`` with
    a truth, else ``M`` and 2; ``h = H / s``, ``w = W / s``.  False if the shape is not supported -- nothing is written and the caller
    takes the general definition."""
    rc = _lib.load().c2w_block_moments(_p(x), _p(y), _p(n), _p(pivot), _p(sums), M, T, F, H, W, s, _stream())
    return _accepted(rc, "c2w_block_moments")
