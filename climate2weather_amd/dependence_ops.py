"""ctypes wrappers of the co-moment entry points of libc2w_hip.so (include/c2w_hip.h: c2w_comoments_update), in the style of
``extreme_ops.py``; the host side that calls them is ``dependence.py``."""
from __future__ import annotations

from . import _lib
from .ops import _accepted, _p, _stream


def supported(hw: int, F: int) -> bool:
    return bool(_lib.load().c2w_comoments_supported(hw, F))


def comoments_update(x, y, n, pivot, truth_pivot, sums, invalid, M, T, F, hw) -> bool:
    """``T`` consecutive hours: the state ``n (D, hw)`` int32, ``pivot (D, F, hw)`` and ``truth_pivot (D, F, hw)`` fp32 and
    ``sums (D, NS, hw)`` float64 is read and written; ``invalid (D,)`` int64 is ADDED to: the caller zeroed all of them when it made
    them.  x (M, T, F, hw) and y (T, F, hw) or None dense fp32, 16-byte aligned; ``D = M + 1`` and ``NS = 4 F + F (F + 1) / 2`` with a
    truth, else ``M`` and ``F + F (F + 1) / 2`` (``truth_pivot`` may then be None).  False if hw or F is not supported -- nothing is
    written and the caller takes the general definition."""
    rc = _lib.load().c2w_comoments_update(_p(x), _p(y), _p(n), _p(pivot), _p(truth_pivot), _p(sums), _p(invalid), M, T, F, hw, _stream())
    return _accepted(rc, "c2w_comoments_update")
