"""ctypes wrappers of the extremes entry points of libc2w_hip.so (include/c2w_hip.h: c2w_block_extremes_update, c2w_lmoments), in the
style of ``spell_ops.py``; the host side that calls them is ``extremes.py``."""
from __future__ import annotations

from . import _lib
from .ops import _accepted, _p, _stream


def update_supported(hw: int, block: int, max_blocks: int) -> bool:
    return bool(_lib.load().c2w_block_extremes_supported(hw, block, max_blocks))


def lmoments_supported(hw: int, n: int) -> bool:
    return bool(_lib.load().c2w_lmoments_supported(hw, n))


def block_extremes_update(x, y, direction, open_keys, table, invalid, M, T, F, hw, block, max_blocks, t0) -> bool:
    """``T`` consecutive hours, the first of them the absolute hour ``t0``: ``open_keys (D, F, hw)`` int32 -- the bit patterns of the
    open block's running keys, 0 for "no value yet" -- is read and written; the extreme of every block whose last hour lies in the call
    is stored in ``table (D, F, max_blocks, hw)`` fp32 at index ``t // block``; ``invalid (D, F)`` int64 is ADDED to: the caller zeroed
    it when it made it.  x (M, T, F, hw) and y (T, F, hw) or None dense fp32, 16-byte aligned; ``D = M + 1`` with a truth, else ``M``;
    direction (F,) int32, 1 for maxima and 0 for minima.  False if hw, block or max_blocks is not supported -- nothing is written and the
    caller takes the general definition."""
    rc = _lib.load().c2w_block_extremes_update(_p(x), _p(y), _p(direction), _p(open_keys), _p(table), _p(invalid), M, T, F, hw, block, max_blocks,
                                               t0, _stream())
    return _accepted(rc, "c2w_block_extremes_update")


def lmoments(table, lmom, n_valid, R, n, hw) -> bool:
    """``table (R, n, hw)`` fp32 -> ``lmom (R, 4, hw)`` float64 and ``n_valid (R, hw)`` int32 (include/c2w_hip.h::c2w_lmoments).  False
    if hw or n is not supported -- nothing is written."""
    rc = _lib.load().c2w_lmoments(_p(table), _p(lmom), _p(n_valid), R, n, hw, _stream())
    return _accepted(rc, "c2w_lmoments")
