"""ctypes wrappers of the temporal-increment entry points of libc2w_hip.so (include/c2w_hip.h: c2w_tincr_*), in the style of
``ops.py``; the host side that calls them is ``temporal.py``."""
from __future__ import annotations

from . import _lib
from .ops import _accepted, _nbytes, _p, _stream


def tincr_supported(hw: int, L: int) -> bool:
    return bool(_lib.load().c2w_tincr_supported(hw, L))


def tincr_scratch_bytes(rows: int, T: int, F: int, hw: int, L: int) -> int:
    """bytes of scratch ``tincr_terms`` needs for ``rows`` rows -- the data sets, and the truth if there is one (0 while a plane is one
    chunk of 4096 cells)"""
    return int(_lib.load().c2w_tincr_scratch_bytes(rows, T, F, hw, L))


def tincr_terms(x, y, S, scratch, n_rep, T, F, hw, L) -> bool:
    """S (D, T, F, L, 3) float64 = per row, anchor time, variable and lag the sums over the cells of ``(|dx|, dx^2, (dx - dy)^2)``, from x
    (n_rep, T, F, hw) and y (T, F, hw) or None -- dense fp32, 16-byte aligned; the rows are y, if given, then x
    (include/c2w_hip.h::c2w_tincr_terms: the definition, the special cases, the fixed summation order).  scratch: a float64 device tensor
    of at least ``tincr_scratch_bytes`` bytes, or None where that is 0.  False if hw or L is not supported -- nothing is written and the
    caller takes the general definition."""
    rc = _lib.load().c2w_tincr_terms(_p(x), _p(y), _p(S), _p(scratch), _nbytes(scratch), n_rep, T, F, hw, L, _stream())
    return _accepted(rc, "c2w_tincr_terms")
