"""ctypes wrappers of the event-verification entry points of libc2w_hip.so (include/c2w_hip.h: c2w_event_counts, c2w_fss_sums), in the
style of ``ops.py``; the host side that calls them is ``events.py``."""
from __future__ import annotations

import ctypes
from typing import Sequence

from . import _lib
from .ops import _accepted, _p, _stream


def _ints(values: Sequence[int]):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def counts_supported(hw: int, M: int, K: int) -> bool:
    return bool(_lib.load().c2w_event_counts_supported(hw, M, K))


def event_counts(x, y, thr, direction, counts, invalid, M, T, F, hw, K) -> bool:
    """counts (T, F, K, 2, M + 1) int64 = per plane and threshold the cells by (truth indicator, members with the event); invalid (T, F)
    int64 = the cells with a NaN among their M + 1 values, which are in no bin.  x (M, T, F, hw), y (T, F, hw) dense fp32, 16-byte
    aligned; thr (F, K) fp32 and direction (F, K) int32, 1 for ``x >= thr`` and 0 for ``x <= thr`` (include/c2w_hip.h::c2w_event_counts).
    Both outputs are zeroed by the call.  False if hw, M or K is not supported -- nothing is written and the caller takes the general
    definition."""
    rc = _lib.load().c2w_event_counts(_p(x), _p(y), _p(thr), _p(direction), _p(counts), _p(invalid), M, T, F, hw, K, _stream())
    return _accepted(rc, "c2w_event_counts")


def fss_supported(H: int, W: int, M: int, K: int, radii: Sequence[int]) -> bool:
    return bool(_lib.load().c2w_fss_supported(H, W, M, K, _ints(radii), len(radii)))


def fss_sums(x, y, thr, direction, sums, radii, M, T, F, H, W, K) -> bool:
    """sums (T, F, K, S, M + 2, 2) int64 = per plane, threshold, radius and row -- 0 the truth, 1 .. M the members, M + 1 the ensemble's
    member count -- ``(sum n_d^2, sum n_d n_0)`` over the cells, ``n_d`` the row's sum over the zero-padded ``(2r + 1)^2`` window
    (include/c2w_hip.h::c2w_fss_sums).  ``radii``: S host integers.  The output is zeroed by the call.  False if the shape or a radius is
    not supported -- nothing is written and the caller takes the general definition."""
    rc = _lib.load().c2w_fss_sums(_p(x), _p(y), _p(thr), _p(direction), _p(sums), _ints(radii), M, T, F, H, W, K, len(radii), _stream())
    return _accepted(rc, "c2w_fss_sums")
