"""ctypes wrappers of the event-spell entry points of libc2w_hip.so (include/c2w_hip.h: c2w_spell_update), in the style of
``event_ops.py``; the host side that calls them is ``spells.py``."""
from __future__ import annotations

from . import _lib
from .ops import _accepted, _p, _stream


def supported(hw: int, K: int, max_duration: int, period: int) -> bool:
    return bool(_lib.load().c2w_spell_supported(hw, K, max_duration, period))


def spell_update(x, y, thr, direction, state, hist, onsets, invalid, M, T, F, hw, K, max_duration, period, t0) -> bool:
    """One block of ``T`` times, the first of them the absolute hour ``t0``: ``state (4, D, F, K, hw)`` int32 -- open, longest, count,
    hours of every series -- is read and written; ``hist (D, F, K, max_duration)``, ``onsets (D, F, K, period)`` (None at
    ``period = 0``) and ``invalid (D, F)`` int64 are ADDED to: the caller zeroed them when it made them.  x (M, T, F, hw) and y
    (T, F, hw) or None dense fp32, 16-byte aligned; ``D = M + 1`` with a truth, else ``M``; thr (F, K) fp32 and direction (F, K) int32,
    1 for ``x >= thr`` and 0 for ``x <= thr`` (include/c2w_hip.h::c2w_spell_update).  False if hw, K, max_duration or period is not
    supported -- nothing is written and the caller takes the general definition."""
    rc = _lib.load().c2w_spell_update(_p(x), _p(y), _p(thr), _p(direction), _p(state), _p(hist), _p(onsets), _p(invalid), M, T, F, hw, K,
                                      max_duration, period, t0, _stream())
    return _accepted(rc, "c2w_spell_update")
