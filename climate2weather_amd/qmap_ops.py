"""ctypes wrappers of the quantile-mapping entry points of libc2w_hip.so (include/c2w_hip.h: c2w_qmap_*), in the style of
``temporal_ops.py``; the host side that calls them is ``biascorrect.py``."""
from __future__ import annotations

from . import _lib
from .ops import _accepted, _nbytes, _p, _stream


def qmap_supported(hw: int, K: int, max_len: int) -> bool:
    return bool(_lib.load().c2w_qmap_supported(hw, K, max_len))


def qmap_scratch_bytes(rows: int, cells: int, Tu: int) -> int:
    """bytes of series-major scratch ``qmap_nodes`` needs for a block of ``cells`` cells of ``rows = n_rep F`` (member, variable) pairs
    and ``Tu`` listed times"""
    return int(_lib.load().c2w_qmap_scratch_bytes(rows, cells, Tu))


def qmap_nodes(x, tidx, goff, levels, q, n_valid, scratch, n_rep, T, F, hw, Tu, G, K, max_len, skipna, c0, c1) -> bool:
    """The cells ``[c0, c1)`` of q (n_rep, G, F, hw, K) float64 and n_valid (n_rep, G, F, hw) int64 from x (n_rep, T, F, hw) dense fp32:
    per series -- one variable at one cell over the times ``tidx[goff[g]:goff[g + 1]]`` of group g -- the quantiles at ``levels`` (K,)
    float64 (include/c2w_hip.h::c2w_qmap_nodes: the definition).  tidx (Tu,) and goff (G + 1,) are int32 device tensors, max_len the
    longest group.  scratch: an fp32 device tensor of at least ``qmap_scratch_bytes(n_rep F, c1 - c0, Tu)`` bytes.  False if hw, K or
    max_len is not supported -- nothing is written and the caller takes the general definition."""
    rc = _lib.load().c2w_qmap_nodes(_p(x), _p(tidx), _p(goff), _p(levels), _p(q), _p(n_valid), _p(scratch), _nbytes(scratch), n_rep, T, F, hw, Tu,
                                    G, K, max_len, 1 if skipna else 0, c0, c1, _stream())
    return _accepted(rc, "c2w_qmap_nodes")


def qmap_apply(x, out, xq, yq, tidx, goff, n_rep, T, F, hw, Tu, G, K, max_len) -> bool:
    """out (n_rep, T, F, hw) fp32 = x mapped through the tables xq, yq (G, F, hw, K) float64 of its cell and of its time's group
    (include/c2w_hip.h::c2w_qmap_apply: the arithmetic); ``out`` may be ``x``.  A time that is not in tidx is not written.  False if hw,
    K or max_len is not supported -- nothing is written."""
    rc = _lib.load().c2w_qmap_apply(_p(x), _p(out), _p(xq), _p(yq), _p(tidx), _p(goff), n_rep, T, F, hw, Tu, G, K, max_len, _stream())
    return _accepted(rc, "c2w_qmap_apply")
