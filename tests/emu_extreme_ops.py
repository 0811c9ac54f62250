"""TEST DOUBLE for the extremes launchers (climate2weather_amd.extreme_ops), on CPU tensors.

It restates block_extremes_kernel and lmoments_kernel of csrc/extremes.hip in NumPy with the maps of csrc/extremes_maps.h written out
again in Python: a workgroup per (row, variable, chunk of 1024 cells), the open keys read from ``open_keys`` and written back where they
were read, the walk over the hours in order with an unsigned maximum of directed keys, a store to the table where an hour is the last
of its block and nowhere else, one add of the NaN hours per workgroup to ``invalid``, which is NOT zeroed here; and for the moments the
pads and NaNs as +inf, a sort, the pivot, the four sums in ascending order, one division each.  Unsupported arguments answer False and
write nothing.  ``install`` also makes the extremes module treat CPU tensors as device tensors, so the host code takes the launcher's
branch."""
from __future__ import annotations

import sys

import numpy as np
import torch

CALLS = []  # ("update", M, T, F, hw, block, B, t0) / ("lmoments", R, n, hw) of every call that reached a launcher

THREADS, CELLS, CHUNK, MAX_BLOCK, MAX_B, MAX_T, MAX_N = 256, 4, 1024, 1 << 20, 4096, 1 << 20, 64
NONE, NAN_BITS = 0, 0x7FC00000


def update_supported(hw, block, max_blocks):
    return hw >= 4 and hw % 4 == 0 and 1 <= block <= MAX_BLOCK and 1 <= max_blocks <= MAX_B


def lmoments_supported(hw, n):
    return hw >= 4 and hw % 4 == 0 and 1 <= n <= MAX_N


def chunks(hw):
    return (hw + CHUNK - 1) // CHUNK


def _dkey(bits, flip):
    key = bits ^ np.where(bits >> np.uint32(31) != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))
    nan = (bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, np.uint32(NONE), key ^ flip), nan


def _extreme_bits(dkey, flip):
    key = dkey ^ flip
    bits = key ^ np.where(key >> np.uint32(31) != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))
    return np.where(dkey == NONE, np.uint32(NAN_BITS), bits)


def block_extremes_update(x, y, direction, open_keys, table, invalid, M, T, F, hw, block, max_blocks, t0):
    CALLS.append(("update", int(M), int(T), int(F), int(hw), int(block), int(max_blocks), int(t0)))
    if not update_supported(hw, block, max_blocks) or M < 1:
        return False
    for t in (x,) + (() if y is None else (y,)):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
    D, B = M + (0 if y is None else 1), max_blocks
    assert direction.dtype == torch.int32 and direction.is_contiguous() and direction.numel() >= F
    assert open_keys.dtype == torch.int32 and open_keys.is_contiguous() and open_keys.numel() >= D * F * hw and open_keys.data_ptr() % 16 == 0
    assert table.dtype == torch.float32 and table.is_contiguous() and table.numel() >= D * F * B * hw and table.data_ptr() % 16 == 0
    assert invalid.dtype == torch.int64 and invalid.is_contiguous() and invalid.numel() >= D * F
    assert 0 <= T <= MAX_T and t0 >= 0 and (t0 + T) // block <= B
    if T == 0:
        return True
    xs = x.reshape(M, T, F, hw).numpy()
    rows = (xs if y is None else np.concatenate([y.reshape(1, T, F, hw).numpy(), xs])).view(np.uint32)
    op = open_keys.reshape(-1).numpy()[:D * F * hw].reshape(D, F, hw).view(np.uint32)       # views: written in place
    tb = table.reshape(-1).numpy()[:D * F * B * hw].reshape(D, F, B, hw).view(np.uint32)
    inv = invalid.reshape(-1).numpy()[:D * F].reshape(D, F)
    dirs = direction.reshape(-1).numpy()
    for d in range(D):
        for f in range(F):
            flip = np.uint32(0 if dirs[f] else 0xFFFFFFFF)
            for c in range(chunks(hw)):
                lo, hi = c * CHUNK, min(hw, (c + 1) * CHUNK)
                cur = op[d, f, lo:hi].copy()                                                 # the threads' registers
                b, left, lds_invalid = t0 // block, block - t0 % block, 0
                for t in range(T):
                    k, nan = _dkey(rows[d, t, f, lo:hi], flip)
                    lds_invalid += int(nan.sum())
                    cur = np.maximum(cur, k)
                    left -= 1
                    if left == 0:
                        tb[d, f, b, lo:hi] = _extreme_bits(cur, flip)
                        cur[:] = NONE
                        left, b = block, b + 1
                op[d, f, lo:hi] = cur                                                        # stored where they were loaded
                inv[d, f] += lds_invalid
    return True


def lmoments(table, lmom, n_valid, R, n, hw):
    CALLS.append(("lmoments", int(R), int(n), int(hw)))
    if not lmoments_supported(hw, n):
        return False
    assert table.dtype == torch.float32 and table.is_contiguous() and table.numel() >= R * n * hw and table.data_ptr() % 16 == 0
    assert lmom.dtype == torch.float64 and lmom.is_contiguous() and lmom.numel() >= R * 4 * hw
    assert n_valid.dtype == torch.int32 and n_valid.is_contiguous() and n_valid.numel() >= R * hw
    if R == 0:
        return True
    t = table.reshape(-1).numpy()[:R * n * hw].reshape(R, n, hw)
    out = lmom.reshape(-1).numpy()[:R * 4 * hw].reshape(R, 4, hw)
    nvo = n_valid.reshape(-1).numpy()[:R * hw].reshape(R, hw)
    K = 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64
    nan = np.isnan(t)
    nv = (~nan).sum(axis=1)                                                                  # (R, hw)
    s = np.full((R, K, hw), np.inf, np.float32)
    s[:, :n] = np.where(nan, np.float32(np.inf), t)
    s = np.sort(s, axis=1).astype(np.float64)
    p = np.take_along_axis(s, (nv // 2)[:, None, :], axis=1)[:, 0]
    S = np.zeros((4, R, hw))
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(n):
            e = np.where(j < nv, s[:, j] - p, 0.0)
            S[0] += e
            S[1] += float(j) * e
            S[2] += float(j * (j - 1)) * e
            S[3] += float(j * (j - 1) * (j - 2)) * e
        m = nv.astype(np.int64)
        den = [m, m * (m - 1), m * (m - 1) * (m - 2), m * (m - 1) * (m - 2) * (m - 3)]
        b = [S[r] / den[r].astype(np.float64) for r in range(4)]
        l = [p + b[0], 2.0 * b[1] - b[0], (6.0 * b[2] - 6.0 * b[1]) + b[0], ((20.0 * b[3] - 30.0 * b[2]) + 12.0 * b[1]) - b[0]]
    for r in range(4):
        out[:, r] = np.where(nv >= r + 1, l[r], np.nan)
    nvo[:] = nv
    return True


def install(monkeypatch, ops_module, extremes_module):
    me = sys.modules[__name__]
    del CALLS[:]
    for name in ("update_supported", "lmoments_supported", "block_extremes_update", "lmoments"):
        monkeypatch.setattr(ops_module, name, getattr(me, name))
    monkeypatch.setattr(extremes_module, "_on_device", lambda x: True)
