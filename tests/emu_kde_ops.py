"""TEST DOUBLE for the marginals launchers (climate2weather_amd.ops: kde_supported, kde_scratch_bytes, kde_eval, pit_supported,
pit_counts), on CPU tensors.

It restates the three kernels of csrc/kde.hip in NumPy with the index maps of csrc/kde_core.h written out again in Python -- the chunk
bounds, the value-to-(time, cell) map, the fold order, the rank histogram's workgroup-to-(variable, times) map and its bin rule -- and
with the kernel's arithmetic in fp32: x - pivot on the loaded value, gk = offset * k formed in double and rounded once, t = fma(-(x -
pivot), k, gk), exp2(-(t t)), chains of 256 terms in fp32 folded into doubles in value order, partial[ds][chunk][j] in the scratch, the
chunks added in index order.  (The grid-point-to-thread map moves no arithmetic; tests/host_kde_main.cpp checks it.)  Unsupported shapes
answer False and write nothing.  ``install`` also makes the marginals module treat CPU tensors as device tensors, so the host code takes
the launcher's branch.
"""
from __future__ import annotations

import math
import sys

import numpy as np
import torch

CALLS = []  # ("kde", n_rep, T, F, hw, N, with_truth) / ("pit", M, T, F, hw) of every call that reached a launcher

THREADS, TILE, FOLD, MAX_CHUNKS, MAX_N, PIT_MAX_M, PIT_COPIES = 256, 1024, 256, 64, 1024, 64, 16
SQRT_HALF_LOG2E = math.sqrt(math.log2(math.e) / 2.0)
CUS = 256  # what the launcher's CU count is on an MI355X


# ------------------------------------------------------------------------------------------------------------------ kde_core.h, restated

def chunk_len(n):
    per = (n + MAX_CHUNKS - 1) // MAX_CHUNKS
    return max(TILE, (per + TILE - 1) // TILE * TILE)


def chunks(n):
    return (n + chunk_len(n) - 1) // chunk_len(n)


def chunk_bounds(n, c):
    return c * chunk_len(n), min(n, (c + 1) * chunk_len(n))


def value_offset(i, F, hw):
    return (i // hw) * (F * hw) + i % hw


def set_base(ds, n_x, T, F, hw):
    """(which buffer, the float offset of the data set's first value, its variable)"""
    if ds < n_x:
        return 0, ((ds // F) * T * F + ds % F) * hw, ds % F
    return 1, (ds - n_x) * hw, ds - n_x


def pit_grid(T, F):
    per_var = min(T, max(1, CUS * 8 // F))
    return per_var * F


# ------------------------------------------------------------------------------------------------------------------ the launchers

def kde_supported(hw, N):
    return hw >= 4 and hw % 4 == 0 and 1 <= N <= MAX_N


def kde_scratch_bytes(D, n, N):
    return D * chunks(n) * N * 8


def _fma32(a, b, c):
    """fp32 fma: the product of two fp32 is exact in float64; the float64 sum is rounded once more to fp32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def kde_eval(x, y, offsets, pivot, h, scratch, dens, n_rep, T, F, hw, N):
    CALLS.append(("kde", int(n_rep), int(T), int(F), int(hw), int(N), y is not None))
    if not kde_supported(hw, N):
        return False
    for t in (x, y):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0)
    n_x, n = n_rep * F, T * hw
    D, nc = n_x + (F if y is not None else 0), chunks(n)
    assert offsets.dtype == torch.float32 and offsets.is_contiguous() and tuple(offsets.shape) == (F, N)
    assert pivot.dtype == torch.float32 and pivot.numel() == F and h.dtype == torch.float64 and h.is_contiguous() and h.numel() == D
    assert scratch.dtype == torch.float64 and scratch.numel() * 8 >= kde_scratch_bytes(D, n, N)
    assert dens.dtype == torch.float64 and dens.is_contiguous() and dens.numel() >= D * N
    bufs = (x.reshape(-1).numpy(), None if y is None else y.reshape(-1).numpy())
    off, piv, hh = offsets.numpy(), pivot.numpy(), h.numpy()
    part = scratch.reshape(-1).numpy()
    part[:D * nc * N] = np.nan  # every entry that is read must have been written by a workgroup
    with np.errstate(all="ignore"):
        for ds in range(D):
            which, base, f = set_base(ds, n_x, T, F, hw)
            k = np.float32(SQRT_HALF_LOG2E / hh[ds])
            gk = (off[f].astype(np.float64) * np.float64(k)).astype(np.float32)
            for c in range(nc):
                lo, hi = chunk_bounds(n, c)
                i = np.arange(lo, hi)
                xo = bufs[which][base + value_offset(i, F, hw)] - piv[f]
                assert xo.dtype == np.float32
                tot = np.zeros(N, np.float64)
                for first in range(0, hi - lo, FOLD):  # a chain starts at every multiple of 256 values of the chunk
                    t = _fma32(-xo[first:first + FOLD, None], k, gk[None, :])
                    e = np.exp2(-(t * t))
                    assert e.dtype == np.float32
                    e[e < np.float32(2.0 ** -126)] = 0.0  # the instruction flushes what is below the smallest normal
                    tot += np.cumsum(e, axis=0, dtype=np.float32)[-1].astype(np.float64)
                bad = not np.all(np.isfinite(xo))
                part[(ds * nc + c) * N:(ds * nc + c + 1) * N] = np.nan if bad else tot
        out = dens.reshape(-1).numpy()
        for ds in range(D):
            s = np.zeros(N, np.float64)
            for c in range(nc):
                s = s + part[(ds * nc + c) * N:(ds * nc + c + 1) * N]
            out[ds * N:(ds + 1) * N] = np.where(np.isnan(s), np.nan, s * (1.0 / (float(n) * hh[ds] * math.sqrt(2.0 * math.pi))))
    return True


def pit_supported(hw, M):
    return hw >= 4 and hw % 4 == 0 and 1 <= M <= PIT_MAX_M


def pit_counts(x, y, counts, M, T, F, hw):
    CALLS.append(("pit", int(M), int(T), int(F), int(hw)))
    if not pit_supported(hw, M):
        return False
    for t in (x, y):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
    assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() >= F * (M + 1)
    xs, ys = x.reshape(-1).numpy(), y.reshape(-1).numpy()
    out = counts.reshape(-1).numpy()
    out[:F * (M + 1)] = 0
    G = pit_grid(T, F)
    plane, member = F * hw, T * F * hw
    cell = np.arange(hw)
    tid = (cell // 4) % THREADS  # the thread that owns a cell's quad
    for b in range(G):
        f = b % F
        hist = np.zeros((PIT_COPIES, M + 1), np.int64)
        for t in range(b // F, T, G // F):
            at = t * plane + f * hw + cell
            with np.errstate(invalid="ignore"):
                r = sum((xs[m * member + at] <= ys[at]).astype(np.int64) for m in range(M))
            np.add.at(hist, (tid % PIT_COPIES, r), 1)
        out[f * (M + 1):(f + 1) * (M + 1)] += hist.sum(axis=0)
    return True


def install(monkeypatch, ops_module, marginals_module):
    me = sys.modules[__name__]
    del CALLS[:]
    for name in ("kde_supported", "kde_scratch_bytes", "kde_eval", "pit_supported", "pit_counts"):
        monkeypatch.setattr(ops_module, name, getattr(me, name))
    monkeypatch.setattr(marginals_module, "_on_device", lambda x: True)
