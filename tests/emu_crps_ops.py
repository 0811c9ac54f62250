"""TEST DOUBLE for the CRPS launchers (climate2weather_amd.ops: crps_supported, crps_scratch_bytes, crps_terms), on CPU tensors.

It restates the two kernels of csrc/crps.hip in NumPy with the index maps of csrc/crps_core.h written out again in Python -- the chunk
bounds, the (round, thread, column) -> cell map, the per-thread accumulation order; the fold through LDS and the fold over the chunks
are emu_ordered_sum's -- and with the kernel's arithmetic in fp32, operation by operation and in the kernel's order: the sort (any
correct sort gives the network's rows), the gaps times the exact weights, the pivot x_(M / 2), the offsets against it, no multiply fused
with an add.  Unsupported shapes answer False and write nothing.  ``install`` also makes the crps module treat CPU tensors as device
tensors, so the host code takes the launcher's branch.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

from emu_ordered_sum import fold_parts, fold_workgroup, nan_if_nan, seq_sum

CALLS = []  # (M, T, F, hw, with_cells) of every call that reached the launcher

THREADS, MAX_M, CHUNK = 256, 64, 4096


# ------------------------------------------------------------------------------------------------------------------ crps_core.h, restated

def rows_of(M):
    return 8 if M <= 8 else 16 if M <= 16 else 32 if M <= 32 else 64


def cells_per_thread(K):
    return 4 if K <= 16 else 2 if K == 32 else 1


def chunks(hw):
    return (hw + CHUNK - 1) // CHUNK


def chunk_bounds(hw, c):
    return c * CHUNK, min(hw, (c + 1) * CHUNK)


def rounds(hw, c, V):
    lo, hi = chunk_bounds(hw, c)
    return (hi - lo + V * THREADS - 1) // (V * THREADS)


def crps_supported(hw, M):
    return hw >= 4 and hw % 4 == 0 and 1 <= M <= MAX_M


def crps_scratch_bytes(T, F, hw):
    return T * F * chunks(hw) * 4 * 8 if chunks(hw) > 1 else 0


# ------------------------------------------------------------------------------------------------------------------ the arithmetic

def cell_terms32(x, y):
    """x (M, n) fp32, y (n,) fp32 -> (4, n) fp32: the kernel's per-cell arithmetic, every operation rounded to fp32 in its order"""
    M = x.shape[0]
    f32 = np.float32
    assert x.dtype == f32 and y.dtype == f32
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(x).all(axis=0) & np.isfinite(y))
        s = np.sort(np.where(np.isnan(x), f32(np.inf), x), axis=0)
        rM = f32(1.0 / M)
        rM1 = f32(1.0 / (M - 1)) if M > 1 else f32(0)
        a, b = np.zeros_like(y), np.zeros_like(y)
        for i in range(M):
            a = a + np.abs(s[i] - y)
            if i > 0:
                b = b + f32(i * (M - i)) * (s[i] - s[i - 1])
        p = s[M // 2]
        es = np.zeros_like(y)
        for i in range(M):
            es = es + (s[i] - p)
        ebar = es * rM
        ss = np.zeros_like(y)
        for i in range(M):
            d = (s[i] - p) - ebar
            ss = ss + d * d
        t = (p - y) + ebar
        out = np.stack([a * rM, b, t * t, ss * rM1 if M > 1 else np.full_like(y, np.nan)])
        assert out.dtype == f32
        out[:, bad] = np.nan
    return out


def thread_sums(terms, V):
    """terms (4, n) fp32 of one chunk in cell order -> (4, 256) float64: what each thread accumulates, in (round, column) order"""
    n = terms.shape[1]
    per_round = V * THREADS
    R = (n + per_round - 1) // per_round
    padded = np.zeros((4, R * per_round), np.float64)  # a thread without cells adds nothing: its accumulator stays +0
    padded[:, :n] = terms
    t = padded.reshape(4, R, THREADS, V).transpose(0, 2, 1, 3).reshape(4, THREADS, R * V)
    return seq_sum(t, 2)


def crps_terms(x, y, sums, cells, scratch, M, T, F, hw):
    CALLS.append((int(M), int(T), int(F), int(hw), cells is not None))
    if not crps_supported(hw, M):
        return False
    for t in (x, y):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
    assert sums.dtype == torch.float64 and sums.is_contiguous() and sums.numel() >= T * F * 4
    nc, V = chunks(hw), cells_per_thread(rows_of(M))
    need = crps_scratch_bytes(T, F, hw)
    assert need == 0 or (scratch is not None and scratch.dtype == torch.float64 and scratch.numel() * 8 >= need)
    xs, ys = x.reshape(M, T * F, hw).numpy(), y.reshape(T * F, hw).numpy()
    out = sums.reshape(-1).numpy()
    part = np.full((T * F, nc, 4), np.nan)  # every entry that is read must have been written by a workgroup
    cl = None
    if cells is not None:
        assert cells.dtype == torch.float32 and cells.is_contiguous() and cells.numel() >= 4 * T * F * hw and cells.data_ptr() % 16 == 0
        cl = cells.reshape(-1).numpy()[:4 * T * F * hw].reshape(4, T * F, hw)
    for pl in range(T * F):
        for c in range(nc):
            lo, hi = chunk_bounds(hw, c)
            terms = cell_terms32(xs[:, pl, lo:hi], ys[pl, lo:hi])
            if cl is not None:
                cl[:, pl, lo:hi] = terms
            part[pl, c] = fold_workgroup(thread_sums(terms, V), nan_if_nan)
    if nc > 1:
        scratch.reshape(-1).numpy()[:T * F * nc * 4] = part.reshape(-1)
    out[:T * F * 4] = (fold_parts(part, 1, nan_if_nan) if nc > 1 else part[:, 0]).reshape(-1)
    return True


def install(monkeypatch, ops_module, crps_module):
    me = sys.modules[__name__]
    del CALLS[:]
    for name in ("crps_supported", "crps_scratch_bytes", "crps_terms"):
        monkeypatch.setattr(ops_module, name, getattr(me, name))
    monkeypatch.setattr(crps_module, "_on_device", lambda x: True)
