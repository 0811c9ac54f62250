"""TEST DOUBLE for the temporal-increment launchers (climate2weather_amd.temporal_ops), on CPU tensors.

It restates the kernel of csrc/temporal.hip in NumPy with the index maps of csrc/temporal_core.h written out again in Python -- the
chunks of 4096 cells, the rounds of 256 threads with 4 adjacent cells each, the passes of 4 lags, the clamp of a lag past the end of the
series (its sums are dropped) -- and with the kernel's arithmetic in fp32, operation by operation and in the kernel's order, no multiply
fused with an add; the fold through LDS and over the chunks is emu_ordered_sum's.  Unsupported shapes answer False and write nothing.
``install`` also makes the temporal module treat CPU tensors as device tensors, so the host code takes the launcher's branch.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

from emu_ordered_sum import fold_parts, fold_workgroup, nan_if_not_finite, seq_sum

CALLS = []  # (n_rep, with_truth, T, F, hw, L) of every call that reached the launcher

THREADS, MAX_L, CHUNK, BATCH = 256, 24, 4096, 4


def tincr_supported(hw, L):
    return hw >= 4 and hw % 4 == 0 and 1 <= L <= MAX_L


def chunks(hw):
    return (hw + CHUNK - 1) // CHUNK


def passes(L):
    return (L + BATCH - 1) // BATCH


def lags_of(T, t, L):
    return min(L, T - 1 - t)


def tincr_scratch_bytes(rows, T, F, hw, L):
    if rows < 1 or T < 1 or F < 1 or not tincr_supported(hw, L):
        return 0
    return rows * T * F * chunks(hw) * 3 * L * 8 if chunks(hw) > 1 else 0


def workgroup_sums(terms):
    """terms (..., hw) fp32, one term per cell -> (..., chunks) float64 as the workgroups form them: thread tid of a chunk adds its
    cells (it 256 + tid) 4 + j in ascending order into a double, the 256 threads fold.  Cells past the end of the plane add +0.0, which
    changes no bit of a sum of non-negative terms that starts at +0.0."""
    assert terms.dtype == np.float32
    hw, nc = terms.shape[-1], chunks(terms.shape[-1])
    padded = np.zeros(terms.shape[:-1] + (nc * CHUNK,), np.float64)
    padded[..., :hw] = terms
    per_thread = padded.reshape(terms.shape[:-1] + (nc, CHUNK // (4 * THREADS), THREADS, 4))
    per_thread = np.moveaxis(per_thread, -2, -3).reshape(terms.shape[:-1] + (nc, THREADS, CHUNK // THREADS))
    return fold_workgroup(seq_sum(per_thread, -1), nan_if_not_finite)


def partial_terms(rows, with_truth, L):
    """rows (D, T, F, hw) fp32, row 0 the truth if with_truth -> partial (D, T, F, chunks, L, 3) float64, what the first launch writes"""
    f32 = np.float32
    assert rows.dtype == f32
    D, T, F, hw = rows.shape
    part = np.zeros((D, T, F, chunks(hw), L, 3), np.float64)
    with np.errstate(all="ignore"):
        for tau in range(1, min(L, T - 1) + 1):
            dx = rows[:, tau:] - rows[:, :-tau]   # (D, T - tau, F, hw) fp32
            sq = dx * dx
            assert dx.dtype == f32 and sq.dtype == f32
            part[:, :T - tau, :, :, tau - 1, 0] = workgroup_sums(np.abs(dx))
            part[:, :T - tau, :, :, tau - 1, 1] = workgroup_sums(sq)
            if with_truth:
                e = dx - dx[:1]
                ee = e * e
                assert ee.dtype == f32
                part[:, :T - tau, :, :, tau - 1, 2] = workgroup_sums(ee)
    return part


def tincr_terms(x, y, S, scratch, n_rep, T, F, hw, L):
    CALLS.append((int(n_rep), y is not None, int(T), int(F), int(hw), int(L)))
    if not tincr_supported(hw, L):
        return False
    for t in (x, y):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0)
    D, nc = n_rep + (y is not None), chunks(hw)
    n = D * T * F * L * 3
    assert S.dtype == torch.float64 and S.is_contiguous() and S.numel() >= n
    need = tincr_scratch_bytes(D, T, F, hw, L)
    assert need == 0 or (scratch is not None and scratch.dtype == torch.float64 and scratch.numel() * 8 >= need)
    rows = x.reshape(n_rep, T, F, hw).numpy()
    if y is not None:
        rows = np.concatenate([y.reshape(1, T, F, hw).numpy(), rows])
    part = partial_terms(rows, y is not None, L)
    if nc > 1:
        scratch.reshape(-1).numpy()[:n * nc] = part.reshape(-1)
    out = fold_parts(part, 3, nan_if_not_finite) if nc > 1 else part[:, :, :, 0]
    S.reshape(-1).numpy()[:n] = out.reshape(-1)
    return True


def install(monkeypatch, ops_module, temporal_module):
    me = sys.modules[__name__]
    del CALLS[:]
    for name in ("tincr_supported", "tincr_scratch_bytes", "tincr_terms"):
        monkeypatch.setattr(ops_module, name, getattr(me, name))
    monkeypatch.setattr(temporal_module, "_on_device", lambda x: True)
