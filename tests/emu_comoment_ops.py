"""TEST DOUBLE for the co-moment launchers (climate2weather_amd.dependence_ops), on CPU tensors.

It restates comoments_update_kernel of csrc/comoments.hip in NumPy with the maps of csrc/comoments_maps.h written out again in Python:
a workgroup per (row, chunk of 256 V(F) cells), the state (n, the pivots, the NS doubles a cell) read once and written back where it
was read, the walk over the hours in order in which an hour that is not valid is walked WITH THE PIVOT IN THE VALUE'S PLACE (every
difference +0.0, every product +0.0: the kernel has no branch there), every accumulator a plain ``s = s + term`` with the product
rounded on its own, and one add of the invalid cell-hours per workgroup to ``invalid``, which is NOT zeroed here.  Unsupported
arguments answer False and write nothing.  ``install`` also makes the dependence module treat CPU tensors as device tensors, so the
host code takes the launcher's branch."""
from __future__ import annotations

import sys

import numpy as np
import torch

CALLS = []  # (M, T, F, hw, with_truth) of every call that reached the launcher

THREADS, UNROLL, MAX_F, MAX_T = 256, 4, 8, 1 << 20


def cells_per_thread(F):
    return 4 if F <= 1 else 2 if F <= 2 else 1


def chunk_cells(F):
    return THREADS * cells_per_thread(F)


def entries(F, with_truth):
    return F + F * (F + 1) // 2 + (3 * F if with_truth else 0)


def supported(hw, F):
    return hw >= 4 and hw % 4 == 0 and 1 <= F <= MAX_F


def chunks(hw, F):
    return (hw + chunk_cells(F) - 1) // chunk_cells(F)


def _finite(a):
    return (a.view(np.uint32) & np.uint32(0x7F800000)) != np.uint32(0x7F800000)


def comoments_update(x, y, n, pivot, truth_pivot, sums, invalid, M, T, F, hw):
    CALLS.append((int(M), int(T), int(F), int(hw), y is not None))
    if not supported(hw, F) or M < 1:
        return False
    truth = y is not None
    D, NS, NP = M + (1 if truth else 0), entries(F, truth), F * (F + 1) // 2
    for t in (x,) + ((y, truth_pivot) if truth else ()):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
    assert n.dtype == torch.int32 and n.is_contiguous() and n.numel() >= D * hw and n.data_ptr() % 16 == 0
    assert pivot.dtype == torch.float32 and pivot.is_contiguous() and pivot.numel() >= D * F * hw and pivot.data_ptr() % 16 == 0
    assert sums.dtype == torch.float64 and sums.is_contiguous() and sums.numel() >= D * NS * hw and sums.data_ptr() % 16 == 0
    assert invalid.dtype == torch.int64 and invalid.is_contiguous() and invalid.numel() >= D
    assert 0 <= T <= MAX_T
    if T == 0:
        return True
    xs = x.reshape(M, T, F, hw).numpy()
    ys = y.reshape(T, F, hw).numpy() if truth else None
    nn = n.reshape(-1).numpy()[:D * hw].reshape(D, hw)                                        # views: written in place
    P = pivot.reshape(-1).numpy()[:D * F * hw].reshape(D, F, hw)
    PT = truth_pivot.reshape(-1).numpy()[:D * F * hw].reshape(D, F, hw) if truth else None
    S = sums.reshape(-1).numpy()[:D * NS * hw].reshape(D, NS, hw)
    inv = invalid.reshape(-1).numpy()[:D]
    pairs = [(f, g) for f in range(F) for g in range(f, F)]
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(D):
            row = (ys if d == 0 else xs[d - 1]) if truth else xs[d]                           # (T, F, hw)
            for c in range(chunks(hw, F)):
                lo, hi = c * chunk_cells(F), min(hw, (c + 1) * chunk_cells(F))
                cn, cp, cs = nn[d, lo:hi].copy(), P[d, :, lo:hi].copy(), S[d, :, lo:hi].copy()  # the threads' registers
                cpt = PT[d, :, lo:hi].copy() if truth else None
                lds_invalid = 0
                for t in range(T):
                    a = row[t, :, lo:hi]
                    valid = _finite(a).all(axis=0)
                    if truth:
                        b = ys[t, :, lo:hi]
                        valid &= _finite(b).all(axis=0)
                    first = valid & (cn == 0)
                    cn += valid
                    lds_invalid += int((~valid).sum())
                    cp = np.where(first, a, cp)
                    e = np.where(valid, a, cp).astype(np.float64) - cp.astype(np.float64)
                    cs[:F] = cs[:F] + e
                    for k, (f, g) in enumerate(pairs):
                        term = e[f] * e[g]
                        cs[F + k] = cs[F + k] + term
                    if truth:
                        cpt = np.where(first, b, cpt)
                        eT = np.where(valid, b, cpt).astype(np.float64) - cpt.astype(np.float64)
                        q, xx = eT * eT, e * eT
                        cs[F + NP:2 * F + NP] = cs[F + NP:2 * F + NP] + eT
                        cs[2 * F + NP:3 * F + NP] = cs[2 * F + NP:3 * F + NP] + q
                        cs[3 * F + NP:] = cs[3 * F + NP:] + xx
                nn[d, lo:hi], P[d, :, lo:hi], S[d, :, lo:hi] = cn, cp, cs                     # stored where they were loaded
                if truth:
                    PT[d, :, lo:hi] = cpt
                inv[d] += lds_invalid
    return True


def install(monkeypatch, ops_module, module):
    me = sys.modules[__name__]
    del CALLS[:]
    for name in ("supported", "comoments_update"):
        monkeypatch.setattr(ops_module, name, getattr(me, name))
    monkeypatch.setattr(module, "_on_device", lambda x: True)
