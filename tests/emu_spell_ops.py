"""TEST DOUBLE for the event-spell launchers (climate2weather_amd.spell_ops), on CPU tensors.

It restates spell_update_kernel of csrc/spells.hip in NumPy with the maps of csrc/spells_core.h written out again in Python: the
threshold groups of 4, a workgroup per (row, variable, chunk of 1024 cells), the counters read from ``state`` and written back where
they were read, the walk over the planes in order -- an event that starts a run is an add to the workgroup's onset bins, a run that
ends an add to its histogram bins, nothing is closed at the block's end -- and then one add per non-zero bin to the accumulators, which
are NOT zeroed here.  Only the launch with ``k0 = 0`` counts the NaNs.  Unsupported arguments answer False and write nothing.
``install`` also makes the spells module treat CPU tensors as device tensors, so the host code takes the launcher's branch.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

CALLS = []  # (M, T, F, hw, K, max_duration, period, t0) of every call that reached the launcher

THREADS, CELLS, CHUNK, GROUP, MAX_K, MAX_LMAX, MAX_PERIOD, MAX_T = 256, 4, 1024, 4, 8, 256, 24, 1 << 20
LDS_INTS = GROUP * MAX_LMAX + GROUP * MAX_PERIOD + 1


def supported(hw, K, max_duration, period):
    return hw >= 4 and hw % 4 == 0 and 1 <= K <= MAX_K and 1 <= max_duration <= MAX_LMAX and 0 <= period <= MAX_PERIOD


def chunks(hw):
    return (hw + CHUNK - 1) // CHUNK


def groups(K):
    return [(k0, min(GROUP, K - k0)) for k0 in range(0, K, GROUP)]


def spell_update(x, y, thr, direction, state, hist, onsets, invalid, M, T, F, hw, K, max_duration, period, t0):
    CALLS.append((int(M), int(T), int(F), int(hw), int(K), int(max_duration), int(period), int(t0)))
    if not supported(hw, K, max_duration, period) or M < 1:
        return False
    for t in (x,) + (() if y is None else (y,)):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
    assert thr.dtype == torch.float32 and thr.is_contiguous() and direction.dtype == torch.int32 and direction.is_contiguous()
    D = M + (0 if y is None else 1)
    assert state.dtype == torch.int32 and state.is_contiguous() and state.numel() >= 4 * D * F * K * hw and state.data_ptr() % 16 == 0
    assert hist.dtype == torch.int64 and hist.is_contiguous() and hist.numel() >= D * F * K * max_duration
    assert invalid.dtype == torch.int64 and invalid.is_contiguous() and invalid.numel() >= D * F
    assert (onsets is None) == (period == 0) and 0 <= T <= MAX_T and t0 >= 0
    if period:
        assert onsets.dtype == torch.int64 and onsets.is_contiguous() and onsets.numel() >= D * F * K * period
    if T == 0:
        return True
    xs = x.reshape(M, T, F, hw).numpy()
    rows = xs if y is None else np.concatenate([y.reshape(1, T, F, hw).numpy(), xs])
    th, ab = thr.reshape(F, K).numpy(), direction.reshape(F, K).numpy() != 0
    st = state.reshape(-1).numpy()[:4 * D * F * K * hw].reshape(4, D, F, K, hw)       # views: written in place
    hs = hist.reshape(-1).numpy()[:D * F * K * max_duration].reshape(D, F, K, max_duration)
    on = None if onsets is None else onsets.reshape(-1).numpy()[:D * F * K * period].reshape(D, F, K, period)
    inv = invalid.reshape(-1).numpy()[:D * F].reshape(D, F)
    for k0, kn in groups(K):                                   # one launch each
        for d in range(D):
            for f in range(F):
                for c in range(chunks(hw)):
                    lo, hi = c * CHUNK, min(hw, (c + 1) * CHUNK)
                    lds_hist, lds_onsets, lds_invalid = np.zeros((GROUP, MAX_LMAX), np.int64), np.zeros((GROUP, MAX_PERIOD), np.int64), 0
                    reg = st[:, d, f, k0:k0 + kn, lo:hi].astype(np.int64)                # (4, kn, cells): the threads' registers
                    open_, longest, count, hours = reg[0], reg[1], reg[2], reg[3]
                    t_k, a_k = th[f, k0:k0 + kn, None], ab[f, k0:k0 + kn, None]
                    phase = t0 % period if period else 0
                    for t in range(T):
                        v = rows[d, t, f, lo:hi][None]
                        lds_invalid += int(np.isnan(v).sum())
                        with np.errstate(invalid="ignore"):
                            e = np.where(a_k, v >= t_k, v <= t_k)
                        if period:
                            lds_onsets[:kn, phase] += (e & (open_ == 0)).sum(axis=1)
                        ending = ~e & (open_ > 0)
                        for k in range(kn):
                            lds_hist[k] += np.bincount(np.minimum(open_[k][ending[k]], max_duration) - 1, minlength=MAX_LMAX)
                        count += ending
                        longest[:] = np.where(ending, np.maximum(longest, open_), longest)
                        hours += e
                        open_[:] = np.where(e, open_ + 1, 0)
                        phase = phase + 1 if phase + 1 < period else 0
                    st[:, d, f, k0:k0 + kn, lo:hi] = reg                                 # stored where they were loaded
                    hs[d, f, k0:k0 + kn] += lds_hist[:kn, :max_duration]
                    assert int(lds_hist[:, max_duration:].sum()) == 0
                    if period:
                        on[d, f, k0:k0 + kn] += lds_onsets[:kn, :period]
                    if k0 == 0:
                        inv[d, f] += lds_invalid
    return True


def install(monkeypatch, ops_module, spells_module):
    me = sys.modules[__name__]
    del CALLS[:]
    for name in ("supported", "spell_update"):
        monkeypatch.setattr(ops_module, name, getattr(me, name))
    monkeypatch.setattr(spells_module, "_on_device", lambda x: True)
