"""TEST DOUBLE for the quantile launchers (climate2weather_amd.ops: quantile_supported, quantile_scratch_bytes, quantiles), on CPU
tensors.

It restates the two kernels of csrc/quantile.hip in NumPy with the maps of csrc/quantile_core.h written out again in Python: the
data-set and slab maps, the monotone key, the three counting passes over digits of 12 / 10 / 10 bits, the scan of a table in index
order that turns a rank into (bin, rank within the bin), the merge of equal prefixes into ascending slots, the table from the top 12
key bits to the first slot with these bits and the walk from there, and the interpolation in float64.  Unsupported shapes answer False
and write nothing.  ``install`` also makes the quantiles module treat CPU tensors as device tensors, so the host code takes the
launcher's branch.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

CALLS = []  # (n_rep, T, F, hw, Q, with_truth, skipna) of every call that reached the launcher

THREADS, LOCATE_THREADS, MAX_Q, BITS0, BITS1, BITS2, NONE, WG_PER_CU, LOADS = 1024, 128, 16, 12, 10, 10, 255, 8, 4
BINS0, BINS = 1 << BITS0, 1 << BITS1
CUS = 256  # what the launcher's CU count is on an MI355X


# ------------------------------------------------------------------------------------------------------------------ quantile_core.h, restated

def quantile_supported(hw, Q):
    return hw >= 4 and hw % 4 == 0 and 1 <= Q <= MAX_Q


def quantile_scratch_bytes(D, Q):
    if D < 0 or Q < 1 or Q > MAX_Q:
        return 0
    R = 2 * Q
    total = D * BINS0 * 8 + 2 * D * R * BINS * 8 + D * 8  # table0, table1, table2, nan: what the call zeroes
    total += D * R * 8 + D * R * 4 + D * R * 4              # res, pre, rslot
    total += (D * 4 + 7) // 8 * 8 + D * BINS0               # ns, tab
    return (total + 15) // 16 * 16


def count_lds_bytes(pass_, Q):
    return BINS0 * 4 + 16 if pass_ == 0 else 2 * Q * BINS * 4 + 2 * Q * 4 + BINS0 + 16


def slab_count(D, T, cus=CUS):
    return int(min(T, max(1, cus * WG_PER_CU // max(1, D))))


def slab_bounds(T, slabs, s):
    per = (T + slabs - 1) // slabs
    return min(T, s * per), min(T, (s + 1) * per)


def set_base(ds, n_x, T, F, hw):
    """(which buffer, the float offset of the data set's first value)"""
    if ds < n_x:
        return 0, ((ds // F) * T * F + ds % F) * hw
    return 1, (ds - n_x) * hw


def key_of(bits):
    return bits ^ np.where(bits >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def bits_of(key):
    return key ^ np.where(key >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))


def _locate(table, want):
    """the bin of a table, scanned in index order, that holds rank ``want``, and the rank within it"""
    cum = np.cumsum(table)
    b = int(min(np.searchsorted(cum, want, side="right"), table.size - 1))
    return b, int(want - (cum[b - 1] if b else 0))


def _slots(newpre, up):
    """ascending distinct prefixes, the slot of every rank, and tab: top 12 bits -> the first slot with them"""
    pre = sorted(set(newpre))
    rslot = [pre.index(p) for p in newpre]
    tab = np.full(BINS0, NONE, np.int64)
    for j in reversed(range(len(pre))):
        tab[pre[j] >> up] = j
    return np.array(pre, np.uint32), rslot, tab


def _slot_of(keys, pre, tab, shift):
    """the slot of every key (-1: none): tab, then the walk over the slots that share the top 12 bits"""
    up = 32 - BITS0 - shift
    top = (keys >> np.uint32(32 - BITS0)).astype(np.int64)
    j = tab[top]
    slot = np.full(keys.size, -1, np.int64)
    live = j != NONE
    for _ in range(len(pre)):
        jj = np.minimum(j, len(pre) - 1)
        live &= (j < len(pre)) & ((pre[jj] >> np.uint32(up)) == top)
        hit = live & (pre[jj] == (keys >> np.uint32(shift)))
        slot[hit] = j[hit]
        live &= ~hit
        j = j + 1
    return slot


def _one_data_set(keys_by_slab, n, q, skipna):
    """keys_by_slab: the non-NaN keys every workgroup of the data set loaded; -> (out (Q,), stats (Q, 2), nv)"""
    Q = len(q)
    nv = int(sum(k.size for k in keys_by_slab))
    if nv == 0 or (not skipna and nv < n):
        return np.full(Q, np.nan), np.full((Q, 2), np.nan, np.float32), nv
    # pass 0: every workgroup adds its LDS counters to the data set's table
    table = np.zeros(BINS0, np.int64)
    for k in keys_by_slab:
        table += np.bincount((k >> np.uint32(32 - BITS0)).astype(np.int64), minlength=BINS0)
    pos = np.float64(nv - 1) * np.asarray(q, np.float64)
    lo = np.clip(np.floor(pos).astype(np.int64), 0, nv - 1)
    want = [int(r) for j in range(Q) for r in (lo[j], min(lo[j] + 1, nv - 1))]
    found = [_locate(table, w) for w in want]
    newpre, res = [b for b, _ in found], [r for _, r in found]
    for pass_, shift in ((1, BITS1 + BITS2), (2, BITS2)):
        pre, rslot, tab = _slots(newpre, 0 if pass_ == 1 else BITS1)
        assert len(pre) <= 2 * Q and count_lds_bytes(pass_, Q) >= len(pre) * BINS * 4
        tables = np.zeros((len(pre), BINS), np.int64)
        for k in keys_by_slab:
            slot = _slot_of(k, pre, tab, shift)
            hit = slot >= 0
            digit = ((k[hit] >> np.uint32(shift - BITS1)) & np.uint32(BINS - 1)).astype(np.int64)
            tables += np.bincount(slot[hit] * BINS + digit, minlength=len(pre) * BINS).reshape(len(pre), BINS)
        found = [_locate(tables[s], w) for s, w in zip(rslot, res)]
        newpre = [(int(pre[s]) << BITS1) | b for s, (b, _) in zip(rslot, found)]
        res = [r for _, r in found]
    vals = bits_of(np.array(newpre, np.uint32)).view(np.float32).reshape(Q, 2)
    a, b = vals[:, 0].astype(np.float64), vals[:, 1].astype(np.float64)
    t = pos - np.floor(pos)
    with np.errstate(invalid="ignore"):
        diff = b - a
        out = np.where(t >= 0.5, b - diff * (1.0 - t), a + diff * t)
    return out, vals, nv


# ------------------------------------------------------------------------------------------------------------------ the launcher

def quantiles(x, y, q, skipna, scratch, out, stats, n_valid, n_rep, T, F, hw):
    Q = len(q)
    CALLS.append((int(n_rep), int(T), int(F), int(hw), Q, y is not None, bool(skipna)))
    if not quantile_supported(hw, Q):
        return False
    for t in (x, y):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0)
    assert all(0.0 <= float(v) <= 1.0 for v in q)
    n_x, n = n_rep * F, T * hw
    D = n_x + (F if y is not None else 0)
    assert scratch.numel() * scratch.element_size() >= quantile_scratch_bytes(D, Q) and scratch.data_ptr() % 16 == 0
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= D * Q
    assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() >= D * Q * 2
    assert n_valid.dtype == torch.int64 and n_valid.is_contiguous() and n_valid.numel() >= D
    bufs = (x.reshape(-1).numpy().view(np.uint32), None if y is None else y.reshape(-1).numpy().view(np.uint32))
    slabs = slab_count(D, T)
    o, s, c = out.reshape(-1).numpy(), stats.reshape(-1).numpy(), n_valid.reshape(-1).numpy()
    for ds in range(D):
        which, base = set_base(ds, n_x, T, F, hw)
        keys = []
        for sl in range(slabs):
            t0, t1 = slab_bounds(T, slabs, sl)
            at = (base + np.arange(t0, t1)[:, None] * (F * hw) + np.arange(hw)[None, :]).reshape(-1)
            bits = bufs[which][at]
            keys.append(key_of(bits[(bits & np.uint32(0x7FFFFFFF)) <= np.uint32(0x7F800000)]))
        row, st, nv = _one_data_set(keys, n, [float(v) for v in q], skipna)
        o[ds * Q:(ds + 1) * Q], s[ds * 2 * Q:(ds + 1) * 2 * Q], c[ds] = row, st.reshape(-1), nv
    return True


def install(monkeypatch, ops_module, quantiles_module):
    me = sys.modules[__name__]
    del CALLS[:]
    for name in ("quantile_supported", "quantile_scratch_bytes", "quantiles"):
        monkeypatch.setattr(ops_module, name, getattr(me, name))
    monkeypatch.setattr(quantiles_module, "_on_device", lambda x: True)
