"""TEST DOUBLE for the quantile-mapping launchers (climate2weather_amd.qmap_ops), on CPU tensors.

It restates the kernels of csrc/qmap.hip in NumPy with the maps of csrc/qmap_core.h written out again in Python -- the series-major
scratch of the gather, the monotone key with NaNs and padding at the top, the count as the first position that holds the top key, the
two ranks and numpy's _lerp operation by operation, the bisection for the last node <= x, the three branches of the mapping in float64
with no multiply fused with an add, one rounding to fp32 -- for every series at once.  Unsupported shapes answer False and write nothing.
``install`` also makes the biascorrect module treat CPU tensors as device tensors, so the host code takes the launcher's branch.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

CALLS = []  # (name, hw, K, max_len) of every call that reached a launcher

MAX_K, MAX_N, TOP = 128, 16384, np.uint32(0xFFFFFFFF)


def qmap_supported(hw, K, max_len):
    return hw >= 4 and hw % 4 == 0 and 2 <= K <= MAX_K and 0 <= max_len <= MAX_N


def qmap_scratch_bytes(rows, cells, Tu):
    if rows < 1 or cells < 1 or Tu < 1:
        return 0
    return (rows * cells * Tu * 4 + 15) // 16 * 16


def key_of(bits):
    """quantile_core.h: unsigned order of the key is the order of the values"""
    return bits ^ np.where(bits >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def bits_of(key):
    return key ^ np.where(key >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))


def sorted_keys(series):
    """series (..., n) fp32 -> (keys (..., n) uint32 ascending, NaNs as TOP at the end; nv (...,) the first position holding TOP)"""
    bits = np.ascontiguousarray(series).view(np.uint32)
    nan = (bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    keys = np.sort(np.where(nan, TOP, key_of(bits)), axis=-1)
    return keys, (keys != TOP).sum(axis=-1).astype(np.int64)


def nodes_of(keys, nv, n, levels, skipna):
    """quantile_core.h rank_of / lerp_of on the sorted keys: (..., K) float64"""
    with np.errstate(all="ignore"):
        pos = (nv - 1).astype(np.float64)[..., None] * levels      # (..., K)
        fl = np.floor(pos)
        last = np.maximum(nv - 1, 0)[..., None]
        lo = np.minimum(np.maximum(fl.astype(np.int64), 0), last)
        hi = np.minimum(lo + 1, last)
        if keys.shape[-1] == 0:
            return np.full(pos.shape, np.nan)
        a = bits_of(np.take_along_axis(keys, lo, -1)).view(np.float32).astype(np.float64)
        b = bits_of(np.take_along_axis(keys, hi, -1)).view(np.float32).astype(np.float64)
        t = pos - fl
        diff = b - a
        up, down = diff * t, diff * (1.0 - t)
        res = np.where(t >= 0.5, b - down, a + up)
    dead = (nv == 0) if skipna else (nv < n)
    return np.where(dead[..., None], np.nan, res)


def _lists(tidx, goff, G, Tu):
    tidx, goff = tidx.numpy(), goff.numpy()
    assert tidx.dtype == np.int32 and goff.dtype == np.int32 and tidx.shape == (Tu,) and goff.shape == (G + 1,)
    assert goff[0] == 0 and goff[G] == Tu and np.all(np.diff(goff) >= 0)
    return tidx, goff


def qmap_nodes(x, tidx, goff, levels, q, n_valid, scratch, n_rep, T, F, hw, Tu, G, K, max_len, skipna, c0, c1):
    CALLS.append(("nodes", int(hw), int(K), int(max_len)))
    if not qmap_supported(hw, K, max_len):
        return False
    assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() == n_rep * T * F * hw
    assert levels.dtype == torch.float64 and levels.numel() == K
    assert q.dtype == torch.float64 and q.is_contiguous() and q.numel() == n_rep * G * F * hw * K
    assert n_valid.dtype == torch.int64 and n_valid.is_contiguous() and n_valid.numel() == n_rep * G * F * hw
    assert 0 <= c0 < c1 <= hw and Tu <= T
    tidx, goff = _lists(tidx, goff, G, Tu)
    assert max_len == max(int(d) for d in np.diff(goff))
    need = qmap_scratch_bytes(n_rep * F, c1 - c0, Tu)
    assert need == 0 or (scratch is not None and scratch.dtype == torch.float32 and scratch.numel() * 4 >= need)
    xs = x.reshape(n_rep, T, F, hw).numpy()
    lv = levels.numpy()
    qv, nvv = q.view(n_rep, G, F, hw, K).numpy(), n_valid.view(n_rep, G, F, hw).numpy()
    # the gather: scratch[rep F + f][cell - c0][position]
    series = np.ascontiguousarray(np.moveaxis(xs[:, tidx, :, c0:c1], 1, -1))  # (n_rep, F, cells, Tu)
    if need:
        scratch.view(-1).numpy()[:series.size] = series.reshape(-1)
    for g in range(G):
        part = series[..., goff[g]:goff[g + 1]]
        keys, nv = sorted_keys(part)
        qv[:, g, :, c0:c1] = nodes_of(keys, nv, part.shape[-1], lv, skipna)
        nvv[:, g, :, c0:c1] = nv
    return True


def bisect(xq, x):
    """the nodes with xq <= x are [0, lo): the loop of qmap_core.h::map_one, for xq (..., K) and x (...,)"""
    K = xq.shape[-1]
    lo, hi = np.zeros(x.shape, np.int64), np.full(x.shape, K, np.int64)
    while np.any(lo < hi):
        active = lo < hi
        mid = (lo + hi) >> 1
        with np.errstate(invalid="ignore"):
            le = np.take_along_axis(xq, np.minimum(mid, K - 1)[..., None], -1)[..., 0] <= x
        lo, hi = np.where(active & le, mid + 1, lo), np.where(active & ~le, mid, hi)
    return lo


def map_values(x, xq, yq):
    """x (...,) fp32 through the tables xq, yq (..., K) float64 of every element: fp32"""
    K = xq.shape[-1]
    v = x.astype(np.float64)
    lo = bisect(xq, v)
    j = np.clip(lo - 1, 0, K - 2)[..., None]
    with np.errstate(all="ignore"):
        xj, xj1 = np.take_along_axis(xq, j, -1)[..., 0], np.take_along_axis(xq, j + 1, -1)[..., 0]
        yj, yj1 = np.take_along_axis(yq, j, -1)[..., 0], np.take_along_axis(yq, j + 1, -1)[..., 0]
        slope = (yj1 - yj) / (xj1 - xj)
        step = (v - xj) * slope
        inside = yj + step
        inside = np.where(inside > yj1, yj1, inside)
        below = v + (yq[..., 0] - xq[..., 0])
        above = v + (yq[..., -1] - xq[..., -1])
        return np.where(lo == 0, below, np.where(lo == K, above, inside)).astype(np.float32)


def qmap_apply(x, out, xq, yq, tidx, goff, n_rep, T, F, hw, Tu, G, K, max_len):
    CALLS.append(("apply", int(hw), int(K), int(max_len)))
    if not qmap_supported(hw, K, max_len):
        return False
    for t in (x, out):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0 and t.numel() == n_rep * T * F * hw
    for t in (xq, yq):
        assert t.dtype == torch.float64 and t.is_contiguous() and t.numel() == G * F * hw * K
    tidx, goff = _lists(tidx, goff, G, Tu)
    xs, res = x.reshape(n_rep, T, F, hw).numpy(), out.view(n_rep, T, F, hw).numpy()
    tx, ty = xq.view(G, F, hw, K).numpy(), yq.view(G, F, hw, K).numpy()
    for g in range(G):
        idx = tidx[goff[g]:goff[g + 1]]
        if len(idx) == 0:
            continue
        v = xs[:, idx].copy()  # (n_rep, n, F, hw)
        res[:, idx] = map_values(v, np.broadcast_to(tx[g], v.shape + (K,)), np.broadcast_to(ty[g], v.shape + (K,)))
    return True


def install(monkeypatch, ops_module, biascorrect_module):
    me = sys.modules[__name__]
    del CALLS[:]
    for name in ("qmap_supported", "qmap_scratch_bytes", "qmap_nodes", "qmap_apply"):
        monkeypatch.setattr(ops_module, name, getattr(me, name))
    monkeypatch.setattr(biascorrect_module, "_on_device", lambda x: True)
