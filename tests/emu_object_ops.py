"""TEST DOUBLE for the event-object launchers (climate2weather_amd.object_ops), on CPU tensors.

It restates object_tables_kernel of csrc/objects.hip in NumPy and plain Python with the maps of csrc/objects_maps.h written out again:
a workgroup per plane ``b = ((d T + t) F + f) K + k``; the runs along a row take the index of their first cell; the runs of adjacent
rows (and diagonals at connectivity 8) are united by a union-find that links the larger root to the smaller; one flattening pass; a run
adds its length once to its root's area, its sums and box to its root's list slot where the root's rank in index order is under
``max_objects``; then the plane's row, its list (unused slots ``-1, 0 ...``) and, from the ``k = 0`` workgroup, its NaN count are
STORED, and the area bins ADDED to an accumulator that is not zeroed here.  Unsupported arguments answer False and write nothing.
``install`` also makes the objects module treat CPU tensors as device tensors, so the host code takes the launcher's branch.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

CALLS = []  # (M, T, F, H, W, K, connectivity, max_objects) of every call that reached the launcher

MAX_CELLS, MAX_K, MAX_OBJECTS = 16384, 8, 256


def supported(H, W, K, connectivity, max_objects):
    return H >= 1 and W >= 4 and W % 4 == 0 and H * W <= MAX_CELLS and 1 <= K <= MAX_K and connectivity in (4, 8) and 0 <= max_objects <= MAX_OBJECTS


def _find(parent, a):
    while parent[a] < a:
        a = parent[a]
    return a


def _plane(e, connectivity, max_objects):
    """e (H, W) bool -> (row of 6, {bin: objects}, list (max_objects, 8))"""
    H, W = e.shape
    runs = []                                   # (i, j0, j1) with j1 exclusive, in index order
    for i in range(H):
        edge = np.flatnonzero(np.diff(np.concatenate([[0], e[i].astype(np.int8), [0]])))
        runs += [(i, int(a), int(b)) for a, b in zip(edge[0::2], edge[1::2])]
    head = [i * W + a for i, a, _ in runs]
    parent = {h: h for h in head}
    by_row = {}
    for n, (i, a, b) in enumerate(runs):
        by_row.setdefault(i, []).append(n)
    reach = 1 if connectivity == 8 else 0
    for n, (i, a, b) in enumerate(runs):
        for m in by_row.get(i - 1, []):
            _, c, d = runs[m]
            if c < b + reach and a - reach < d:                       # the runs overlap, or touch at a corner
                ra, rb = _find(parent, head[n]), _find(parent, head[m])
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)                 # the larger root to the smaller
    root = [_find(parent, h) for h in head]                           # the flattening pass
    roots = sorted(set(root))
    rank = {r: n for n, r in enumerate(roots)}                        # the scan in index order: the label order of the list
    area, border = dict.fromkeys(roots, 0), dict.fromkeys(roots, False)
    lst = np.zeros((max_objects, 8), np.int64)
    lst[:, 0], lst[:, 4], lst[:, 5], lst[:, 6], lst[:, 7] = -1, 1 << 31, -1, 1 << 31, -1
    row = np.zeros(6, np.int64)
    for (i, a, b), r in zip(runs, root):
        n = b - a
        area[r] += n                                                  # once a run, from its first cell
        border[r] |= i == 0 or i == H - 1 or a == 0 or b == W
        sj = n * (2 * a + n - 1) // 2
        row[1] += n
        row[4] += i * n
        row[5] += sj
        if rank[r] < max_objects:
            s = lst[rank[r]]
            s[2] += i * n
            s[3] += sj
            s[4], s[5], s[6], s[7] = min(s[4], i), max(s[5], i), min(s[6], a), max(s[7], b - 1)
    bins = {}
    for r in roots:
        bins[area[r].bit_length() - 1] = bins.get(area[r].bit_length() - 1, 0) + 1
        row[2] = max(row[2], area[r])
        row[3] += border[r]
        if rank[r] < max_objects:
            lst[rank[r], 0], lst[rank[r], 1] = r, area[r]
    row[0] = len(roots)
    lst[len(roots):] = [-1, 0, 0, 0, 0, 0, 0, 0]
    return row, bins, lst


def object_tables(x, y, thr, direction, plane, area_hist, objects, invalid, M, T, F, H, W, K, connectivity, max_objects):
    CALLS.append((int(M), int(T), int(F), int(H), int(W), int(K), int(connectivity), int(max_objects)))
    if not supported(H, W, K, connectivity, max_objects) or M < 1:
        return False
    hw = H * W
    for t in (x,) + (() if y is None else (y,)):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
    assert thr.dtype == torch.float32 and thr.is_contiguous() and direction.dtype == torch.int32 and direction.is_contiguous()
    D, B = M + (0 if y is None else 1), int(hw).bit_length()
    assert plane.dtype == torch.int64 and plane.is_contiguous() and plane.numel() >= D * T * F * K * 6
    assert area_hist.dtype == torch.int64 and area_hist.is_contiguous() and area_hist.numel() >= D * F * K * B
    assert invalid.dtype == torch.int64 and invalid.is_contiguous() and invalid.numel() >= D * T * F
    assert (objects is None) == (max_objects == 0) and T >= 0
    if max_objects:
        assert objects.dtype == torch.int32 and objects.is_contiguous() and objects.numel() >= D * T * F * K * max_objects * 8
    if T == 0:
        return True
    xs = x.reshape(M, T, F, hw).numpy()
    rows = xs if y is None else np.concatenate([y.reshape(1, T, F, hw).numpy(), xs])
    th, ab = thr.reshape(F, K).numpy(), direction.reshape(F, K).numpy() != 0
    pl = plane.reshape(-1).numpy()[:D * T * F * K * 6].reshape(D, T, F, K, 6)          # views: written in place
    hs = area_hist.reshape(-1).numpy()[:D * F * K * B].reshape(D, F, K, B)
    inv = invalid.reshape(-1).numpy()[:D * T * F].reshape(D, T, F)
    ob = None if objects is None else objects.reshape(-1).numpy()[:D * T * F * K * max_objects * 8].reshape(D, T, F, K, max_objects, 8)
    for b in range(D * T * F * K):                                                     # one workgroup each
        k, f, t, d = b % K, b // K % F, b // K // F % T, b // K // F // T
        v = rows[d, t, f]
        with np.errstate(invalid="ignore"):
            e = (v >= th[f, k]) if ab[f, k] else (v <= th[f, k])
        row, bins, lst = _plane(e.reshape(H, W), connectivity, max_objects)
        pl[d, t, f, k] = row
        for bin_, n in bins.items():
            hs[d, f, k, bin_] += n
        if ob is not None:
            ob[d, t, f, k] = lst
        if k == 0:
            inv[d, t, f] = int(np.isnan(v).sum())
    return True


def install(monkeypatch, ops_module, objects_module):
    me = sys.modules[__name__]
    del CALLS[:]
    for name in ("supported", "object_tables"):
        monkeypatch.setattr(ops_module, name, getattr(me, name))
    monkeypatch.setattr(objects_module, "_on_device", lambda x: True)
