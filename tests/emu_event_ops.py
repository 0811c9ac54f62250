"""TEST DOUBLE for the event-verification launchers (climate2weather_amd.event_ops), on CPU tensors.

It restates the two kernels of csrc/events.hip in NumPy with the index maps of csrc/events_core.h written out again in Python: for the
joint table the chunks of 4096 cells, the bins of a workgroup and bin (0, 0) obtained as the valid cells less the other bins; for the
FSS sums the tiles of 64 x 64 cells, the halo of the call's largest radius (in x rounded up to a multiple of 4) clipped to the domain,
the summed-area table of the REGION with a zero row and column in front -- 16-bit for an indicator row, 32-bit for the member count
-- and the four corner reads clipped to the region.  Unsupported shapes answer False and write nothing.  ``install`` also makes the
events module treat CPU tensors as device tensors, so the host code takes the launcher's branch.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

CALLS = []  # ("counts", M, T, F, hw, K) / ("fss", M, T, F, H, W, K, radii) of every call that reached a launcher

THREADS, CHUNK, MAX_M, MAX_K, MAX_S, MAX_R, TILE, REGION = 256, 4096, 64, 8, 8, 16, 64, 96


def counts_supported(hw, M, K):
    return hw >= 4 and hw % 4 == 0 and 1 <= M <= MAX_M and 1 <= K <= MAX_K


def chunks(hw):
    return (hw + CHUNK - 1) // CHUNK


def fss_no_overflow(H, W, M, R):
    n = M * (2 * R + 1) ** 2
    return n * n <= ((1 << 62) - 1) // (H * W)


def fss_supported(H, W, M, K, radii):
    radii = list(radii)
    if H < 4 or W < 4 or W % 4 != 0 or H * W > (1 << 20) or not 1 <= M <= MAX_M or not 1 <= K <= MAX_K:
        return False
    if not 1 <= len(radii) <= MAX_S or any(r < 0 or r > MAX_R for r in radii):
        return False
    return fss_no_overflow(H, W, M, max(radii))


def tiles_y(H):
    return (H + TILE - 1) // TILE


def tiles_x(W):
    return (W + TILE - 1) // TILE


def geo_of(H, W, R, tile):
    """(ty0, tx0, th, tw, y0, x0, rh, rw): the tile and the region staged for it"""
    Rx = (R + 3) // 4 * 4
    ty0, tx0 = tile // tiles_x(W) * TILE, tile % tiles_x(W) * TILE
    th, tw = min(TILE, H - ty0), min(TILE, W - tx0)
    y0, x0 = max(0, ty0 - R), max(0, tx0 - Rx)
    y1, x1 = min(H, ty0 + th + R), min(W, tx0 + tw + Rx)
    return ty0, tx0, th, tw, y0, x0, y1 - y0, x1 - x0


def _indicator(v, thr, above):
    with np.errstate(invalid="ignore"):
        return np.where(above, v >= thr, v <= thr)


def _check_inputs(x, y, thr, direction):
    for t in (x, y):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
    assert thr.dtype == torch.float32 and thr.is_contiguous() and direction.dtype == torch.int32 and direction.is_contiguous()


def event_counts(x, y, thr, direction, counts, invalid, M, T, F, hw, K):
    CALLS.append(("counts", int(M), int(T), int(F), int(hw), int(K)))
    if not counts_supported(hw, M, K):
        return False
    _check_inputs(x, y, thr, direction)
    nb = 2 * (M + 1)
    assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() >= T * F * K * nb
    assert invalid.dtype == torch.int64 and invalid.is_contiguous() and invalid.numel() >= T * F
    xs, ys = x.reshape(M, T * F, hw).numpy(), y.reshape(T * F, hw).numpy()
    th, ab = thr.reshape(F, K).numpy(), direction.reshape(F, K).numpy() != 0
    out, inv = np.zeros((T * F, K, nb), np.int64), np.zeros((T * F,), np.int64)  # the launcher zeroes both
    for plane in range(T * F):
        f = plane % F
        for c in range(chunks(hw)):
            lo, hi = c * CHUNK, min(hw, (c + 1) * CHUNK)
            g, s = ys[plane, lo:hi], xs[:, plane, lo:hi]
            nan = np.isnan(g) | np.isnan(s).any(axis=0)
            n_valid = int((~nan).sum())
            for k in range(K):
                o = _indicator(g, th[f, k], ab[f, k]).astype(np.int64)
                j = _indicator(s, th[f, k], ab[f, k]).sum(axis=0)
                b = (o * (M + 1) + j)[~nan]
                hist = np.bincount(b[b != 0], minlength=nb).astype(np.int64)  # bin (0, 0) is never added ...
                hist[0] = n_valid - hist[1:].sum()                              # ... it is what is left of the valid cells
                out[plane, k] += hist
            inv[plane] += int(nan.sum())
    counts.reshape(-1).numpy()[:out.size] = out.reshape(-1)
    invalid.reshape(-1).numpy()[:inv.size] = inv
    return True


def _region_table(e, dtype):
    """e (..., rh, rw) small integers -> the (..., 97, 97) table of the region in the kernel's entry type, zero row and column in front"""
    sat = np.zeros(e.shape[:-2] + (REGION + 1, REGION + 1), dtype)
    rh, rw = e.shape[-2:]
    sat[..., 1:rh + 1, 1:rw + 1] = e
    sat[..., 1:rh + 1, 1:rw + 1] = np.cumsum(sat[..., 1:rh + 1, 1:rw + 1], axis=-1, dtype=dtype)  # the scan along the rows
    sat[..., 1:rh + 1, 1:rw + 1] = np.cumsum(sat[..., 1:rh + 1, 1:rw + 1], axis=-2, dtype=dtype)  # then along the columns
    return sat


def _windows(sat, geo, r):
    """(..., th, tw) int64: the window sums of the tile's cells from four reads at corners clipped to the region"""
    ty0, tx0, th, tw, y0, x0, rh, rw = geo
    ry, rx = ty0 - y0 + np.arange(th), tx0 - x0 + np.arange(tw)
    a0, a1 = np.maximum(ry - r, 0)[:, None], np.minimum(ry + r + 1, rh)[:, None]
    b0, b1 = np.maximum(rx - r, 0)[None, :], np.minimum(rx + r + 1, rw)[None, :]
    s = sat.astype(np.int64)
    return s[..., a1, b1] - s[..., a0, b1] - s[..., a1, b0] + s[..., a0, b0]


def fss_sums(x, y, thr, direction, sums, radii, M, T, F, H, W, K):
    radii = [int(r) for r in radii]
    CALLS.append(("fss", int(M), int(T), int(F), int(H), int(W), int(K), tuple(radii)))
    if not fss_supported(H, W, M, K, radii):
        return False
    _check_inputs(x, y, thr, direction)
    S, R = len(radii), max(radii)
    assert sums.dtype == torch.int64 and sums.is_contiguous() and sums.numel() >= T * F * K * S * (M + 2) * 2
    xs, ys = x.reshape(M, T * F, H, W).numpy(), y.reshape(T * F, H, W).numpy()
    th, ab = thr.reshape(F, K).numpy(), direction.reshape(F, K).numpy() != 0
    out = np.zeros((T * F, K, S, M + 2, 2), np.int64)  # the launcher zeroes it
    for plane in range(T * F):
        f = plane % F
        for k in range(K):
            for tile in range(tiles_y(H) * tiles_x(W)):
                geo = geo_of(H, W, R, tile)
                ty0, tx0, th_, tw, y0, x0, rh, rw = geo
                assert rh <= REGION and rw <= REGION and x0 % 4 == 0 and rw % 4 == 0
                e0 = _indicator(ys[plane, y0:y0 + rh, x0:x0 + rw], th[f, k], ab[f, k])
                em = _indicator(xs[:, plane, y0:y0 + rh, x0:x0 + rw], th[f, k], ab[f, k])
                cnt = em.sum(axis=0).astype(np.uint8)  # the member counts ride as bytes
                sat0, satm, sate = _region_table(e0, np.uint16), _region_table(em, np.uint16), _region_table(cnt, np.uint32)
                for s, r in enumerate(radii):
                    n0 = _windows(sat0, geo, r)
                    n = np.concatenate([n0[None], _windows(satm, geo, r), _windows(sate, geo, r)[None]])
                    out[plane, k, s, :, 0] += (n * n).sum(axis=(-1, -2))
                    out[plane, k, s, :, 1] += (n * n0).sum(axis=(-1, -2))
    sums.reshape(-1).numpy()[:out.size] = out.reshape(-1)
    return True


def install(monkeypatch, ops_module, events_module):
    me = sys.modules[__name__]
    del CALLS[:]
    for name in ("counts_supported", "event_counts", "fss_supported", "fss_sums"):
        monkeypatch.setattr(ops_module, name, getattr(me, name))
    monkeypatch.setattr(events_module, "_on_device", lambda x: True)
