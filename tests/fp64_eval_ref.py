"""Float64 reference of the validation tail (c2w_sq_err_levels / c2w_sq_err_levels_noise, csrc/evaluation.hip) with element-wise
bounds, built from tests/fp64_ref.py's error model (C_ACC, _acc; that file stays as it is).  Never calls climate2weather_amd.ops.

Every (image, channel) sum s[b][c] of HW positive terms (y - eps)^2 is bounded by fp64_ref._acc(s, sum of squared terms, HW, chain) with
``chain`` the longest run of dependent fp32 additions a term can go through, read off the launch geometry:

  tiled kernel (sq_err_image_channel_kernel; HW % 4 == 0 and the LDS tile fits):
      2 (the four pixels of a thread: (a + b) + (c + d)) + tps (one add per tile of the slab onto the thread's slot)
      + 4 (xor tree over the 16 lanes of a channel) + nslab (the slabs, in order, in loss_level_table_kernel)
  any-shape kernel (sq_err_image_channel_any_kernel): tps * 64 (one thread walks the slab's pixels) + nslab

A table entry is the sum, in DOUBLE, of its bin's images: its bound is the sum of their bounds plus 2^-53 per addition of the running
value.  per_image[b] adds the image's C channel sums in fp32: ceil(C / 256) per thread + 6 (wave tree) + 3 (the four waves).
"""
from __future__ import annotations

import numpy as np
import torch

import fp64_ref
from fp64_ref import D, V, _acc, _nchw, _rows

EV_PT, EV_TARGET_BLOCKS, EV_LDS_MAX = 64, 2048, 64 * 1024  # csrc/evaluation.hip


def slab_plan(B, HW):
    ntile = -(-HW // EV_PT)
    want = max(1, min(ntile, -(-EV_TARGET_BLOCKS // B)))
    tps = -(-ntile // want)
    return ntile, tps, -(-ntile // tps)


def scratch_bytes(B, C, HW):
    return B * slab_plan(B, HW)[2] * C * 4


def tiled(C, HW, ldc):
    return (ldc * (EV_PT + 1) + C * (EV_PT // 4)) * 4 <= EV_LDS_MAX and HW % 4 == 0


def chain(B, C, HW, ldc):
    _, tps, nslab = slab_plan(B, HW)
    return (2 + tps + 4 + nslab) if tiled(C, HW, ldc) else (tps * EV_PT + nslab)


def level_bins(t, K):
    """min(K - 1, floor(t * K)) with ONE fp32 multiply, t clamped to [0, 1] (include/c2w_hip.h)"""
    tt = np.clip(np.asarray(t, dtype=np.float32).reshape(-1), np.float32(0), np.float32(1))
    return np.minimum(np.floor((tt * np.float32(K)).astype(np.float32)).astype(np.int64), K - 1)


def terms(y, eps, B, C, HW, ldc):
    """(B, HW, C) float64: the exact squared errors of the real channels"""
    d = _rows(y, B * HW, ldc)[:, :C].to(D) - _nchw(eps, B, C, HW)
    return (d * d).view(B, HW, C)


def image_channel(y, eps, B, C, HW, ldc):
    """V of the (B, C) per-image, per-channel sums"""
    t2 = terms(y, eps, B, C, HW, ldc)
    s, sq = t2.sum(1), (t2 * t2).sum(1)
    return V(s, _acc(s, sq, HW, chain(B, C, HW, ldc)))


def sq_err_levels(y, eps, t, B, C, HW, ldc, K, calls=1):
    """dict(table=V (K, C), count (K,) int64, per_image=V (B,)) after ``calls`` identical calls onto a zeroed table"""
    ic = image_channel(y, eps, B, C, HW, ldc)
    bins = torch.from_numpy(level_bins(t.detach().cpu().numpy(), K)).to(ic.v.device)
    tv = torch.zeros((K, C), dtype=D, device=ic.v.device).index_add_(0, bins, ic.v)
    te = torch.zeros((K, C), dtype=D, device=ic.v.device).index_add_(0, bins, ic.e)
    count = torch.bincount(bins, minlength=K)
    te = te + 2.0 ** -53 * (count.to(D) * calls)[:, None] * tv.abs() * calls
    S, SQ = ic.v.sum(1), (ic.v * ic.v).sum(1)
    pe = ic.e.sum(1) + _acc(S, SQ, C, -(-C // 256) + 6 + 3)
    return dict(table=V(tv * calls, te * calls), count=count * calls, per_image=V(S, pe))


def slab_term(y, eps, B, C, HW, ldc, b, slab):
    """(C,) float64: what slab ``slab`` of image ``b`` contributes to its image's channel sums (the planted defect: a slab dropped)"""
    _, tps, _ = slab_plan(B, HW)
    lo, hi = min(HW, slab * tps * EV_PT), min(HW, (slab + 1) * tps * EV_PT)
    return terms(y, eps, B, C, HW, ldc)[b, lo:hi].sum(0)


def padding_term(y, B, C, HW, ldc, b):
    """float64 scalar: sum over image b's pixels of y[.][C]^2 (the planted defect: a padding channel read as if its eps were 0)"""
    return (_rows(y, B * HW, ldc)[b * HW:(b + 1) * HW, C].to(D) ** 2).sum()


assert_within, assert_rejects, report = fp64_ref.assert_within, fp64_ref.assert_rejects, fp64_ref.report
