"""TEST DOUBLE for the launchers of the held-out validation (climate2weather_amd.ops: sq_err_levels, sq_err_levels_scratch_bytes), layered
over tests/emu_ops.py (which stays as it is).

Each function restates the contract of its C-ABI entry point (include/c2w_hip.h) in torch / numpy, on CPU tensors.  The seed forms answer
"unsupported" (the library's own answer for shapes outside its regenerating kernels), so the host code takes its documented fall-back:
it materialises the stream with philox_normal -- restated here as Philox4x32-10 + Box-Muller in numpy (csrc/philox.h) -- and calls the
tensor forms.
"""
from __future__ import annotations

import numpy as np
import torch

import emu_ops
from emu_ops import _rows

from climate2weather_amd._lib import C2wError

EV_PT, EV_TARGET_BLOCKS = 64, 2048  # csrc/evaluation.hip


def slab_plan(B, HW):
    """(tiles per image, tiles per slab, slabs per image): csrc/evaluation.hip::slab_plan"""
    ntile = -(-HW // EV_PT)
    want = max(1, min(ntile, -(-EV_TARGET_BLOCKS // B)))
    tps = -(-ntile // want)
    return ntile, tps, -(-ntile // tps)


def sq_err_levels_scratch_bytes(B, C, HW):
    return B * slab_plan(B, HW)[2] * C * 4


def level_bins_f32(t, K):
    """the interface's bin rule, in numpy float32 (independent of evaluation.level_bins)"""
    tt = np.clip(np.asarray(t, dtype=np.float32).reshape(-1), np.float32(0), np.float32(1))
    prod = (tt * np.float32(K)).astype(np.float32)
    return np.minimum(np.floor(prod).astype(np.int64), K - 1)


def sq_err_levels(y, eps, t, table, count, per_image, B, C, HW, ldc, K, scratch, dtype):
    if isinstance(eps, int):
        return False  # C2W_ERR_UNSUPPORTED: the caller materialises the stream
    if scratch is None or scratch.numel() * scratch.element_size() < sq_err_levels_scratch_bytes(B, C, HW):
        raise C2wError("c2w_sq_err_levels failed: bad argument")
    assert table.dtype == torch.float64 and tuple(table.shape) == (K, C) and count.dtype == torch.int64 and count.numel() == K
    Y = _rows(y, B * HW, ldc)[:, :C].float().view(B, HW, C).permute(0, 2, 1)
    d = Y - eps.reshape(-1)[: B * C * HW].view(B, C, HW).float()
    s = (d * d).sum(-1)  # (B, C) fp32
    bins = torch.from_numpy(level_bins_f32(t.reshape(-1)[:B].numpy(), K))
    for b in range(B):  # images in ascending order, like the kernel
        table[int(bins[b])] += s[b].double()
        count[int(bins[b])] += 1
    if per_image is not None:
        per_image.reshape(-1)[:B] = s.sum(1)
    return True


def _philox_normal_np(n, seed):
    M32 = np.uint64(0xFFFFFFFF)
    blk = np.arange((n + 3) // 4, dtype=np.uint64)
    c0, c1 = blk & M32, blk >> np.uint64(32)
    c2, c3 = np.zeros_like(blk), np.zeros_like(blk)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    u = [((c >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0) for c in (c0, c1, c2, c3)]
    ra, rb = np.sqrt(np.float32(-2.0) * np.log(u[0])), np.sqrt(np.float32(-2.0) * np.log(u[2]))
    a, b = np.float32(6.28318530717958647692) * u[1], np.float32(6.28318530717958647692) * u[3]
    out = np.stack((ra * np.cos(a), ra * np.sin(a), rb * np.cos(b), rb * np.sin(b)), axis=1).astype(np.float32)
    return out.reshape(-1)[:n]


def philox_normal(out, n, seed):
    out.reshape(-1)[:n] = torch.from_numpy(_philox_normal_np(n, seed))


def nchw_to_nhwc_noise(x, seed, musig, y, B, C, HW, ldc, dtype):
    return False


def windows_to_nhwc_noise(data, img_off, seed, musig, y, B, C, HW, ldc, dtype):
    return False


NAMES = ["sq_err_levels_scratch_bytes", "sq_err_levels", "philox_normal", "nchw_to_nhwc_noise", "windows_to_nhwc_noise"]


def install(monkeypatch, target):
    """emu_ops.install, then the validation launchers on top."""
    import sys
    emu_ops.install(monkeypatch, target)
    me = sys.modules[__name__]
    for name in NAMES:
        monkeypatch.setattr(target, name, getattr(me, name))
