"""TEST DOUBLE for the SSIM launcher (climate2weather_amd.ops: ssim, ssim_supported), on CPU tensors.

It restates the contract of c2w_ssim (include/c2w_hip.h) in NumPy float64: pair i is (x[i], y[i % n_truth]) with the data range of
slot i % n_truth, window sums over the windows inside the field (a cumulative-sum box filter, no library), out[i] a double, nothing
written past n_pairs.  Unsupported shapes and windows answer False and write nothing.  ``install`` also makes ssim.ssim treat CPU
tensors as device tensors, so the host code takes the launcher's branch.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

WINDOWS = (7, 11, 15)
CALLS = []  # (n_pairs, n_truth, H, W, win) of every call that reached the double


def ssim_supported(H, W, win):
    return H % 8 == 0 and W % 8 == 0 and 16 <= H <= 128 and 16 <= W <= 128 and win in WINDOWS


def box_mean(a, win):
    """(..., H, W) -> (..., H - win + 1, W - win + 1): the mean over every window inside the field"""
    c = np.cumsum(np.cumsum(np.pad(a, [(0, 0)] * (a.ndim - 2) + [(1, 0), (1, 0)]), axis=-2), axis=-1)
    return (c[..., win:, win:] - c[..., :-win, win:] - c[..., win:, :-win] + c[..., :-win, :-win]) / (win * win)


def ssim(x, y, data_range, out, n_pairs, n_truth, H, W, win):
    CALLS.append((int(n_pairs), int(n_truth), int(H), int(W), int(win)))
    if not ssim_supported(H, W, win):
        return False
    for t in (x, y):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
    assert data_range.dtype == torch.float32 and data_range.is_contiguous() and data_range.numel() == n_truth
    assert out.dtype == torch.float64 and out.is_contiguous() and n_truth >= 1
    idx = np.arange(n_pairs) % n_truth
    a = x.reshape(-1)[:n_pairs * H * W].reshape(n_pairs, H, W).numpy().astype(np.float64)
    b = y.reshape(-1)[:n_truth * H * W].reshape(n_truth, H, W).numpy().astype(np.float64)[idx]
    R = data_range.numpy().astype(np.float64)[idx][:, None, None]
    # the pivot changes nothing in exact arithmetic; it is here because the contract names it
    p = b.mean(axis=(-2, -1), keepdims=True)
    a, b = a - p, b - p
    cn = win * win / (win * win - 1.0)
    ua, ub = box_mean(a, win), box_mean(b, win)
    va, vb, vab = cn * (box_mean(a * a, win) - ua * ua), cn * (box_mean(b * b, win) - ub * ub), cn * (box_mean(a * b, win) - ua * ub)
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    ux, uy = ua + p, ub + p
    S = (1.0 - (ua - ub) ** 2 / (ux * ux + uy * uy + C1)) * ((2.0 * vab + C2) / (va + vb + C2))
    out.reshape(-1)[:n_pairs] = torch.from_numpy(S.mean(axis=(-2, -1)))
    return True


def install(monkeypatch, ops_module, ssim_module):
    me = sys.modules[__name__]
    del CALLS[:]
    for name in ("ssim", "ssim_supported"):
        monkeypatch.setattr(ops_module, name, getattr(me, name))
    monkeypatch.setattr(ssim_module, "_on_device", lambda x: True)
