"""TEST DOUBLE for the spectrum launcher (climate2weather_amd.ops: rapsd, rapsd_supported), on CPU tensors.

It restates the contract of c2w_rapsd (include/c2w_hip.h) in NumPy float64, by the route the kernel takes: the mean off, the half
spectrum kv = 0 .. N/2 - 1 with kv = 0 counted once and kv >= 1 twice, the Nyquist row and column never formed, bin 0 from the field's own
sum.  Unsupported shapes answer False and write nothing.  ``install`` also makes spectra.rapsd treat CPU tensors as device tensors, so the
host code takes the launcher's branch.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

SIZES = (8, 16, 32, 64, 128)
CALLS = []  # (n_fields, H, W) of every call that reached the double


def rapsd_supported(H, W):
    return H == W and H in SIZES


def half_plane_weights(N):
    """(N, N/2, N/2) float64: weight of cell (u, kv) in bin k -- 1 (kv = 0) or 2 (kv >= 1) over the bin's weight, by the integer rule"""
    u = np.arange(N)
    ku = np.where(u < N // 2, u, u - N)
    kv = np.arange(N // 2)
    s = ku[:, None] ** 2 + kv[None, :] ** 2
    w = np.where(kv == 0, 1.0, 2.0)[None, :] * np.ones((N, 1))
    w[N // 2, :] = 0.0  # ku = -N/2
    out = np.zeros((N, N // 2, N // 2))
    for k in range(N // 2):
        m = (s > k * k - k) & (s <= k * k + k) if k else s == 0
        out[:, :, k] = np.where(m, w, 0.0)
        out[:, :, k] /= out[:, :, k].sum()
    return out


def rapsd(x, spec, n_fields, H, W):
    CALLS.append((int(n_fields), int(H), int(W)))
    if not rapsd_supported(H, W):
        return False
    assert x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() % 16 == 0 and spec.dtype == torch.float32 and spec.is_contiguous()
    a = x.reshape(-1)[:n_fields * H * W].reshape(n_fields, H, W).numpy().astype(np.float64)
    total = a.sum(axis=(-2, -1))
    z = np.fft.fft2(a - total[:, None, None] / (H * W))[:, :, :W // 2]
    s = np.einsum("fuv,uvk->fk", np.abs(z) ** 2 / (H * W), half_plane_weights(H))
    s[:, 0] = total * total / (H * W)
    spec.reshape(-1)[:n_fields * (H // 2)] = torch.from_numpy(s.astype(np.float32)).reshape(-1)
    return True


def install(monkeypatch, ops_module, spectra_module):
    me = sys.modules[__name__]
    del CALLS[:]
    for name in ("rapsd", "rapsd_supported"):
        monkeypatch.setattr(ops_module, name, getattr(me, name))
    monkeypatch.setattr(spectra_module, "_on_device", lambda x: True)
