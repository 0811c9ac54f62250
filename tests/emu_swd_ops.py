"""TEST DOUBLE for the sliced-Wasserstein launchers (climate2weather_amd.ops: swd_supported, swd_project, swd_project_pair, swd_distance),
on CPU tensors.

It restates the contracts of c2w_swd_project and c2w_swd_distance (include/c2w_hip.h) in NumPy: x^ = (x - shift[f]) * scale[f] formed in
fp32 on the value, the products and sums in float64, proj[rep][f][p][t] stored as fp32; the columns sorted, differences and squares in
double, a NaN in either column written as NaN.  Unsupported shapes answer False and write nothing.  ``install`` also makes
wasserstein.sliced_wasserstein treat CPU tensors as device tensors, so the host code takes the launcher's branch.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

CALLS = []  # ("project", n_rep, T, F, d, P) / ("distance", n_rep, F, P, T) of every call that reached the double


def swd_supported(d, P, T):
    return d % 64 == 0 and 64 <= d <= 65536 and 1 <= P <= 128 and 1 <= T <= 16384


def swd_project(x, theta, shift, scale, proj, n_rep, T, F, d, P):
    CALLS.append(("project", int(n_rep), int(T), int(F), int(d), int(P)))
    if not (d % 64 == 0 and 64 <= d <= 65536 and 1 <= P <= 128):
        return False
    for t in (x, theta):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
    for t in (shift, scale):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == F
    assert proj.dtype == torch.float32 and proj.is_contiguous() and proj.numel() >= n_rep * F * P * T and theta.numel() == P * d
    xs = x.reshape(-1)[:n_rep * T * F * d].reshape(n_rep, T, F, d).numpy()
    xh = (xs - shift.numpy()[:, None]) * scale.numpy()[:, None]
    assert xh.dtype == np.float32
    # (n_rep, T, F, P); a sum along the last axis, not a matrix product: a row's value must not depend on the batch around it
    p = (xh.astype(np.float64)[..., None, :] * theta.numpy().astype(np.float64)).sum(axis=-1)
    proj.reshape(-1)[:n_rep * F * P * T] = torch.from_numpy(np.ascontiguousarray(p.transpose(0, 2, 3, 1)).astype(np.float32).reshape(-1))
    return True


def swd_project_pair(x, y, theta, shift, scale, proj_x, proj_y, n_rep, T, F, d, P):
    return swd_project(y, theta, shift, scale, proj_y, 1, T, F, d, P) and swd_project(x, theta, shift, scale, proj_x, n_rep, T, F, d, P)


def swd_distance(proj_x, proj_y, out, n_rep, F, P, T):
    CALLS.append(("distance", int(n_rep), int(F), int(P), int(T)))
    if not 1 <= T <= 16384:
        return False
    for t in (proj_x, proj_y):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert out.dtype == torch.float64 and out.is_contiguous()
    a = proj_x.reshape(-1)[:n_rep * F * P * T].reshape(n_rep, F, P, T).numpy().astype(np.float64)
    b = proj_y.reshape(-1)[:F * P * T].reshape(1, F, P, T).numpy().astype(np.float64)
    bad = np.isnan(a).any(axis=-1) | np.isnan(b).any(axis=-1)
    with np.errstate(invalid="ignore"):
        D = ((np.sort(a, axis=-1) - np.sort(b, axis=-1)) ** 2).mean(axis=-1)
    D[bad] = np.nan
    out.reshape(-1)[:n_rep * F * P] = torch.from_numpy(D.reshape(-1))
    return True


def install(monkeypatch, ops_module, swd_module):
    me = sys.modules[__name__]
    del CALLS[:]
    for name in ("swd_supported", "swd_project", "swd_project_pair", "swd_distance"):
        monkeypatch.setattr(ops_module, name, getattr(me, name))
    monkeypatch.setattr(swd_module, "_on_device", lambda x: True)
