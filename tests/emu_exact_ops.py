"""TEST DOUBLE for the four launchers of the window-streamed exact guidance (climate2weather_amd.ops: guidance_delta, window_gather_list,
window_cotangent_list, window_grad_fold_list), layered over tests/emu_ops.py (which stays as it is).

Each function restates the contract of its C-ABI entry point (include/c2w_hip.h) in torch, on CPU tensors: the lists are read from the int32
tensors the route uploads, rows are rounded through the compute type, and the fold adds the windows in ascending list order.
"""
from __future__ import annotations

import torch

import emu_ops
from emu_ops import TD, _rows


def guidance_delta(x, eps, yobs, stdv, delta, nobs, F, H, W, s_step, t_step, mu, sigma, gamma):
    """delta = (what emu_ops.guidance leaves on the observed frames) - eps; eps itself is not written."""
    L = x.numel() // (F * H * W)
    X = x.reshape(-1)[: L * F * H * W].view(L, F, H, W)
    Ev = eps.reshape(-1)[: L * F * H * W].view(L, F, H, W)
    x0 = (X[::t_step][:nobs] - sigma * Ev[::t_step][:nobs]) / mu
    err = yobs.reshape(nobs, F, H // s_step, W // s_step) - torch.nn.functional.avg_pool2d(x0, s_step)
    gam = gamma.reshape(1, F, 1, 1) if isinstance(gamma, torch.Tensor) else gamma
    var = stdv.reshape(1, F, 1, 1) ** 2 + gam * (sigma / mu) ** 2
    g = (err / var).repeat_interleave(s_step, 2).repeat_interleave(s_step, 3) / (s_step * s_step)
    delta.reshape(-1)[: nobs * F * H * W] = (-(sigma * g / mu)).reshape(-1)


def window_gather_list(x, y, first, n, F, HW, k, ldc, dtype):
    w = 2 * k + 1
    X = x.reshape(-1)
    Y = _rows(y, n * HW, ldc)
    Y[:] = 0
    for j in range(n):
        f0 = int(first[j])
        win = X[f0 * F * HW: (f0 + w) * F * HW].view(w * F, HW)
        Y[j * HW:(j + 1) * HW, : w * F] = win.t().to(TD[dtype])


def window_cotangent_list(delta, dy, first, kind, n, L, F, HW, k, t_step, nobs, ldc, dtype):
    w = 2 * k + 1
    D = delta.reshape(-1, nobs, F, HW)
    Y = _rows(dy, n * HW, ldc)
    Y[:] = 0
    for j in range(n):
        m, i0 = divmod(int(first[j]), L)
        kd = int(kind[j])
        for tau in range(w):
            kept = tau == k or (tau < k and kd & 1) or (tau > k and kd & 2)
            frame = i0 + tau
            if kept and frame % t_step == 0 and frame // t_step < nobs:
                Y[j * HW:(j + 1) * HW, tau * F:(tau + 1) * F] = D[m, frame // t_step].t().to(TD[dtype])


def window_grad_fold_list(dx, out, first, n, l0, nl, F, HW, k, scale):
    w = 2 * k + 1
    DX = dx.reshape(-1)[: n * w * F * HW].view(n, w, F * HW)
    O = out.reshape(-1, F * HW)
    for l in range(l0, l0 + nl):
        s = None
        for j in range(n):  # ascending list order, one owner per element
            d = l - int(first[j])
            if 0 <= d < w:
                s = DX[j, d].clone() if s is None else s + DX[j, d]
        if s is not None:
            O[l] += scale * s


NAMES = ["guidance_delta", "window_gather_list", "window_cotangent_list", "window_grad_fold_list"]


def install(monkeypatch, target):
    """emu_ops.install, then the streamed-exact-guidance launchers on top."""
    import sys
    emu_ops.install(monkeypatch, target)
    me = sys.modules[__name__]
    for name in NAMES:
        monkeypatch.setattr(target, name, getattr(me, name))
