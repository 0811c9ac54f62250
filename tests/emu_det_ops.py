"""TEST DOUBLE for the deterministic mode of climate2weather_amd.ops, layered over tests/emu_ops.py (which stays as it is).

What the HIP library does under C2W_CONV_DETERMINISTIC / in the c2w_*_det launchers is restated with the same contract: the
contribution a launch would add with atomics is STORED into slots of the caller's scratch (whose previous contents are poison here),
and a "reduce" adds the slots onto the destination in ascending order.  A missing or short scratch raises.  LOG records every
reduce, so a test can see that each site of a training step went through one.
"""
from __future__ import annotations

import torch

import emu_ops

NSLOT = 3
LOG = []  # (site, floats per slot) of every reduce issued


class ScratchError(RuntimeError):
    pass


def _through_scratch(site, dst, n, scratch, need_bytes, launch):
    """``launch()`` accumulates its contribution into dst.reshape(-1)[:n]; route it through NSLOT slots of ``scratch`` instead."""
    if scratch is None or scratch.numel() * scratch.element_size() < need_bytes:
        raise ScratchError(f"{site}: scratch missing or shorter than {need_bytes} bytes")
    flat = dst.reshape(-1)[:n]
    before = flat.clone()
    flat.zero_()
    launch()
    contrib = flat.clone()
    s = scratch.reshape(-1)
    s.fill_(float("nan"))  # nothing may depend on what the scratch held before
    s[0:n] = contrib * 0.5
    s[n:2 * n] = contrib * 0.25
    s[2 * n:3 * n] = contrib - s[0:n] - s[n:2 * n]
    acc = s[0:n].clone()
    for k in range(1, NSLOT):  # ascending slot order
        acc += s[k * n:(k + 1) * n]
    flat.copy_(before + acc)
    s.fill_(float("nan"))  # contents are undefined after the call
    LOG.append((site, n))


def _dm_floats(npix, HW, C, ldm):
    return C if ldm == 0 else (npix // HW - 1) * ldm + C


def ln_backward_det_scratch_bytes(npix, HW, C, ldm):
    return NSLOT * _dm_floats(npix, HW, C, ldm) * 4


def colsum_det_scratch_bytes(rows, C):
    return NSLOT * C * 4


def loss_det_scratch_bytes():
    return NSLOT * 4


def conv_det_scratch_bytes(g, dtype, ln_ldm=None, loss=False):
    assert not loss, "emu_ops.conv_loss_supported() is False: nobody may size a fused-loss scratch here"
    assert ln_ldm is not None
    return ln_backward_det_scratch_bytes(g["B"] * g["Hout"] * g["Wout"], g["Hout"] * g["Wout"], g["Cout"], ln_ldm)


def conv_wgrad_workspace_bytes(g, dtype, deterministic=False):
    return NSLOT * g["Cout"] * 4 if deterministic else 0


def conv_wgrad_grouped_workspace_bytes(g, n, dtype, deterministic=False):
    return n * NSLOT * g["Cout"] * 4 if deterministic else 0


def ln_backward(dy, x, m, dres, dx, dm, npix, HW, C, ldm, eps, unbiased, dtype, det=None):
    def launch():
        emu_ops.ln_backward(dy, x, m, dres, dx, dm, npix, HW, C, ldm, eps, unbiased, dtype)
    if det is None or dm is None:
        return launch()
    _through_scratch("ln_backward", dm, _dm_floats(npix, HW, C, ldm), det, ln_backward_det_scratch_bytes(npix, HW, C, ldm), launch)


def colsum(a, out, rows, C, lda, dtype, det=None):
    def launch():
        emu_ops.colsum(a, out, rows, C, lda, dtype)
    if det is None:
        return launch()
    _through_scratch("colsum", out, C, det, colsum_det_scratch_bytes(rows, C), launch)


def mse_loss_grad(y, eps, dy, loss_sum, B, C, HW, ldc, gscale, dtype, scaler=None, det=None):
    def launch():
        emu_ops.mse_loss_grad(y, eps, dy, loss_sum, B, C, HW, ldc, gscale, dtype, scaler=scaler)
    if det is None:
        return launch()
    _through_scratch("mse_loss_grad", loss_sum, 1, det, loss_det_scratch_bytes(), launch)


def sq_err(y, eps, out, loss_sum, B, C, HW, ldc, dtype, det=None):
    res = []

    def launch():
        res.append(emu_ops.sq_err(y, eps, out, loss_sum, B, C, HW, ldc, dtype))
    if det is None or loss_sum is None:
        launch()
        return res[0]
    _through_scratch("sq_err", loss_sum, 1, det, loss_det_scratch_bytes(), launch)
    return res[0]


def conv_wgrad(x, dy, dw, g, dtype, dbias=None, workspace=None, deterministic=False):
    def launch():
        emu_ops.conv_wgrad(x, dy, dw, g, dtype, dbias=dbias, workspace=None)
    if not deterministic or dbias is None:
        return launch()
    _through_scratch("conv_wgrad", dbias, g["Cout"], workspace, conv_wgrad_workspace_bytes(g, dtype, True), launch)


def conv_wgrad_grouped(items, g, dtype, workspace=None, deterministic=False):
    if not deterministic:
        return emu_ops.conv_wgrad_grouped(items, g, dtype, workspace=None)
    need = conv_wgrad_grouped_workspace_bytes(g, len(items), dtype, True)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        raise ScratchError(f"conv_wgrad_grouped: workspace missing or shorter than {need} bytes")
    emu_ops.GROUPED_LAUNCHES.append((g["Hout"], len(items)))
    per = NSLOT * g["Cout"]
    for i, (x, dy, dw, db) in enumerate(items):
        conv_wgrad(x, dy, dw, g, dtype, dbias=db, workspace=workspace.reshape(-1)[i * per:(i + 1) * per], deterministic=True)


def conv(x, w, bias, y, g, dtype, det=None, **kw):
    ln = kw.get("ln")

    def launch():
        emu_ops.conv(x, w, bias, y, g, dtype, **kw)
    if det is None:
        return launch()
    assert ln is not None and ln.get("dm") is not None, "det scratch handed to a conv launch that reduces nothing"
    npix, HW = g["B"] * g["Hout"] * g["Wout"], g["Hout"] * g["Wout"]
    ldm = ln.get("ldm", 0)
    _through_scratch("conv_ln", ln["dm"], _dm_floats(npix, HW, g["Cout"], ldm), det, conv_det_scratch_bytes(g, dtype, ln_ldm=ldm), launch)


NEW_NAMES = ["ln_backward_det_scratch_bytes", "colsum_det_scratch_bytes", "loss_det_scratch_bytes", "conv_det_scratch_bytes"]
WRAPPED = ["conv_wgrad_workspace_bytes", "conv_wgrad_grouped_workspace_bytes", "ln_backward", "colsum", "mse_loss_grad", "sq_err", "conv_wgrad",
           "conv_wgrad_grouped", "conv"]


def install(monkeypatch, target):
    """emu_ops.install, then the deterministic-mode launchers on top."""
    import sys
    emu_ops.install(monkeypatch, target)
    me = sys.modules[__name__]
    for name in NEW_NAMES + WRAPPED:
        monkeypatch.setattr(target, name, getattr(me, name))
    monkeypatch.setattr(target, "new_workspace", lambda device, nbytes=0: torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=device))
    del LOG[:]
