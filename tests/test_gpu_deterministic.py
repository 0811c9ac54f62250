"""The deterministic mode on the GPU (include/c2w_hip.h: C2W_CONV_DETERMINISTIC, the c2w_*_det launchers; Engine.deterministic).

Per site -- every launch that sums with fp32 atomics by default --
  (a) twenty launches on fixed operands give the same bits, alone and beside a memory-bound kernel on a second stream;
  (b) the reduced value meets the float64 bound tests/fp64_ref.py gives the default path for that reduction (the fixed-order sums
      have shorter chains of dependent additions than the atomics the bounds were written for);
  (c) every other output of the launch is bit-identical to the default mode's;
  (d) a missing or short scratch is refused (C2W_ERR_BAD_ARG), never replaced by atomics.
Then whole steps: all 228 gradient tensors and the loss of identical steps, the module path, fresh processes, and the default mode
against the mode at the sites that do not reduce.
"""
import math
import os
import subprocess
import sys

import pytest
import torch

import fp64_ref as R
from climate2weather_amd import _lib, ops
from test_gpu_kernels import CONV_CASES, GROUP_CASES, _out_hw

pytestmark = pytest.mark.gpu

F32, BF16, F16 = ops.DTYPE_F32, ops.DTYPE_BF16, ops.DTYPE_F16
TD = ops.TORCH_DTYPE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = dict(embedding_dim=512, hidden_blocks=[3] * 5, hidden_channels=[128, 128, 256, 384, 512], kernel_size=3, padding_mode="zeros",
               attention_levels=[4])
_BIG = {}


def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _knobs_follow_the_environment():
    yield
    ops.knobs_reload()


def rnd(shape, dt, seed, scale=1.0):
    g = torch.Generator(device=dev()).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=dev()) * scale).to(TD[dt])


def scratch(nbytes):
    return torch.full((max(nbytes // 4, 4),), float("nan"), dtype=torch.float32, device=dev())  # poison: nothing may read what it did not write


def launches_equal(run, dests, n=20):
    """(a): ``run()`` accumulates onto ``dests`` (restored to their initial values before every launch); 2 x n launches, the second
    half beside a memory-bound kernel on another stream.  Returns the first launch's results."""
    if "big" not in _BIG:
        _BIG["big"], _BIG["side"] = torch.empty(32 << 20, dtype=torch.float32, device=dev()).normal_(), torch.cuda.Stream()
    big, side = _BIG["big"], _BIG["side"]
    init = [d.clone() for d in dests]
    first = None
    for phase in (0, 1):
        for i in range(n):
            for d, d0 in zip(dests, init):
                d.copy_(d0)
            if phase == 1 and i % 4 == 0:
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    big.mul_(1.0001)
            run()
            cur = [d.clone() for d in dests]
            if first is None:
                first = cur
            else:
                for k, (a, b) in enumerate(zip(cur, first)):
                    assert torch.equal(a, b), f"launch {i} ({'beside a stream' if phase else 'alone'}): output {k} differs from the first launch"
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return first


def refused(call):
    with pytest.raises(_lib.C2wError, match="bad argument"):
        call()
    torch.cuda.synchronize()


def geom(B, Hin, Win, Cin, Hout, Wout, Cout, ldy, wrows, mode):
    return dict(B=B, Hin=Hin, Win=Win, Cin=Cin, Hout=Hout, Wout=Wout, Cout=Cout, ldy=ldy, wrows=wrows, mode=mode)


# ------------------------------------------------------------------------------------------------ weight-gradient bias sums
WG_CASES = [c for c in CONV_CASES if c[0] != ops.CONV_TS2] + [
    (ops.CONV_S1, 24, 16, 16, 128, 128, 128, 128),  # 48 K tiles over 48 splits (patch kernel)
    (ops.CONV_S1, 8, 32, 32, 128, 128, 65, 128),    # the output conv's narrow-M form (65 rows) with a split
    (ops.CONV_S1, 16, 8, 8, 128, 128, 128, 128),    # 8x8 images in pairs, split
    (ops.CONV_S2, 8, 32, 32, 64, 128, 128, 128),    # gather kernel, split
    (ops.CONV_1X1, 640, 1, 1, 128, 384, 384, 384),  # 1x1 (gather), split
]


@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("case,gather", [(c, False) for c in WG_CASES] + [(c, True) for c in WG_CASES if c[0] == ops.CONV_S1])  # (only 3x3 stride-1 has two kernels)
def test_wgrad_bias_gradient(case, dt, gather, monkeypatch):
    mode, B, Hin, Win, Cin, Cout, wrows, ldy = case
    if gather:
        monkeypatch.setenv("C2W_FORCE_GATHER", "1")
        ops.knobs_reload()
    taps = 1 if mode == ops.CONV_1X1 else 9
    Hout, Wout = _out_hw(mode, Hin, Win)
    g = geom(B, Hin, Win, Cin, Hout, Wout, wrows, ldy, wrows, mode)
    x, dy = rnd((B * Hin * Win, Cin), dt, 1), rnd((B * Hout * Wout, ldy), dt, 2)
    nw = wrows * taps * Cin
    dw = rnd((nw + 64,), F32, 3, 0.1)
    db = rnd((wrows + 8,), F32, 4)
    dw0, db0 = dw.clone(), db.clone()
    need = ops.conv_wgrad_workspace_bytes(g, dt, deterministic=True)
    plain = ops.conv_wgrad_workspace_bytes(g, dt)
    assert need >= plain and (need > plain) == (plain > 0)  # bias rows ride behind the partial tiles of a split launch
    ws = scratch(need)
    # default mode with the same workspace: the reference of (c)
    dw_def, db_def = dw0.clone(), db0.clone()
    ops.conv_wgrad(x, dy, dw_def, g, dt, dbias=db_def, workspace=ws)
    ws.fill_(float("nan"))
    first = launches_equal(lambda: ops.conv_wgrad(x, dy, dw, g, dt, dbias=db, workspace=ws, deterministic=True), [dw, db])
    assert torch.equal(first[0], dw_def), "dw differs from the default mode's"
    rw, rb = R.wgrad(x, dy, g)
    what = f"deterministic wgrad bias {case} dt={dt} gather={gather}"
    R.report(what, R.assert_within(first[1][:wrows], R.accumulated(db0[:wrows], rb), what=what))
    R.assert_within(db_def[:wrows], R.accumulated(db0[:wrows], rb), what=what + " (default mode)")
    assert torch.equal(first[1][wrows:], db0[wrows:]) and torch.equal(first[0][nw:], dw0[nw:])  # nothing written past the tensors
    if need > 0:
        refused(lambda: ops.conv_wgrad(x, dy, dw, g, dt, dbias=db, workspace=None, deterministic=True))
        refused(lambda: ops.conv_wgrad(x, dy, dw, g, dt, dbias=db, workspace=ws[: need // 4 - 4], deterministic=True))
        refused(lambda: ops.conv_wgrad(x, dy, dw, g, dt, dbias=db, workspace=ws[: plain // 4], deterministic=True))  # the default mode's size
        assert torch.equal(dw, first[0]) and torch.equal(db, first[1])  # a refused call writes nothing


def test_wgrad_atomics_knob_is_refused_in_deterministic_mode(monkeypatch):
    mode, B, Hin, Win, Cin, Cout, wrows, ldy = CONV_CASES[0]
    g = geom(B, Hin, Win, Cin, Hin, Win, wrows, ldy, wrows, mode)
    x, dy = rnd((B * Hin * Win, Cin), BF16, 1), rnd((B * Hin * Win, ldy), BF16, 2)
    dw, db = torch.zeros(wrows * 9 * Cin, device=dev()), torch.zeros(wrows, device=dev())
    ws = scratch(ops.conv_wgrad_workspace_bytes(g, BF16, deterministic=True))
    monkeypatch.setenv("C2W_WGRAD_ATOMICS", "1")
    ops.knobs_reload()
    ops.conv_wgrad(x, dy, dw, g, BF16, dbias=db, workspace=ws)  # the default mode takes the knob
    refused(lambda: ops.conv_wgrad(x, dy, dw, g, BF16, dbias=db, workspace=ws, deterministic=True))


@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("case", GROUP_CASES)
def test_grouped_wgrad_bias_gradients(case, dt):
    mode, B, Hin, Win, Cin, Cout, n = case
    if dt == F32:
        Cin, Cout = Cin // 2 if Cin > 64 else Cin, Cout // 2  # fp32 tiles are half as wide: same number of tiles
    Hout, Wout = _out_hw(mode, Hin, Win)
    g = geom(B, Hin, Win, Cin, Hout, Wout, Cout, Cout, Cout, mode)
    assert ops.conv_wgrad_grouped_supported(g, n, dt)
    taps = 1 if mode == ops.CONV_1X1 else 9
    xs = [rnd((B * Hin * Win, Cin), dt, 10 + i) for i in range(n)]
    dys = [rnd((B * Hout * Wout, Cout), dt, 40 + i) for i in range(n)]
    dws = [rnd((Cout * taps * Cin,), F32, 70 + i, 0.1) for i in range(n)]
    dbs = [rnd((Cout + 8,), F32, 100 + i) for i in range(n)]
    dw0, db0 = [t.clone() for t in dws], [t.clone() for t in dbs]
    items = lambda W, Bs: [(xs[i], dys[i], W[i], Bs[i] if i % 3 != 1 else None) for i in range(n)]  # some layers without a bias
    need = ops.conv_wgrad_grouped_workspace_bytes(g, n, dt, deterministic=True)
    plain = ops.conv_wgrad_grouped_workspace_bytes(g, n, dt)
    assert need >= plain and (need > plain) == (plain > 0)
    ws = scratch(need)
    dw_def, db_def = [t.clone() for t in dw0], [t.clone() for t in db0]
    ops.conv_wgrad_grouped(items(dw_def, db_def), g, dt, workspace=ws)
    ws.fill_(float("nan"))
    first = launches_equal(lambda: ops.conv_wgrad_grouped(items(dws, dbs), g, dt, workspace=ws, deterministic=True), dws + dbs)
    for i in range(n):
        assert torch.equal(first[i], dw_def[i]), f"layer {i}: dw differs from the default mode's"
        if i % 3 == 1:
            assert torch.equal(first[n + i], db0[i])
            continue
        _, rb = R.wgrad(xs[i], dys[i], g)
        what = f"deterministic grouped wgrad bias {case} dt={dt} layer {i}"
        R.report(what, R.assert_within(first[n + i][:Cout], R.accumulated(db0[i][:Cout], rb), what=what))
        assert torch.equal(first[n + i][Cout:], db0[i][Cout:])
    if need > 0:
        refused(lambda: ops.conv_wgrad_grouped(items(dws, dbs), g, dt, workspace=ws[: need // 4 - 4], deterministic=True))
        refused(lambda: ops.conv_wgrad_grouped(items(dws, dbs), g, dt, workspace=None, deterministic=True))


# ------------------------------------------------------------------------------------------------------ pointwise sites
LN_CASES = [
    # (B, HW, C, per-image rows)
    (2, 256, 384, True),     # level 3 of the default network: one chunk per image
    (3, 1000, 64, True),     # chunks that do not divide the image, a ragged last chunk
    (2, 4096, 128, True),    # 256 chunks per image: 16 threads share an output in the reduce
    (8, 4096, 128, False),   # one shared row, 2048 slots: 256 threads share an output
    (5, 64, 512, False),     # one shared row, 5 slots: one thread per output
]


@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("shape", LN_CASES)
def test_ln_backward_modulation_gradient(shape, dt):
    B, HW, C, per_image = shape
    npix, ldm = B * HW, (C + 64) if per_image else 0
    x, dy, dres = rnd((npix, C), dt, 1), rnd((npix, C), dt, 2), rnd((npix, C), dt, 3)
    m = rnd((B if per_image else 1, C + 64), F32, 4)
    dm = rnd((B if per_image else 1, C + 64), F32, 5)
    dm0 = dm.clone()
    mm, dmm = m.view(-1)[32:], dm.view(-1)[32:]
    dx_def, dm_def = torch.empty_like(x), dm0.clone()
    ops.ln_backward(dy, x, mm, dres, dx_def, dm_def.view(-1)[32:], npix, HW, C, ldm, 1e-5, True, dt)
    need = ops.ln_backward_det_scratch_bytes(npix, HW, C, ldm)
    assert need > 0
    ws = scratch(need)
    dx = torch.empty_like(x)
    first = launches_equal(lambda: ops.ln_backward(dy, x, mm, dres, dx, dmm, npix, HW, C, ldm, 1e-5, True, dt, det=ws), [dm, dx])
    assert torch.equal(first[1], dx_def), "dx differs from the default mode's"
    _, rdm = R.ln_backward(dy, x, mm, dres, npix, HW, C, ldm, 1e-5, True, dt)
    what = f"deterministic ln_backward dm {shape} dt={dt}"
    R.report(what, R.assert_within(first[0][:, 32:32 + C], R.accumulated(dm0[:, 32:32 + C], rdm), what=what))
    keep = torch.ones_like(dm0, dtype=torch.bool)
    keep[:, 32:32 + C] = False
    assert torch.equal(first[0][keep], dm0[keep])  # nothing written outside the modulation rows
    refused(lambda: ops.ln_backward(dy, x, mm, dres, dx, dmm, npix, HW, C, ldm, 1e-5, True, dt, det=ws[: need // 4 - 1]))
    ops.ln_backward(dy, x, mm, dres, dx, None, npix, HW, C, ldm, 1e-5, True, dt, det=ws[:4])  # no dm: nothing to reduce, no scratch read
    assert torch.equal(dx, dx_def)


@pytest.mark.parametrize("dt", [F32, BF16, F16])
def test_loss_sums_and_colsum(dt):
    """mse_loss_grad (+ the device-resident scale), mse_loss_grad_noise, sq_err (memory and regenerated noise) and colsum.  Shapes: more
    tiles than the grid has blocks (the grid-stride loop), fewer pixels than a tile, and the untiled kernel (rows too wide for LDS)."""
    need = ops.loss_det_scratch_bytes()
    ws = scratch(need)
    for (B, C, HW, ldc) in [(40, 52, 64 * 64, 64), (3, 6, 40, 8), (2, 200, 256, 256)]:
        tiled = ldc * 65 * 4 <= 64 * 1024
        y = rnd((B * HW, ldc), dt, 1)
        eps = rnd((B, C, HW), F32, 2)
        gs = 2.0 / (B * C * HW)
        scaler = torch.tensor([8.0, 0.0, 0.0, 0.0], device=dev())
        rsum = R.mse_loss_sum(y, eps, B, C, HW, ldc).view(1)
        for sc in (None, scaler):
            ls = torch.full((1,), 777.25, device=dev())
            dy, dy_def, ls_def = torch.empty_like(y), torch.empty_like(y), ls.clone()
            ops.mse_loss_grad(y, eps, dy_def, ls_def, B, C, HW, ldc, gs, dt, scaler=sc)
            first = launches_equal(lambda: ops.mse_loss_grad(y, eps, dy, ls, B, C, HW, ldc, gs, dt, scaler=sc, det=ws), [ls, dy])
            assert torch.equal(first[1], dy_def), "dy differs from the default mode's"
            what = f"deterministic mse_loss_grad loss sum {(B, C, HW, ldc)} dt={dt} scaler={sc is not None}"
            R.report(what, R.assert_within(first[0], R.accumulated(torch.full((1,), 777.25, device=dev()), rsum), what=what))
        refused(lambda: ops.mse_loss_grad(y, eps, dy, ls, B, C, HW, ldc, gs, dt, det=ws[: need // 4 - 1]))
        if not tiled:
            continue
        seed = 0x1234567
        e2 = torch.empty(B * C * HW, device=dev())
        ops.philox_normal(e2, e2.numel(), seed)
        rsum2 = R.mse_loss_sum(y, e2, B, C, HW, ldc).view(1)
        ls = torch.full((1,), -3.5, device=dev())
        ls0 = ls.clone()
        dy, dy_def, ls_def = torch.empty_like(y), torch.empty_like(y), ls.clone()
        assert ops.mse_loss_grad_noise(y, seed, dy_def, ls_def, B, C, HW, ldc, gs, dt)
        first = launches_equal(lambda: ops.mse_loss_grad_noise(y, seed, dy, ls, B, C, HW, ldc, gs, dt, det=ws), [ls, dy])
        assert torch.equal(first[1], dy_def)
        what = f"deterministic mse_loss_grad_noise loss sum {(B, C, HW, ldc)} dt={dt}"
        R.report(what, R.assert_within(first[0], R.accumulated(ls0, rsum2), what=what))
        refused(lambda: ops.mse_loss_grad_noise(y, seed, dy, ls, B, C, HW, ldc, gs, dt, det=ws[: need // 4 - 1]))
        if HW % 4:
            continue
        for src, ref in ((eps, rsum), (seed, rsum2)):
            out, out_def = torch.empty(B * C * HW, device=dev()), torch.empty(B * C * HW, device=dev())
            assert ops.sq_err(y, src, out_def, ls_def, B, C, HW, ldc, dt)
            ls.copy_(ls0)
            first = launches_equal(lambda: ops.sq_err(y, src, out, ls, B, C, HW, ldc, dt, det=ws), [ls, out])
            assert torch.equal(first[1], out_def), "sq_err's tensor differs from the default mode's"
            what = f"deterministic sq_err loss sum {(B, C, HW, ldc)} dt={dt} regenerated={isinstance(src, int)}"
            R.report(what, R.assert_within(first[0], R.accumulated(ls0, R.sq_err_sum(y, src if not isinstance(src, int) else e2, B, C, HW, ldc).view(1)), what=what))
            refused(lambda: ops.sq_err(y, src, out, ls, B, C, HW, ldc, dt, det=ws[: need // 4 - 1]))
    for rows, C in [(70000, 64), (5000, 2112), (3, 8)]:  # 35 / 3 / 1 row blocks; 2112 channels: more than one 256-vector slice of the row
        a = rnd((rows, C + 8), dt, 3)
        out = rnd((C + 8,), F32, 4)
        out0 = out.clone()
        need_c = ops.colsum_det_scratch_bytes(rows, C)
        wc = scratch(need_c)
        first = launches_equal(lambda: ops.colsum(a, out, rows, C, C + 8, dt, det=wc), [out])
        what = f"deterministic colsum {rows}x{C} dt={dt}"
        R.report(what, R.assert_within(first[0][:C], R.accumulated(out0[:C], R.colsum(a, rows, C, C + 8, dt)), what=what))
        assert torch.equal(first[0][C:], out0[C:])
        refused(lambda: ops.colsum(a, out, rows, C, C + 8, dt, det=wc[: need_c // 4 - 1]))


# ------------------------------------------------------------------------------------------------- fused conv epilogues
@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("per_image", [True, False])
@pytest.mark.parametrize("kernel", ["8x16 eight waves", "8x16 four waves", "16x16", "16x16 stored statistics"])
def test_fused_layernorm_backward_modulation_gradient(kernel, per_image, dt, monkeypatch):
    B, H, W, C = 3, 32, 48, 128
    if kernel == "8x16 four waves":
        monkeypatch.setenv("C2W_NO_HALF8", "1")
    monkeypatch.setenv("C2W_CONV_T3", "16" if kernel.startswith("16x16") else "0")
    ops.knobs_reload()
    g = geom(B, H, W, C, H, W, C, C, C, ops.CONV_S1)
    assert ops.conv_lnbwd_supported(g, dt)
    assert ops.conv_dispatch(g, dt) == (_lib.KERNEL_PATCH_16X16 if kernel.startswith("16x16") else _lib.KERNEL_PATCH_8X16)
    npix, ldm = B * H * W, (C + 64) if per_image else 0
    x = rnd((npix, C), dt, 1)
    w = rnd((C, 9, C), dt, 2, 1.0 / math.sqrt(9 * C))
    lnx, res = rnd((npix, C), dt, 7), rnd((npix, C), dt, 4)
    nrow = B if per_image else 1
    m = rnd((nrow, C + 64), F32, 6)
    dm = rnd((nrow, C + 64), F32, 5)
    dm0 = dm.clone()
    ln = dict(x=lnx, m=m.view(-1)[32:], ldm=ldm, eps=1e-5, unbiased=True)
    stored = kernel.endswith("stored statistics")
    if stored:  # what the forward's fused LayerNorm kept: the normalised rows and their 1/sigma
        hn, rstd = torch.empty_like(lnx), torch.empty(npix, device=dev())
        ops.ln_forward(lnx, m.view(-1)[32:], hn, npix, H * W, C, ldm, 1e-5, True, dt)
        u = lnx.float() + (m[:, 32:32 + C].repeat_interleave(H * W, 0) if per_image else m[:, 32:32 + C])
        rstd.copy_((u.var(dim=1, unbiased=True) + 1e-5).rsqrt())
        ln = dict(x=hn, rstd=rstd, m=None, ldm=ldm, eps=1e-5, unbiased=True)
    y, y_def, dm_def = torch.empty_like(x), torch.empty_like(x), dm0.clone()
    ops.conv(x, w, None, y_def, g, dt, res=res, ln=dict(ln, dm=dm_def.view(-1)[32:]))
    need = ops.conv_det_scratch_bytes(g, dt, ln_ldm=ldm)
    assert need > 0
    ws = scratch(need)
    first = launches_equal(lambda: ops.conv(x, w, None, y, g, dt, res=res, ln=dict(ln, dm=dm.view(-1)[32:]), det=ws), [dm, y])
    assert torch.equal(first[1], y_def), "the input gradient differs from the default mode's"
    what = f"deterministic fused LN backward dm {kernel} per_image={per_image} dt={dt}"
    if not stored:  # (tests/fp64_ref.py restates the recomputed-statistics form; the stored form is held against the default mode's below)
        ref = R.conv(x, w, g, dt, res=res, ln=ln)
        R.report(what, R.assert_within(first[0][:, 32:32 + C], R.accumulated(dm0[:, 32:32 + C], ref["dm"]), what=what))
    # the same fp32 terms in another order: far inside bf16's own rounding of the terms
    d, s = (first[0] - dm_def).abs().max().item(), (dm_def - dm0).abs().max().item()
    assert d <= 1e-4 * s, (what, d, s)
    keep = torch.ones_like(dm0, dtype=torch.bool)
    keep[:, 32:32 + C] = False
    assert torch.equal(first[0][keep], dm0[keep])
    refused(lambda: ops.conv(x, w, None, y, g, dt, res=res, ln=dict(ln, dm=dm.view(-1)[32:]), det=ws[: need // 4 - 1]))


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("C", [52, 65])
def test_fused_loss_sum_of_the_output_convolution(C, dt, monkeypatch):
    B, H = 3, 32
    monkeypatch.setenv("C2W_CONV_T3", "16")  # the fused loss lives in the 16x16-tile kernel; at this size it is taken on request only
    ops.knobs_reload()
    g = dict(geom(B, H, H, 128, H, H, 128, 128, C, ops.CONV_S1))
    assert ops.conv_loss_supported(g, dt)
    npix, lde = B * H * H, (C + 7) // 8 * 8
    x = rnd((npix, 128), dt, 1)
    w = rnd((C, 9, 128), dt, 2, 1.0 / math.sqrt(9 * 128))
    bias = rnd((C,), F32, 3)
    er = torch.zeros((npix, lde), dtype=torch.float16, device=dev())
    er[:, :C] = rnd((npix, C), F16, 9)
    y = torch.empty((npix, 128), dtype=TD[dt], device=dev())
    ops.conv(x, w, bias, y, g, dt)  # the prediction as stored: the fused kernel squares the same values
    ls = torch.full((1,), 1234.5, device=dev())
    ls0, ls_def = ls.clone(), ls.clone()
    dy, dy_def = torch.empty_like(y), torch.empty_like(y)
    scaler = torch.tensor([4.0, 0.0, 0.0, 0.0], device=dev())
    lf = dict(eps=er, lde=lde, gscale=2.0 / (B * C * H * H), C=C, scaler=scaler)
    ops.conv(x, w, bias, dy_def, g, dt, loss=dict(lf, sum=ls_def))
    need = ops.conv_det_scratch_bytes(g, dt, loss=True)
    assert need == B * (H // 16) * (H // 16) * 4
    ws = scratch(need)
    first = launches_equal(lambda: ops.conv(x, w, bias, dy, g, dt, loss=dict(lf, sum=ls), det=ws), [ls, dy])
    assert torch.equal(first[1], dy_def), "the loss gradient differs from the default mode's"
    ref = R.fused_loss_sum(y, er, C, lde, npix, B * (H // 16) * (H // 16))
    what = f"deterministic fused loss sum C={C} dt={dt}"
    R.report(what, R.assert_within(first[0], R.accumulated(ls0, ref.view(1)), what=what))
    refused(lambda: ops.conv(x, w, bias, dy, g, dt, loss=dict(lf, sum=ls), det=ws[: need // 4 - 1]))
    refused(lambda: _no_scratch_conv(x, w, bias, dy, g, dt, dict(lf, sum=ls)))  # the flag without any scratch


def _no_scratch_conv(x, w, bias, y, g, dt, loss):
    """ops.conv with C2W_CONV_DETERMINISTIC set and det_ws left NULL"""
    import ctypes
    a = ops._conv_args(x, w, bias, None, None, y, g, ops.ACT_NONE, ops.MUL_PLAIN)
    a.flags |= _lib.CONV_DETERMINISTIC
    a.loss_sum, a.loss_scaler = ops._p(loss["sum"]), ops._p(loss.get("scaler"))
    a.loss_eps, a.loss_lde, a.loss_gscale, a.loss_C = ops._p(loss["eps"]), int(loss["lde"]), float(loss["gscale"]), int(loss["C"])
    _lib.check(_lib.load().c2w_conv_forward(ctypes.byref(a), dt, 0, ops._stream()), "c2w_conv_forward")


# ------------------------------------------------------------------------------------------------------------- whole steps
def _grads(tr):
    return {n: tr.eng.flat_grad[off:off + int(torch.tensor(shape).prod())].clone() for n, (off, shape, _) in tr.eng.layout.views.items()}


def _identical_steps(B, C, H, precision, repeats, grad_stream, regenerated):
    """``repeats`` identical steps (same batch, t, noise and weights) with Trainer(deterministic=True): the loss and all 228 gradient
    tensors of every step equal the first step's bit for bit.  ``regenerated``: the step's own Philox noise from a fixed seed (the
    loss fused into the output convolution where that kernel exists) instead of a noise tensor (the separate loss tail)."""
    from climate2weather_amd.score import ScoreUNet
    from climate2weather_amd.training import Trainer
    torch.manual_seed(0)
    net = ScoreUNet(channels=C, spatial=2, activation=torch.nn.SiLU, **DEFAULT).cuda()
    gen = torch.Generator().manual_seed(128)
    x = (torch.randn(B, C, H, H, generator=gen) * 0.5 + 0.5).cuda()
    t = torch.rand(B, generator=gen).cuda()
    eps = None if regenerated else torch.randn(B, C, H, H, generator=gen).cuda()
    tr = Trainer(net, precision=precision, ema_rates=(), deterministic=True)
    tr.eng.use_grad_stream = grad_stream
    assert len(tr.eng.layout.views) == 228
    ref = None
    for r in range(repeats):
        tr.eng.flat_grad.zero_()
        tr.rng_cpu.manual_seed(77)  # the same noise seed every time
        loss = tr._forward_backward(x, t, eps, sync=False)
        torch.cuda.synchronize()
        assert math.isfinite(loss.item())
        cur = (loss.clone(), _grads(tr))
        if ref is None:
            ref = cur
            assert all(torch.isfinite(v).all() for v in cur[1].values())
            continue
        assert torch.equal(cur[0], ref[0]), f"round {r}: the loss changed between identical steps"
        changed = [n for n in cur[1] if not torch.equal(cur[1][n], ref[1][n])]
        assert not changed, f"round {r}: {len(changed)} of 228 gradient tensors changed between identical steps, first {changed[0]}"


@pytest.mark.parametrize("regenerated", [False, True])
@pytest.mark.parametrize("grad_stream", [False, True])
def test_identical_steps_reproduce_all_228_gradients_and_the_loss_at_the_bench_shape(grad_stream, regenerated):
    _identical_steps(128, 65, 128, "bf16", 12, grad_stream, regenerated)


@pytest.mark.parametrize("regenerated", [False, True])
@pytest.mark.parametrize("grad_stream", [False, True])
@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_identical_steps_reproduce_all_228_gradients_and_the_loss_at_two_windows(precision, grad_stream, regenerated):
    _identical_steps(2, 52, 128, precision, 50, grad_stream, regenerated)


def test_the_mode_changes_only_the_reduction_sites():
    """Mode off against mode on at the same knob settings: the forward output and the 70 conv weight gradients are bit-identical; what
    differs is the summation order at the reduction sites (biases, modulation gradients and what they feed, the loss)."""
    from climate2weather_amd.score import ScoreUNet
    from climate2weather_amd.training import Trainer
    out = {}
    for det in (False, True):
        torch.manual_seed(0)
        net = ScoreUNet(channels=52, spatial=2, activation=torch.nn.SiLU, **DEFAULT).cuda()
        gen = torch.Generator().manual_seed(7)
        x = (torch.randn(2, 52, 128, 128, generator=gen) * 0.5 + 0.5).cuda()
        t = torch.rand(2, generator=gen).cuda()
        eps = torch.randn(2, 52, 128, 128, generator=gen).cuda()
        tr = Trainer(net, precision="bf16", ema_rates=(), deterministic=det)
        with torch.no_grad():
            net.precision = "bf16"
            y = net(x, t).clone()
        tr.eng.flat_grad.zero_()
        loss = tr._forward_backward(x, t, eps, sync=False)
        torch.cuda.synchronize()
        out[det] = (y, float(loss), _grads(tr), {n for n, p in net.named_parameters() if p.dim() == 4})
    assert torch.equal(out[False][0], out[True][0])
    assert len(out[True][3]) == 70
    for n in out[True][3]:
        assert torch.equal(out[False][2][n], out[True][2][n]), n
    assert out[True][1] == pytest.approx(out[False][1], rel=1e-5)
    for n, gd in out[True][2].items():
        ga = out[False][2][n]
        assert (gd - ga).norm().item() <= 1e-3 * max(ga.norm().item(), 1e-30), n


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_module_path_gradients_are_bit_equal_over_repeats(precision):
    """ScoreUNet forward + loss.backward() through the autograd seam with the module's switch on: p.grad bit-equal over ten repeats of
    one backward and of two accumulated backward passes."""
    from climate2weather_amd.score import ScoreUNet
    cfg = dict(embedding_dim=64, hidden_channels=[128, 128], hidden_blocks=[1, 1], attention_levels=[1], kernel_size=3, padding_mode="zeros")
    torch.manual_seed(5)
    net = ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, **cfg).cuda()
    net.precision = precision
    net.deterministic = True
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(4, 6, 64, 64, generator=gen).cuda()
    t = torch.rand(4, generator=gen).cuda()
    eps = torch.randn(4, 6, 64, 64, generator=gen).cuda()
    assert net._get_engine().deterministic is True
    ref = {}
    for r in range(10):
        for passes in (1, 2):
            net.zero_grad(set_to_none=True)
            for _ in range(passes):
                loss = ((net(x, t) - eps) ** 2).mean()
                loss.backward()
            torch.cuda.synchronize()
            cur = {n: p.grad.clone() for n, p in net.named_parameters()}
            cur["loss"] = loss.detach().clone()
            if passes not in ref:
                ref[passes] = cur
                continue
            changed = [n for n in cur if not torch.equal(cur[n], ref[passes][n])]
            assert not changed, f"repeat {r}, {passes} backward pass(es): {changed[:3]} changed"
    assert not torch.equal(ref[1]["unet.heads.0.bias"], ref[2]["unet.heads.0.bias"])  # the second pass accumulated


_CHILD = r"""
import hashlib, sys
import torch
from climate2weather_amd.score import ScoreUNet
from climate2weather_amd.training import Trainer
prec = sys.argv[1]
cfg = dict(embedding_dim=64, hidden_channels=[64, 128], hidden_blocks=[1, 1], attention_levels=[1], kernel_size=3, padding_mode="zeros")
torch.manual_seed(11)
net = ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, **cfg).cuda()
tr = Trainer(net, lr=2e-3, precision=prec, ema_rates=[0.999], deterministic=True)
gen = torch.Generator().manual_seed(3)
base = torch.randn(8, 6, 32, 32, generator=gen) * 0.5 + 0.5
for s in range(60):
    x = (base + 0.05 * torch.randn(8, 6, 32, 32, generator=gen)).cuda()
    t = torch.rand(8, generator=gen).cuda()
    eps = torch.randn(8, 6, 32, 32, generator=gen).cuda()
    print(s, float(tr.step(x, t=t, eps=eps)).hex())
torch.cuda.synchronize()
for name, buf in (("parameters", tr.eng.flat), ("ema", tr.ema_flats[0])):
    print(name, hashlib.sha256(buf.detach().cpu().numpy().tobytes()).hexdigest())
"""


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_two_fresh_processes_train_to_the_same_bits(precision, tmp_path):
    """The 60-step toy training of test_gpu_host.py::test_bf16_and_fp16_training_track_fp32_training in two fresh processes: the same
    loss trajectory and the same parameter / EMA digests, byte for byte."""
    script = tmp_path / "train_child.py"
    script.write_text(_CHILD)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("C2W_DETERMINISTIC", None)
    outs = []
    for _ in range(2):
        p = subprocess.run([sys.executable, str(script), precision], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
        assert p.returncode == 0, p.stderr[-2000:]
        outs.append(p.stdout)
    assert len(outs[0].splitlines()) == 62 and "parameters" in outs[0]
    assert outs[0] == outs[1]
