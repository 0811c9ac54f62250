"""CPU checks of tests/fp64_ref.py, the float64 reference and error bound of the GPU tier's element-wise checks:

  * the fp64 reference equals a direct loop formula on tiny shapes in all five conv modes (padding, wrows < Cout, kvalid);
  * the fp32 PyTorch restatement (tests/emu_ops.py), run here on the storage-typed operands, is within the bound for every family;
  * every planted defect of the GPU tier's power checks is rejected;
  * the bound is not vacuous: the restatement's observed err / bound is above 1e-3 on a small conv and a weight gradient.
"""
import math

import numpy as np
import pytest
import torch

import emu_ops as E
import fp64_ref as R

F32, BF16, F16 = E.DTYPE_F32, E.DTYPE_BF16, E.DTYPE_F16
TD = E.TD
MODES = [E.CONV_1X1, E.CONV_S1, E.CONV_S2, E.CONV_UP, E.CONV_TS2]


def rnd(shape, dt, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(TD[dt])


def geom(B, Hin, Win, Cin, Hout, Wout, Cout, ldy, wrows, mode):
    return dict(B=B, Hin=Hin, Win=Win, Cin=Cin, Hout=Hout, Wout=Wout, Cout=Cout, ldy=ldy, wrows=wrows, mode=mode)


def out_hw(mode, H, W):
    if mode == E.CONV_S2:
        return H // 2, W // 2
    if mode in (E.CONV_UP, E.CONV_TS2):
        return 2 * H, 2 * W
    return H, W


def direct_conv(X, Wt, mode, Hout, Wout):
    """X (B, H, W, Cin), Wt (rows, taps, Cin) as float64 numpy -> (B, Hout, Wout, rows), one output at a time"""
    B, H, W, Cin = X.shape
    rows = Wt.shape[0]
    out = np.zeros((B, Hout, Wout, rows))
    for b in range(B):
        for oh in range(Hout):
            for ow in range(Wout):
                acc = np.zeros(rows)
                if mode == E.CONV_1X1:
                    acc += Wt[:, 0] @ X[b, oh, ow]
                for kh in range(3) if mode != E.CONV_1X1 else ():
                    for kw in range(3):
                        if mode == E.CONV_S1:
                            ih, iw = oh + kh - 1, ow + kw - 1
                        elif mode == E.CONV_S2:
                            ih, iw = 2 * oh + kh - 1, 2 * ow + kw - 1
                        elif mode == E.CONV_UP:
                            uh, uw = oh + kh - 1, ow + kw - 1
                            if not (0 <= uh < 2 * H and 0 <= uw < 2 * W):
                                continue
                            ih, iw = uh // 2, uw // 2
                        else:  # transposed stride 2, padding 1: oh = 2 ih - 1 + kh
                            if (oh + 1 - kh) % 2 or (ow + 1 - kw) % 2:
                                continue
                            ih, iw = (oh + 1 - kh) // 2, (ow + 1 - kw) // 2
                        if 0 <= ih < H and 0 <= iw < W:
                            acc += Wt[:, kh * 3 + kw] @ X[b, ih, iw]
                out[b, oh, ow] = acc
    return out


@pytest.mark.parametrize("mode", MODES)
def test_fp64_conv_reference_equals_the_direct_loop(mode):
    B, H, W, Cin, Cout, wrows, kvalid = 2, 4, 6, 5, 8, 6, 3
    taps = 1 if mode == E.CONV_1X1 else 9
    Hout, Wout = out_hw(mode, H, W)
    g = geom(B, H, W, Cin, Hout, Wout, Cout, Cout, wrows, mode)
    x = rnd((B * H * W, Cin), F32, 1)
    x[:, kvalid:] = 0  # the kvalid promise
    w = rnd((wrows, taps, Cin), F32, 2)
    bias = rnd((wrows,), F32, 3)
    ref = R.conv_sum(x, w, g, bias=bias, kvalid=kvalid)
    d = direct_conv(x.double().view(B, H, W, Cin).numpy(), w.double().numpy(), mode, Hout, Wout) + bias.double().numpy()
    got = ref.v.view(B, Hout, Wout, Cout).numpy()
    np.testing.assert_allclose(got[..., :wrows], d, rtol=1e-12, atol=1e-12)
    assert (got[..., wrows:] == 0).all() and (ref.e.view(B, Hout, Wout, Cout)[..., wrows:] == 0).all()
    # weight gradient: the same loop is the adjoint -- dW = sum over pixels of dy * patch
    dy = rnd((B * Hout * Wout, Cout), F32, 4)
    dW, db = R.wgrad(x, dy, geom(B, H, W, Cin, Hout, Wout, Cout, Cout, Cout, mode)) if mode != E.CONV_TS2 else (None, None)
    if dW is not None:
        Xn, Gn = x.double().view(B, H, W, Cin).numpy(), dy.double().view(B, Hout, Wout, Cout).numpy()
        want = np.zeros((Cout, taps, Cin))
        for t in range(taps):
            for ci in range(Cin):
                unit = np.zeros((1, taps, Cin))
                unit[0, t, ci] = 1
                want[:, t, ci] = (direct_conv(Xn, unit, mode, Hout, Wout)[..., 0:1] * Gn).sum((0, 1, 2))
        np.testing.assert_allclose(dW.v.view(Cout, taps, Cin).numpy(), want, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(db.v.numpy(), Gn.sum((0, 1, 2)), rtol=1e-12, atol=1e-12)


CPU_CONV = [  # (mode, B, Hin, Win, Cin, Cout, wrows)
    (E.CONV_S1, 2, 8, 16, 64, 128, 128),
    (E.CONV_S1, 1, 8, 8, 128, 64, 52),
    (E.CONV_S2, 2, 8, 8, 64, 64, 64),
    (E.CONV_UP, 1, 4, 8, 64, 64, 64),
    (E.CONV_TS2, 2, 4, 4, 64, 64, 64),
    (E.CONV_1X1, 6, 1, 1, 64, 96, 96),
]
EPILOGUES = [dict(), dict(act=E.ACT_SILU), dict(res=True), dict(mul=True, mulmode=E.MUL_DSILU, res=True), dict(mul=True), dict(y2=True),
             dict(act=E.ACT_SILU_PAIR)]


@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("case", CPU_CONV)
def test_restatement_is_within_the_bound_conv(case, dt):
    mode, B, H, W, Cin, Cout, wrows = case
    taps = 1 if mode == E.CONV_1X1 else 9
    Hout, Wout = out_hw(mode, H, W)
    g = geom(B, H, W, Cin, Hout, Wout, Cout, Cout, wrows, mode)
    npix = B * Hout * Wout
    x = rnd((B * H * W, Cin), dt, 1)
    w = rnd((wrows, taps, Cin), dt, 2, 1.0 / math.sqrt(taps * Cin))
    bias = rnd((wrows,), F32, 3)
    res, mul = rnd((npix, Cout), dt, 4), rnd((npix, Cout), dt, 5)
    lay = dict(B=B, H=Hout, W=Wout, C=Cout, creal=wrows)
    for ep in EPILOGUES:
        kw = dict(ep)
        kw["res"] = res if kw.get("res") else None
        kw["mul"] = mul if kw.get("mul") else None
        two = kw.pop("y2", False) or kw.get("act") == E.ACT_SILU_PAIR
        y, y2 = torch.zeros((npix, Cout), dtype=TD[dt]), torch.zeros((npix, Cout), dtype=TD[dt])
        E.conv(x, w, bias, y, g, dt, y2=y2 if two else None, **kw)
        ref = R.conv(x, w, g, dt, bias=bias, y2=two, **kw)
        worst = R.assert_within(y, ref["y"], what=f"conv {case} {ep}", layout=lay)
        if two:
            R.assert_within(y2, ref["y2"], what=f"conv {case} {ep} second output", layout=lay)
        if not ep:
            assert worst > 1e-3, f"vacuous bound: {worst:.2e}"  # the bound is not loose
            # power check: one tap of one input channel missing at the border pixels of image 0
            tap = 4 if mode != E.CONV_1X1 else None
            t = R.conv_term(x, w, g, 0, slice(0, 1), tap, R.border_mask(Hout, Wout))
            R.assert_rejects(y.double() - t, ref["y"], what="missing border tap")


@pytest.mark.parametrize("dt", [BF16, F16])
def test_restatement_is_within_the_bound_epilogues(dt):
    """pool2, fused LayerNorm forward (with rstd) and backward (dm), the padded edge conv 65(128) -> 128 with kvalid"""
    B, H, W, C = 2, 8, 16, 128
    g = geom(B, H, W, C, H, W, C, C, C, E.CONV_S1)
    npix = B * H * W
    x = rnd((npix, C), dt, 1)
    w = rnd((C, 9, C), dt, 2, 1.0 / math.sqrt(9 * C))
    bias = rnd((C,), F32, 3)
    res = rnd((npix, C), dt, 4)
    m = rnd((B, C + 64), F32, 6)
    lay = dict(B=B, H=H, W=W, C=C)
    yp = torch.zeros((npix // 4, C), dtype=TD[dt])
    E.conv(x, w, None, yp, g, dt, pool2=True)
    R.assert_within(yp, R.conv(x, w, g, dt, pool2=True)["y"], what="pool2")
    for unbiased in (True, False):
        lnf = dict(m=m.view(-1)[32:], ldm=C + 64, eps=1e-5, unbiased=unbiased)
        y, hn, rs = torch.zeros((npix, C), dtype=TD[dt]), torch.zeros((npix, C), dtype=TD[dt]), torch.zeros(npix)
        E.conv(x, w, bias, y, g, dt, res=res, lnf=dict(lnf, y=hn, rstd=rs))
        ref = R.conv(x, w, g, dt, bias=bias, res=res, lnf=lnf)
        R.assert_within(y, ref["y"], what="conv next to lnf", layout=lay)
        R.assert_within(hn, ref["hn"], what="lnf output", layout=lay)
        R.assert_within(rs, ref["rstd"], what="lnf rstd")
        lnx = rnd((npix, C), dt, 7)
        dm = torch.zeros_like(m)
        ln = dict(x=lnx, m=m.view(-1)[32:], ldm=C + 64, eps=1e-5, unbiased=unbiased)
        E.conv(x, w, None, y, g, dt, res=res, ln=dict(ln, dm=dm.view(-1)[32:]))
        ref = R.conv(x, w, g, dt, res=res, ln=ln)
        R.assert_within(y, ref["y"], what="fused ln bwd dx", layout=lay)
        got_dm = dm[:, 32:32 + C]
        R.assert_within(got_dm, ref["dm"], what="fused ln bwd dm")
        # power check: one 8x16 tile of image 0 missing from dm -- its rows' contribution, from the same reference on that tile alone
        gt = geom(1, 8, 16, C, 8, 16, C, C, C, E.CONV_S1)
        xt = x.view(B, H, W, C)[0:1].reshape(-1, C)  # image 0 is exactly one 8x16 tile
        tile = R.conv(xt, w, gt, dt, res=res[:128], ln=dict(ln, x=lnx[:128], m=m[0:1].reshape(-1)[32:], ldm=0))["dm"]
        bad = got_dm.double().clone()
        bad[0] -= tile.v[0]
        R.assert_rejects(bad, ref["dm"], what="fused ln bwd dm, tile missing")
    # network input 65(128) -> 128: channel 64's term at one tap missing
    xi = x.clone()
    xi[:, 65:] = 0
    wi = w.clone()
    wi[:, :, 65:] = 0
    y = torch.zeros((npix, C), dtype=TD[dt])
    E.conv(xi, wi, bias, y, g, dt)
    ref = R.conv(xi, wi, g, dt, bias=bias, kvalid=65)
    R.assert_within(y, ref["y"], what="edge conv", layout=dict(lay, creal=65))
    R.assert_rejects(y.double() - R.conv_term(xi, wi, g, 1, slice(64, 65), 4), ref["y"], what="edge conv, channel 64 at one tap")
    # split-K: one 64-channel K chunk of one output tile (8x16 pixels of image 1, 128 channels) missing
    R.assert_rejects(y.double() - R.conv_term(xi, wi, g, 1, slice(0, 64), None, R.tile_mask(H, W)), ref["y"], what="split-K chunk")


@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("mode", [E.CONV_S1, E.CONV_S2, E.CONV_UP, E.CONV_1X1])
def test_restatement_is_within_the_bound_wgrad(mode, dt):
    B, H, W, Cin, Cout = (3, 8, 16, 64, 128) if mode != E.CONV_1X1 else (512, 1, 1, 64, 96)
    taps = 1 if mode == E.CONV_1X1 else 9
    Hout, Wout = out_hw(mode, H, W)
    g = geom(B, H, W, Cin, Hout, Wout, Cout, Cout, Cout, mode)
    x = rnd((B * H * W, Cin), dt, 1)
    dy = rnd((B * Hout * Wout, Cout), dt, 2)
    dw, db = torch.zeros(Cout * taps * Cin), torch.zeros(Cout)
    E.conv_wgrad(x, dy, dw, g, dt, dbias=db)
    rw, rb = R.wgrad(x, dy, g)
    worst = R.assert_within(dw, rw, what="dW")
    R.assert_within(db, rb, what="dbias")
    assert worst > 1e-3, f"vacuous bound: {worst:.2e}"
    if mode == E.CONV_1X1:
        return
    # power checks: one 8x16 tile of image 1 removed from the pixel sum, and added twice
    mask = R.tile_mask(Hout, Wout, th=min(8, Hout), tw=min(16, Wout))
    tw_, tb_ = R.wgrad(x, dy, g, images=(1, 2), pixels=mask)
    for sgn in (-1.0, 1.0):
        R.assert_rejects(dw.double() + sgn * tw_.v.reshape(-1), rw.v.reshape(-1), rw.e.reshape(-1), what=f"dW tile x{1 + sgn:g}")
        R.assert_rejects(db.double() + sgn * tb_.v, rb, what=f"dbias tile x{1 + sgn:g}")


@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("shape", [(2, 128, 128, True), (2, 256, 384, True), (3, 64, 512, False)])
def test_restatement_is_within_the_bound_layernorm(shape, dt):
    B, HW, C, per_sample = shape
    npix = B * HW
    x, dy, dres = rnd((npix, C), dt, 1), rnd((npix, C), dt, 3), rnd((npix, C), dt, 4)
    m = rnd((B if per_sample else 1, C + 64), F32, 2)
    ldm = C + 64 if per_sample else 0
    mm = m.view(-1)[32:]
    y = torch.zeros_like(x)
    E.ln_forward(x, mm, y, npix, HW, C, ldm, 1e-5, True, dt)
    R.assert_within(y, R.ln_forward(x, mm, npix, HW, C, ldm, 1e-5, True, dt)[0], what="ln fwd")
    dx, dm = torch.zeros_like(x), torch.zeros_like(m)
    E.ln_backward(dy, x, mm, dres, dx, dm.view(-1)[32:], npix, HW, C, ldm, 1e-5, True, dt)
    rdx, rdm = R.ln_backward(dy, x, mm, dres, npix, HW, C, ldm, 1e-5, True, dt)
    R.assert_within(dx, rdx, what="ln bwd dx")
    got = dm[:, 32:32 + C]
    R.assert_within(got, rdm, what="ln bwd dm")
    # power check: one 128-pixel tile of image 0 removed from dm
    _, tdm = R.ln_backward(dy[:128], x[:128], m[0:1].reshape(-1)[32:], None, 128, 128, C, ldm, 1e-5, True, dt)
    bad = got.double().clone()
    bad[0] -= tdm.v[0]
    R.assert_rejects(bad, rdm, what="ln bwd dm, tile missing")


@pytest.mark.parametrize("dt", [F32, BF16, F16])
def test_restatement_is_within_the_bound_reductions(dt):
    B, C, HW, ldc = 4, 52, 4096, 64
    y = rnd((B * HW, ldc), dt, 1)
    eps = rnd((B, C, HW), F32, 2)
    dy, ls = torch.zeros_like(y), torch.zeros(1)
    E.mse_loss_grad(y, eps, dy, ls, B, C, HW, ldc, 0.37, dt)
    ref = R.mse_loss_sum(y, eps, B, C, HW, ldc)
    R.assert_within(ls, ref.v.view(1), ref.e.view(1), what="mse loss sum")
    R.assert_within(dy, R.mse_dy(y, eps, B, C, HW, ldc, 0.37, dt), what="mse dy")
    block = R.mse_loss_sum(y[:256], eps[:1, :, :256], 1, C, 256, ldc).v  # one 256-pixel block
    R.assert_rejects(ls.double() - block, ref.v.view(1), ref.e.view(1), what="loss sum, block missing")
    out, ls2 = torch.zeros(B * C * HW), torch.zeros(1)
    E.sq_err(y, eps, out, ls2, B, C, HW, ldc, dt)
    ref = R.sq_err_sum(y, eps, B, C, HW, ldc)
    R.assert_within(ls2, ref.v.view(1), ref.e.view(1), what="sq_err loss sum")
    a = rnd((5000, 192), dt, 3)
    cs = torch.zeros(128)
    E.colsum(a, cs, 5000, 128, 192, dt)
    ref = R.colsum(a, 5000, 128, 192, dt)
    R.assert_within(cs, ref, what="colsum")
    R.assert_rejects(cs.double() - a[:256, :128].double().sum(0), ref, what="colsum, 256 rows missing")
    v = torch.randn(300000, generator=torch.Generator().manual_seed(4))
    s = torch.zeros(1)
    E.sumsq(v, s, v.numel())
    ref = R.sumsq(v, v.numel())
    R.assert_within(s, ref.v.view(1), ref.e.view(1), what="sumsq")
    R.assert_rejects(s.double() - (v[:256].double() ** 2).sum(), ref.v.view(1), ref.e.view(1), what="sumsq, 256 elements missing")


def test_assert_within_names_the_place_and_region():
    ref = torch.zeros(2 * 8 * 16 * 192, dtype=torch.float64)
    bound = torch.full_like(ref, 1e-3)
    got = ref.clone().view(2 * 8 * 16, 192)
    got[(1 * 8 + 7) * 16 + 3, 170] = 1.0  # image 1, row 7, column 3, channel 170
    with pytest.raises(AssertionError) as ei:
        R.assert_within(got, ref.view_as(got), bound.view_as(got), "probe", layout=dict(B=2, H=8, W=16, C=192, creal=180))
    msg = str(ei.value)
    assert "image 1, row 7, column 3, channel 170" in msg and "border row/column" in msg and "tile seam" in msg
    assert "last partial channel tile" in msg and "1 of" in msg
    assert R.assert_within(ref, ref, bound) == 0.0
