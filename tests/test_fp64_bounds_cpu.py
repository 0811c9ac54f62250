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

import attention_cases as A
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


def _relu_case(dt, seed=1):
    B, H, W, C = 2, 8, 16, 128
    g = geom(B, H, W, C, H, W, C, C, C, E.CONV_S1)
    npix = B * H * W
    x = rnd((npix, C), dt, seed)
    w = rnd((C, 9, C), dt, seed + 1, 1.0 / math.sqrt(9 * C))
    bias = rnd((C,), F32, seed + 2)
    return g, npix, x, w, bias, dict(B=B, H=H, W=W, C=C)


@pytest.mark.parametrize("dt", [F32, BF16, F16])
def test_restatement_is_within_the_bound_relu(dt):
    """C2W_ACT_RELU and C2W_ACT_RELU_PAIR (with multiplier and residual in front of the pair), the mask's consistency rule, and the mutant
    "ReLU missing on one 8x16 tile" (negatives pass) planted in float64 on the restatement's output"""
    g, npix, x, w, bias, lay = _relu_case(dt)
    C = g["Cout"]
    res, mul = rnd((npix, C), dt, 4), rnd((npix, C), dt, 5)
    y, pre = torch.zeros((npix, C), dtype=TD[dt]), torch.zeros((npix, C), dtype=TD[dt])
    E.conv(x, w, bias, y, g, dt, act=E.ACT_RELU)
    ref = R.conv(x, w, g, dt, bias=bias, act=R.ACT_RELU)
    worst = R.assert_within(y, ref["y"], what="relu", layout=lay)
    assert worst > 1e-3 and float(y.min()) == 0.0 and float((y == 0).float().mean()) > 0.2
    E.conv(x, w, bias, pre, g, dt)
    bad = y.double().view(2, 8, 16, C).clone()
    bad[1] = pre.double().view(2, 8, 16, C)[1]  # image 1 is exactly one 8x16 tile
    R.assert_rejects(bad.view(npix, C), ref["y"], what="ReLU missing on one tile")
    R.assert_rejects(y.double() - R.conv_term(x, w, g, 0, slice(0, 1), 4, R.border_mask(8, 16)), ref["y"], what="relu, missing border tap")
    for kw in (dict(), dict(res=res), dict(mul=mul, res=res)):
        y2 = torch.full((npix, C), 7.0, dtype=TD[dt])
        E.conv(x, w, bias, y, g, dt, act=E.ACT_RELU_PAIR, y2=y2, **kw)
        ref = R.conv(x, w, g, dt, bias=bias, act=R.ACT_RELU_PAIR, **kw)
        assert set(ref) == {"y"}  # the mask has no numeric bound
        R.assert_within(y, ref["y"], what=f"relu pair {sorted(kw)}", layout=lay)
        R.assert_mask_consistent(y, y2, what="relu pair")
        flipped = y2.clone()
        i = int((y.reshape(-1) > 0).nonzero()[17])
        flipped.view(-1)[i] = 0
        with pytest.raises(AssertionError, match="disagree on 1 of"):
            R.assert_mask_consistent(y, flipped)
        flipped = y2.clone()
        flipped.view(-1)[int((y.reshape(-1) == 0).nonzero()[5])] = 1
        with pytest.raises(AssertionError, match="disagree on 1 of"):
            R.assert_mask_consistent(y, flipped)


def test_nan_footprint_rule():
    """a NaN in x reaches 3x3 pixels x all weight rows of the float64 reference, through ReLU too; the helper wants exactly those"""
    dt = BF16
    g, npix, x, w, bias, lay = _relu_case(dt)
    x.view(2, 8, 16, 128)[1, 3, 5, 9] = float("nan")
    y = torch.zeros((npix, 128), dtype=TD[dt])
    E.conv(x, w, bias, y, g, dt, act=E.ACT_RELU)
    ref = R.conv(x, w, g, dt, bias=bias, act=R.ACT_RELU)
    worst, n = R.assert_nan_footprint(y, ref["y"], what="relu nan", layout=lay)
    assert n == 9 * 128 and worst <= 1.0
    erased = torch.where(torch.isnan(y), torch.zeros_like(y), y)  # what max(NaN, 0) = 0 does
    with pytest.raises(AssertionError, match="NaN where"):
        R.assert_nan_footprint(erased, ref["y"], what="erased")
    spread = y.clone()
    spread[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="NaN where"):
        R.assert_nan_footprint(spread, ref["y"], what="spread")


def _kept_operands(npix, C, dt, unbiased, seed=7):
    """xhat and 1/sigma as a real LayerNorm forward keeps them: the normalised rows in the storage type, rstd in fp32; image 0's first rows
    are constant (xhat = 0, rstd = 1/sqrt(eps))"""
    u = rnd((npix, C), dt, seed).float()
    u[:32] = 0.75
    var, mean = torch.var_mean(u, dim=1, unbiased=unbiased, keepdim=True)
    rs = (var + 1e-5).rsqrt()
    return ((u - mean) * rs).to(TD[dt]), rs.view(-1).contiguous()


@pytest.mark.parametrize("dt", [BF16, F16])
def test_restatement_is_within_the_bound_kept_statistics(dt):
    """the fused LayerNorm backward from kept statistics (ln.rstd), per-sample and shared dm rows, with / without residual; mutants:
    den = C instead of C - 1, one 8x16 tile missing from dm"""
    B, H, W, C = 2, 8, 16, 128
    g = geom(B, H, W, C, H, W, C, C, C, E.CONV_S1)
    npix = B * H * W
    x = rnd((npix, C), dt, 1)
    w = rnd((C, 9, C), dt, 2, 1.0 / math.sqrt(9 * C))
    res = rnd((npix, C), dt, 4)
    lay = dict(B=B, H=H, W=W, C=C)
    for unbiased in (True, False):
        xh, rs = _kept_operands(npix, C, dt, unbiased)
        assert rs.max().item() == pytest.approx(1e-5 ** -0.5, rel=1e-6)
        for ldm in (C + 64, 0):
            for r in (res, None):
                dm = torch.zeros((B if ldm else 1, C + 64))
                ln = dict(x=xh, rstd=rs, ldm=ldm, eps=1e-5, unbiased=unbiased)
                y = torch.zeros((npix, C), dtype=TD[dt])
                E.conv(x, w, None, y, g, dt, res=r, ln=dict(ln, dm=dm.view(-1)[32:]))
                ref = R.conv(x, w, g, dt, res=r, ln=ln)
                R.assert_within(y, ref["y"], what="kept statistics dx", layout=lay)
                got_dm = dm[:, 32:32 + C]
                R.assert_within(got_dm, ref["dm"], what="kept statistics dm")
                if dt == F16:  # den = C for C - 1 (or the reverse): the restatement with the other flag is what such a kernel writes
                    yb, dmb = torch.zeros_like(y), torch.zeros_like(dm)
                    E.conv(x, w, None, yb, g, dt, res=r, ln=dict(ln, unbiased=not unbiased, dm=dmb.view(-1)[32:]))
                    R.assert_rejects(yb.double(), ref["y"], what="kept statistics, wrong denominator")
                # one 8x16 tile (image 0) missing from dm
                gt = geom(1, 8, 16, C, 8, 16, C, C, C, E.CONV_S1)
                tile = R.conv(x[:128], w, gt, dt, ln=dict(ln, x=xh[:128], rstd=rs[:128], ldm=0))["dm"]
                bad = got_dm.double().clone()
                bad[0] -= tile.v[0]
                R.assert_rejects(bad, ref["dm"], what="kept statistics dm, tile missing")


@pytest.mark.parametrize("dt", [BF16, F16])
def test_the_dm_bound_sees_the_wrong_denominator_of_the_kept_statistics(dt):
    """den = C where the LayerNorm was unbiased changes one term of o by 1 / 128 = 2 u_T(bf16) of it: per element that is inside the
    worst-case propagation of the tile's own rounding, so in bf16 the rows cannot see it on random data.  The modulation gradient can: its
    bound adds the pixels' roundings in quadrature, the defect adds up coherently where the gradient is aligned with xhat.  Here every pixel
    holds the same normalised row p and the conv (centre tap = identity) hands g = p through: the exact o is 0 (sum p^2 = C - 1), the
    mutant's is rs p / C on every pixel."""
    B, H, W, C = 2, 16, 16, 128
    g = geom(B, H, W, C, H, W, C, C, C, E.CONV_S1)
    npix = B * H * W
    p = rnd((1, C), dt, 5).float()
    var, mean = torch.var_mean(p, dim=1, unbiased=True, keepdim=True)
    xh = ((p - mean) * var.rsqrt()).to(TD[dt]).expand(npix, C).contiguous()
    rs = torch.full((npix,), 1.5)
    w = torch.zeros((C, 9, C), dtype=TD[dt])
    w[:, 4] = torch.eye(C, dtype=TD[dt])
    for ldm in (C, 0):
        ln = dict(x=xh, rstd=rs, ldm=ldm, eps=1e-5, unbiased=True)
        dm, dmb, y = torch.zeros((B if ldm else 1, C)), torch.zeros((B if ldm else 1, C)), torch.zeros((npix, C), dtype=TD[dt])
        E.conv(xh, w, None, y, g, dt, ln=dict(ln, dm=dm))
        ref = R.conv(xh, w, g, dt, ln=ln)
        R.assert_within(y, ref["y"], what="aligned rows dx")
        R.assert_within(dm, ref["dm"], what="aligned rows dm")
        E.conv(xh, w, None, y, g, dt, ln=dict(ln, unbiased=False, dm=dmb))
        R.assert_rejects(dmb.double(), ref["dm"], what="kept statistics dm, den = C for C - 1")


def _chain_operands(npix, HW, C, dt, ldm, seed=11, const=None):
    """the block input x0 (never written), its modulation m0 and what the earlier launch emitted: h = LN(x0 + m0) in the storage type with
    the row's mean and 1/sigma in fp32.  Image 1's first rows of x0 + m0 are constant: h = 0 there and the rebuilt x = mean - m."""
    nb = npix // HW
    m0 = rnd((nb if ldm else 1, ldm or C), F32, seed + 1)
    mrow = m0[:, :C].repeat_interleave(HW, 0) if ldm else m0[:, :C].expand(npix, C)
    x0 = rnd((npix, C), dt, seed, 2.0).float()
    const = const or slice(npix // 2, npix // 2 + 32)
    x0[const] = 0.5 - mrow[const]
    u = x0 + mrow
    var, mean = torch.var_mean(u, dim=1, unbiased=True, keepdim=True)
    rs = (var + 1e-5).rsqrt()
    h = ((u - mean) * rs).to(TD[dt])
    h[const], rs[const], mean[const] = 0.0, 1e-5 ** -0.5, 0.5  # what the LayerNorm of an exactly constant row emits
    return h, rs.view(-1).contiguous(), mean.view(-1).contiguous(), m0, x0


CHAIN_FORMS = {  # the four forms of tests/test_gpu_bench_dispatch.py::test_chain_form_of_the_layernorm_emitting_convolution
    "plain residual, output not written": dict(resn=False, no_y=True, m=True),
    "rebuilt residual, output not written": dict(resn=True, no_y=True, m=True),
    "rebuilt residual, output written": dict(resn=True, no_y=False, m=True),
    "rebuilt residual, plain LayerNorm (up-block consumer)": dict(resn=True, no_y=False, m=False),
}


def chain_launch(conv, form, x, w, bias, g, dt, ops_, fill=3.0, **over):
    """one chain-form launch through `conv` (emu_ops.conv or ops.conv); ops_ = _chain_operands(...).  Returns (y, hn, rstd, mean, kwargs for
    fp64_ref.conv)."""
    h, rs, mean, m0, x0 = ops_
    f = CHAIN_FORMS[form]
    npix, C = g["B"] * g["Hout"] * g["Wout"], g["Cout"]
    ldm = m0.shape[1] if m0.shape[0] > 1 else 0
    dev = x.device
    m1 = rnd(tuple(m0.shape), F32, 23).to(dev) if f["m"] else None
    y = torch.full((npix, C), fill, dtype=TD[dt], device=dev)
    hn = torch.zeros((npix, C), dtype=TD[dt], device=dev)
    rstd, mu = torch.zeros(npix, device=dev), torch.zeros(npix, device=dev)
    lnf = dict(m=m1, ldm=ldm, eps=1e-5, unbiased=True)
    if f["resn"]:
        kw = dict(res=h, resn=dict(rstd=rs, mean=mean, m=m0), no_y=f["no_y"])
    else:
        kw = dict(res=x0.to(TD[dt]), no_y=f["no_y"])
    kw.update(over)
    conv(x, w, bias, y, g, dt, lnf=dict(lnf, y=hn, rstd=rstd, mean=mu), **kw)
    return y, hn, rstd, mu, dict(kw, lnf=dict(lnf, mean=True))


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("form", list(CHAIN_FORMS))
def test_restatement_is_within_the_bound_chain_form(form, dt):
    """lnf.mean / resn / no_y: hn, rstd, mean and (where written) y of the restatement lie inside the bound, with per-sample and shared
    modulation rows; mutants: rebuilt residual without - m, rebuilt residual with rstd used as sigma"""
    B, H, W, C = 2, 8, 16, 128
    g = geom(B, H, W, C, H, W, C, C, C, E.CONV_S1)
    npix = B * H * W
    x = rnd((npix, C), dt, 1)
    w = rnd((C, 9, C), dt, 2, 1.0 / math.sqrt(9 * C))
    bias = rnd((C,), F32, 3)
    lay = dict(B=B, H=H, W=W, C=C)
    for ldm in (C + 64, 0):
        co = _chain_operands(npix, H * W, C, dt, ldm)
        y, hn, rstd, mu, kw = chain_launch(E.conv, form, x, w, bias, g, dt, co)
        ref = R.conv(x, w, g, dt, bias=bias, **kw)
        assert ("y" in ref) == (not CHAIN_FORMS[form]["no_y"])
        if "y" in ref:
            R.assert_within(y, ref["y"], what="chain y", layout=lay)
        else:
            assert bool((y == 3.0).all())
        R.assert_within(hn, ref["hn"], what="chain hn", layout=lay)
        R.assert_within(rstd, ref["rstd"], what="chain rstd")
        R.assert_within(mu, ref["mean"], what="chain mean")
        if not CHAIN_FORMS[form]["resn"]:
            continue
        h, rs, mean, m0, _ = co
        for what, resn in (("without - m", dict(rstd=rs, mean=mean, m=None)), ("rstd used as sigma", dict(rstd=1.0 / rs, mean=mean, m=m0))):
            yb, hnb, rsb, mub, _ = chain_launch(E.conv, form, x, w, bias, g, dt, co, resn=resn)
            if resn["m"] is None:  # (the normalised rows sum to zero: their scale does not reach the mean, it reaches 1/sigma)
                R.assert_rejects(mub.double(), ref["mean"], what=f"chain mean, rebuilt residual {what}")
            else:
                R.assert_rejects(rsb.double(), ref["rstd"], what=f"chain rstd, rebuilt residual {what}")
            R.assert_rejects(hnb.double(), ref["hn"], what=f"chain hn, rebuilt residual {what}")
            if "y" in ref:
                R.assert_rejects(yb.double(), ref["y"], what=f"chain y, rebuilt residual {what}")


@pytest.mark.parametrize("dt", [BF16, F16])
def test_the_mean_bound_sees_a_layernorm_of_the_rounded_sum_where_none_is_written(dt):
    """With C2W_CONV_NO_Y the LayerNorm sees the fp32 sum u.  A kernel that rounded u to the storage type first (the form that writes y)
    would move every element by up to u_T |u| and the row mean by about u_T |u| / sqrt(128).  In hn that is of the size of hn's own rounding
    u_T |hn|: only the elements next to the row's mean (|hn| << 1, where the bound is small: a sixth of them here) show it, most of hn cannot.  The mean
    is an fp32 output: its bound is the conv tile's rounding u_T |a| (worst case over the row) plus fp32 terms, so with a block input much
    larger than the conv result (|x0| ~ 2, |a| ~ 0.01 here, as deep in a residual chain) the mutant's shift of the mean stands out in most
    rows, and the bound on `mean` must reject it."""
    B, H, W, C = 2, 8, 16, 128
    g = geom(B, H, W, C, H, W, C, C, C, E.CONV_S1)
    npix = B * H * W
    x = rnd((npix, C), dt, 1)
    w = rnd((C, 9, C), dt, 2, 0.01 / math.sqrt(9 * C))
    co = _chain_operands(npix, H * W, C, dt, C + 64)
    form = "rebuilt residual, output not written"
    y, hn, rstd, mu, kw = chain_launch(E.conv, form, x, w, None, g, dt, co)
    ref = R.conv(x, w, g, dt, **kw)
    R.assert_within(mu, ref["mean"], what="chain mean")
    R.assert_within(hn, ref["hn"], what="chain hn")
    _, hnb, _, mub, _ = chain_launch(E.conv, form, x, w, None, g, dt, co, no_y=False)  # normalises the rounded sum
    R.assert_rejects(mub.double(), ref["mean"], what="no_y form normalising the rounded sum")
    assert (R.ratio(mub, ref["mean"]) > 1).double().mean().item() > 0.8 > 0.2 > (R.ratio(hnb, ref["hn"]) > 1).double().mean().item()


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


# ---------------------------------------------------------------------------------------------------------------------- attention
ATT_TOL = {F32: 1e-4, BF16: 2e-2, F16: 4e-3}  # test_gpu_kernels.py:22, the tolerance of the check that stays beside the bound
LOG2E = 1.4426950408889634


def fast_exp(x):
    """__expf: exp2 of the fp32 product x * log2(e)"""
    return torch.exp2(x * np.float32(LOG2E))


def _halves(out, prev, C, mutate):
    """the two wave halves' column tiles of an output strip (attention_mfma.hip:164-165, 215, 388, 439); the mutant's upper half starts
    one tile late, so tile ctm keeps the buffer's previous content"""
    if mutate != "ctm+1":
        return out
    ctm = (C // 16) // 2
    res = out.clone()
    res[..., 16 * ctm:16 * ctm + 16] = prev
    return res


def restate_forward(qkv, B, T, C, dt, route, mutate=None, prev=7.0):
    """fp32 / storage-typed restatement of the route's forward arithmetic -> (o rows of the storage type, lse fp32)"""
    t = TD[dt]
    q, k, v = qkv.float().view(B, T, 3 * C).split(C, dim=-1)
    s2 = np.float32(1.0) / np.sqrt(np.float32(C))
    S = torch.einsum("btc,bsc->bts", q, k) * s2
    if route == R.VALU:  # attention.hip:113-132: fp32 P, expf
        m = S.amax(-1, keepdim=True)
        e = (S - m).exp()
        l = e.sum(-1, keepdim=True)
        o = torch.einsum("bts,bsc->btc", e * (1.0 / l), v)
        return o.to(t).view(B * T, C), (m + l.log()).reshape(-1)
    if route == R.T64:  # attention_mfma.hip:138-157: P normalised, then rounded
        m = S.amax(-1, keepdim=True)
        e = fast_exp(S - m)
        l = e.sum(-1, keepdim=True)
        P = (e * (1.0 / l)).to(t).float()
        o = _halves(torch.einsum("bts,bsc->btc", P, v), prev, C, mutate)
        return o.to(t).view(B * T, C), (m + l.log()).reshape(-1)
    mrun = torch.full((B, T, 1), -math.inf)  # attention_mfma.hip:257-318: online softmax over 64-key blocks, P rounded unnormalised
    lrun = torch.zeros((B, T, 1))
    oacc = torch.zeros((B, T, C))
    for j in range(T // 64):
        s = S[..., 64 * j:64 * j + 64]
        mx = torch.maximum(s.amax(-1, keepdim=True), mrun)
        alpha = fast_exp(mrun - mx)
        e = fast_exp(s - mx)
        lrun = lrun * alpha + e.sum(-1, keepdim=True)
        mrun = mx
        if mutate != "no_alpha":
            oacc = oacc * alpha
        oacc = oacc + torch.einsum("bts,bsc->btc", e.to(t).float(), v[:, 64 * j:64 * j + 64])
    return (oacc * (1.0 / lrun)).to(t).view(B * T, C), (mrun + lrun.log()).reshape(-1)


def restate_backward(qkv, o_in, do, lse_in, B, T, C, dt, route, mutate=None, prev=7.0):
    """fp32 / storage-typed restatement of the route's backward arithmetic -> (dqkv rows of the storage type, delta fp32 or None)"""
    t = TD[dt]
    q, k, v = qkv.float().view(B, T, 3 * C).split(C, dim=-1)
    dO = do.float().view(B, T, C)
    l = lse_in.float().view(B, T, 1)
    s2 = np.float32(1.0) / np.sqrt(np.float32(C))
    S = torch.einsum("btc,bsc->bts", q, k) * s2
    dP = torch.einsum("btc,bsc->bts", dO, v)
    if route == R.VALU:  # attention.hip:150-188: P, dS fp32, expf, s^2 after the sum
        delta = (dO * o_in.float().view(B, T, C)).sum(-1, keepdim=True)
        P = (S - l).exp()
        dS = P * (dP - delta)
        dq = torch.einsum("bts,bsc->btc", dS, k) * s2
        dk = torch.einsum("bts,btc->bsc", dS, q) * s2
        dv = torch.einsum("bts,btc->bsc", P, dO)
        return torch.cat((dq, dk, dv), -1).to(t).view(B * T, 3 * C), delta.reshape(-1)
    P = fast_exp(S - l)
    if route == R.T64:  # attention_mfma.hip:196-212: delta = the fp32 row sum of P dP
        delta = (P * dP).sum(-1, keepdim=True)
    else:  # attention.hip:259-260, attention_mfma.hip:356-368: delta = rowdot(dO, o_in)
        delta = (dO * o_in.float().view(B, T, C)).sum(-1, keepdim=True)
    dS = (P * (dP - delta) * s2).to(t).float()
    Pr = P.to(t).float()
    dq = _halves(torch.einsum("bts,bsc->btc", dS, k), prev, C, mutate)
    dk = _halves(torch.einsum("bts,btc->bsc", dS, q), prev, C, mutate)
    dv = _halves(torch.einsum("bts,btc->bsc", Pr, dO), prev, C, mutate)
    return torch.cat((dq, dk, dv), -1).to(t).view(B * T, 3 * C), None if route == R.T64 else delta.reshape(-1)


# every regime on each route: T64, BLOCKS, VALU (every dtype; the tiny test network's attention level); then the kernels' edge widths
# (ksm = 0; odd nks and ctm) and a T that is no multiple of 16
ATT_CPU = [((3, 64, 512), r) for r in A.REGIMES] + [((2, 256, 512), r) for r in A.REGIMES] + [((2, 64, 16), r) for r in A.REGIMES]
ATT_CPU += [(s, r) for s in ((2, 64, 32), (2, 192, 160), (3, 36, 64)) for r in ("randn", "peaked")]
ATT_DEFECTS = {R.VALU: ("p_tile", "key", "delta_row", "ds_scale"), R.T64: ("p_tile", "key", "delta_row", "ds_scale"),
               R.BLOCKS: ("p_tile", "key", "alpha", "dq_block", "delta_row", "ds_scale")}
SECTION = A.SECTION


def _att_dtypes(shape):
    return [F32, BF16, F16] if A.attn_route(*shape, BF16) == R.VALU else [BF16, F16]


def _vacuity(name, bound, scale, dt):
    r = bound / (ATT_TOL[dt] * scale)
    med, mx = r.median().item(), r.max().item()
    print(f"    {name}: bound / (TOL x scale) median {med:.3f} max {mx:.3f}")
    assert med < 1.0, f"{name}: the bound is wider than the old tolerance at a typical element (median {med:.3f})"
    return med


def check_regime_property(regime, qkv, B, T, C):
    pmax, lmin, lmax, up, flat = A.attention_regime_stats(qkv, B, T, C)
    ng = -(-T // A.attention_group(T))
    print(f"    regime {regime}: mean row max {pmax:.3f}, |lse| in [{lmin:.1f}, {lmax:.1f}], groups raising the maximum {up:.2f} of {ng - 1}")
    if regime in ("randn", "smallgrad"):
        assert pmax < 0.6 and lmax <= 14
    elif regime == "peaked":
        assert pmax > 0.8
    elif regime == "shifted":
        assert 40 <= lmin and lmax <= 90 and pmax < 0.5
    elif regime == "rising":
        assert up >= 0.95 * (ng - 1)
    elif regime == "falling":
        assert up <= 0.05 * (ng - 1)
    elif regime == "uniform":
        assert abs(pmax - 1.0 / T) < 1e-12


@pytest.mark.parametrize("shape,regime", ATT_CPU)
def test_restatement_is_within_the_bound_attention(shape, regime):
    """Each route's restatement is within the bound at every element, forward and backward (on the emulated and on its own forward
    outputs); every planted defect is rejected; the regime has the property it is named for; the bound is tighter than the old
    tolerance at the median element.  Measured medians of bound / (TOL x scale), the largest over the regimes run at the shape
    (o / dq / dk / dv; TOL x scale = the old check's tolerance: max |o| forward, max |dqkv| backward):
      (3, 64, 512)  T64    bf16 0.420 / 0.175 / 0.246 / 0.134 (uniform)   fp16 0.298 / 0.373 / 0.372 / 0.090 (uniform; dq, dk smallgrad)
      (2, 256, 512) BLOCKS bf16 0.616 / 0.240 / 0.391 / 0.168 (uniform)   fp16 0.460 / 0.877 / 0.873 / 0.115 (uniform; dq, dk smallgrad)
      (2, 64, 16)   VALU   fp32 0.646 / 0.444 / 0.442 / 0.087 (shifted)   bf16 0.065 / 0.036 / 0.056 / 0.017   fp16 0.049 / 0.029 / 0.039 / 0.012
      (2, 64, 32)   T64    bf16 0.085 / 0.046 / 0.043 / 0.026             fp16 0.055 / 0.031 / 0.029 / 0.017
      (2, 192, 160) BLOCKS bf16 0.068 / 0.072 / 0.068 / 0.037             fp16 0.062 / 0.048 / 0.046 / 0.024
      (3, 36, 64)   VALU   fp32 0.616 / 0.061 / 0.053 / 0.048 (peaked)    bf16 0.040 / 0.020 / 0.018 / 0.007   fp16 0.038 / 0.013 / 0.012 / 0.005
    The two largest: fp16 with do * 2^-12 at T = 256, where dS s^2 is rounded on the fp16 subnormal grid (2^-25 per element over 256
    keys: the old tolerance is itself near that floor), and fp32 with |lse| about 50, where the K-sum of S costs C u32 |S| in the
    exponent.  fp32 at a common offset is run at C = 16 only: at (3, 36, 64) the median for o is 1.62, the old fp32 tolerance of 1e-4 being
    tighter there than the worst case of a 64-term same-sign K-sum.
    The weakest rejection of a planted defect over all cases: p_tile 19.7, key 6.3, alpha 15.1, dq_block 43, delta_row 112,
    ds_scale 534 times the bound."""
    B, T, C = shape
    for dt in _att_dtypes(shape):
        if regime == "smallgrad" and dt != F16:
            continue
        route = A.attn_route(B, T, C, dt)
        print(f"  {shape} {regime} dtype {dt} route {route}")
        qkv, do = A.attention_inputs(regime, B, T, C, dt)
        check_regime_property(regime, qkv, B, T, C)
        x = R.attention_exact(qkv, B, T, C, do)
        lo, ll, lq = R.attn_layout(B, T, C, "o"), R.attn_layout(B, T, C, ()), R.attn_layout(B, T, C, "qkv")
        ro, rl = R.attention_forward(qkv, B, T, C, dt, route, parts=x)
        o, lse = restate_forward(qkv, B, T, C, dt, route)
        R.assert_within(o, ro, what="attention o", layout=lo)
        R.assert_within(lse, rl, what="attention lse", layout=ll)
        _vacuity("o", ro.e, ro.v.abs().max(), dt)
        o_emu, lse_emu = x["o"].float().to(TD[dt]).view(B * T, C), x["lse"].float().reshape(-1)
        gscale = torch.cat((x["dq"], x["dk"], x["dv"]), -1).abs().max()
        for tag, oi, li in (("emulated", o_emu, lse_emu), ("own", o, lse)):
            rg = R.attention_backward(qkv, oi, do, li, B, T, C, dt, route, parts=x)
            assert (rg.e > 0).all()
            dqkv, delta = restate_backward(qkv, oi, do, li, B, T, C, dt, route)
            for s, i in SECTION.items():
                sl = slice(i * C, (i + 1) * C)
                R.assert_within(dqkv[:, sl], V_(rg, sl), what=f"attention d{s} ({tag} inputs)", layout=R.attn_layout(B, T, C, s))
            R.assert_within(dqkv, rg, what=f"attention dqkv ({tag} inputs)", layout=lq)
            if delta is not None:
                R.assert_within(delta, R.rowdot(do, oi, B * T, C), what="delta", layout=ll)
        for s, i in SECTION.items():
            _vacuity("d" + s, rg.e[:, i * C:(i + 1) * C], gscale, dt)
        for kind in ATT_DEFECTS[route]:
            if kind == "alpha" and regime != "rising":
                continue  # defined where the maximum grows across blocks
            sec, term, where = A.attention_defect(kind, qkv, do, B, T, C, image=B - 1)
            if sec == "o":
                w = R.assert_rejects(o.double() + term, ro, what=f"{kind} ({where})")
            else:
                sl = slice(SECTION[sec] * C, (SECTION[sec] + 1) * C)
                w = R.assert_rejects(dqkv[:, sl].double() + term, V_(rg, sl), what=f"{kind} ({where})")
            print(f"    defect {kind} at {where}: err/bound {w:.3g}")
        R.assert_rejects(A.stale_upper_half(dqkv, B, T, C, "v", image=B - 1), rg, what="upper half of dv stale")


def V_(ref, sl):
    return R.V(ref.v[:, sl], ref.e[:, sl])


def test_attention_reference_equals_the_loop_and_float64_autograd():
    B, T, C = 2, 5, 8
    qkv, do = rnd((B * T, 3 * C), F32, 1, 1.5), rnd((B * T, C), F32, 2)
    x = R.attention_exact(qkv, B, T, C, do)
    Q = qkv.double().view(B, T, 3 * C).numpy()
    o, lse = np.zeros((B, T, C)), np.zeros((B, T))
    for b in range(B):
        for i in range(T):
            s = np.array([sum(Q[b, i, c] * Q[b, j, C + c] for c in range(C)) / math.sqrt(C) for j in range(T)])
            w = np.exp(s - s.max())
            lse[b, i] = s.max() + math.log(w.sum())
            for c in range(C):
                o[b, i, c] = sum(w[j] / w.sum() * Q[b, j, 2 * C + c] for j in range(T))
    np.testing.assert_allclose(x["o"].numpy(), o, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(x["lse"].numpy(), lse, rtol=1e-12, atol=1e-12)
    p = qkv.double().view(B, T, 3 * C).clone().requires_grad_(True)
    q, k, v = p.split(C, dim=-1)
    out = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(C), -1) @ v
    (g,) = torch.autograd.grad(out, p, do.double().view(B, T, C))
    for route, dt in ((R.VALU, F32), (R.VALU, BF16)):
        ro, rl = R.attention_forward(qkv, B, T, C, dt, route)
        rg = R.attention_backward(qkv, x["o"].float(), do, x["lse"].float(), B, T, C, dt, route)
        np.testing.assert_allclose(ro.v.numpy(), o.reshape(B * T, C), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(rl.v.numpy(), lse.reshape(-1), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(rg.v.numpy(), g.reshape(B * T, 3 * C).numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(R.rowdot(do, x["o"].float(), B * T, C).v.numpy(), x["delta"].reshape(-1).numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(R.rowdot(do, do, B * T, C).v.numpy(), (do.double() ** 2).sum(-1).numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("dt", [BF16, F16])
def test_attention_bound_rejects_the_two_numerical_mutants(dt):
    """the alpha multiply of attention_mfma.hip:303 skipped; the upper wave half's column tiles starting at ctm + 1 -- as switches of
    the restatements; the failure message names the 64-token block / the wave half"""
    B, T, C = 2, 256, 512
    qkv, do = A.attention_inputs("rising", B, T, C, dt)
    # only the queries of 64-token block 2 keep the rising direction; the others look down it: their maximum is in key block 0 and
    # alpha = 1 afterwards, so the mutant's damage is confined to the rows of that block
    X = qkv.double().view(B, T, 3 * C).clone()
    others = torch.ones(T, dtype=torch.bool)
    others[128:192] = False
    X[:, others, :C] -= 2 * (2.0 * C ** 0.25) / math.sqrt(C)
    qkv = X.view(B * T, 3 * C).to(TD[dt])
    ro, _ = R.attention_forward(qkv, B, T, C, dt, R.BLOCKS)
    lay = R.attn_layout(B, T, C, "o")
    R.assert_within(restate_forward(qkv, B, T, C, dt, R.BLOCKS)[0], ro, what="unmutated", layout=lay)
    o, _ = restate_forward(qkv, B, T, C, dt, R.BLOCKS, mutate="no_alpha")
    with pytest.raises(AssertionError) as ei:
        R.assert_within(o, ro, what="no alpha", layout=lay)
    assert "64-token block 2 of 4" in str(ei.value) and "section o" in str(ei.value), str(ei.value)
    rows = (R.ratio(o, ro) > 1).any(1).view(B, T)
    assert rows[:, 128:192].all() and not rows[:, others].any()  # every row of that block in both images, and no other
    B, T, C = 3, 64, 352  # odd ctm
    for regime in ("randn", "peaked"):
        qkv, do = A.attention_inputs(regime, B, T, C, dt)
        x = R.attention_exact(qkv, B, T, C, do)
        ro, rl = R.attention_forward(qkv, B, T, C, dt, R.T64, parts=x)
        o, lse = restate_forward(qkv, B, T, C, dt, R.T64, mutate="ctm+1", prev=0.0)
        with pytest.raises(AssertionError) as ei:
            R.assert_within(o, ro, what="ctm + 1", layout=R.attn_layout(B, T, C, "o"))
        assert "upper wave half's column tiles" in str(ei.value), str(ei.value)
        cols = (R.ratio(o, ro) > 1).any(0).nonzero().reshape(-1)
        assert cols.min() >= 16 * 11 and cols.max() < 16 * 12 and len(cols) == 16  # exactly the tile the mutant skips
        rg = R.attention_backward(qkv, o, do, lse, B, T, C, dt, R.T64, parts=x)
        good, _ = restate_backward(qkv, o, do, lse, B, T, C, dt, R.T64)
        bad, _ = restate_backward(qkv, o, do, lse, B, T, C, dt, R.T64, mutate="ctm+1", prev=good[:, 3 * C - 16:].float().view(B, T, 16))
        with pytest.raises(AssertionError) as ei:  # the previous content: the neighbouring tile's values, of the right size
            R.assert_within(bad, rg, what="ctm + 1", layout=R.attn_layout(B, T, C, "qkv"))
        assert "upper wave half's column tiles" in str(ei.value), str(ei.value)


def test_attention_locator_names_token_section_strip_block_and_half():
    B, T, C = 2, 256, 64
    lay = R.attn_layout(B, T, C, "qkv")
    ref = torch.zeros((B * T, 3 * C), dtype=torch.float64)
    got = ref.clone()
    got[1 * T + 250, 1 * C + 40] = 1.0
    with pytest.raises(AssertionError) as ei:
        R.assert_within(got, ref, torch.full_like(ref, 1e-3), "probe", layout=lay)
    msg = str(ei.value)
    assert "image 1, token 250, section k, channel 40" in msg and "last 16-row strip" in msg and "last 64-key block" in msg
    assert "upper wave half's column tiles" in msg and "64-token block 3 of 4" in msg
    got = torch.zeros(B * T, dtype=torch.float64)
    got[3] = 1.0
    with pytest.raises(AssertionError) as ei:
        R.assert_within(got, torch.zeros_like(got), torch.full_like(got, 1e-3), "probe", layout=R.attn_layout(B, T, C, ()))
    assert "image 0, token 3" in str(ei.value) and "first 16-row strip" in str(ei.value)
