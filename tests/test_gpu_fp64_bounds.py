"""Element-wise float64 bounds (tests/fp64_ref.py) on the fp32 atomicAdd paths that feed parameter gradients and losses.

  * the geometry of the one unexplained wrong bias gradient (descent.3.2.project.0.bias, fp16, C = 52, B = 2): ln_backward's dm at
    384 channels @16^2 with per-sample modulation rows (level 3 of the default network: the fused LayerNorm backward is 128-channel
    only, so this level takes ln_bwd_kernel) and at 512 @8^2; the weight / bias gradients of the 384->384 @16^2 and 512->512 @8^2
    convs with and without a workspace (without one, dW and dbias are combined with atomics);
  * the same at B = 128, where the atomics come from many workgroups;
  * the fused LayerNorm-backward dm of the conv epilogue (conv_epilogue.h:362) at the bench's 128 @64^2 case;
  * the loss sums (fused into the output conv, conv_patch3.hip:375; mse_loss_grad, sq_err), colsum and sumsq, each at a size with
    thousands of atomic adders on one address.

Every call is made twice onto a destination that already holds non-zero values: the first result must be the old value plus the
reference, the second the first result plus the reference, each within its bound.  Each case also plants its defect (a tile or a
256-pixel block missing) in fp64 on the kernel's output and checks that the bound rejects it.  The references are computed for every
image in full (no subset of images): at these sizes the fp64 work is well under a second per case.
"""
import math

import pytest
import torch

import fp64_ref as R
import test_fp64_bounds_cpu as CB  # the chain form's operands and the four forms, shared with the CPU tier
from climate2weather_amd import _lib, ops

pytestmark = pytest.mark.gpu

BF16, F16 = ops.DTYPE_BF16, ops.DTYPE_F16
TD = ops.TORCH_DTYPE
S1 = ops.CONV_S1


def dev():
    return torch.device("cuda:0")


def rnd(shape, dt, seed, scale=1.0):
    g = torch.Generator(device=dev()).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=dev()) * scale).to(TD[dt])


def geom(B, H, C):
    return dict(B=B, Hin=H, Win=H, Cin=C, Hout=H, Wout=H, Cout=C, ldy=C, wrows=C, mode=S1)


def twice(call, dest, ref, what, defect):
    """call() accumulates onto dest (non-zero); checks dest = old + ref after each of two calls, and rejects the planted defect"""
    worst = 0.0
    for k in (1, 2):
        old = dest.clone()
        call()
        torch.cuda.synchronize()
        want = R.accumulated(old, ref)
        worst = max(worst, R.assert_within(dest, want, what=f"{what} (call {k})"))
    R.assert_rejects(dest.double() - defect, want, what=f"{what}: planted defect")
    R.report(what, worst)
    return want


@pytest.fixture(autouse=True)
def _knobs_follow_the_environment():
    yield
    ops.knobs_reload()


LN_CASES = [(384, 16), (512, 8)]


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("B", [2, 128])
@pytest.mark.parametrize("C,H", LN_CASES)
def test_layernorm_backward_modulation_gradient(C, H, B, dt):
    """ln_bwd_kernel's dm (pointwise.hip:172-193: one atomic sweep per block) with per-sample modulation rows: the per-sample sum that
    becomes project.0.bias's gradient"""
    HW, npix, ldm = H * H, B * H * H, C + 64
    x, dy, dres = rnd((npix, C), dt, 1), rnd((npix, C), dt, 2), rnd((npix, C), dt, 3)
    m = rnd((B, ldm), F16, 4).float()
    dm = rnd((B, ldm), F16, 5).float()  # already holds values: the kernel accumulates
    dx = torch.empty_like(x)
    mm = m.view(-1)[32:]
    rdx, rdm = R.ln_backward(dy, x, mm, dres, npix, HW, C, ldm, 1e-5, True, dt)
    n = min(128, HW)
    _, tile = R.ln_backward(dy[:n], x[:n], mm, None, n, n, C, ldm, 1e-5, True, dt)  # the first 8x16 (or 8x8) pixels of image 0
    defect = torch.zeros_like(rdm.v)
    defect[0] = tile.v[0]
    dmv = dm[:, 32:32 + C]

    def call():
        ops.ln_backward(dy, x, mm, dres, dx, dm.view(-1)[32:], npix, HW, C, ldm, 1e-5, True, dt)

    twice(call, dmv, rdm, f"ln_backward dm {C}@{H}^2 B={B} dt={dt}", defect)
    R.report(f"ln_backward dx {C}@{H}^2 B={B} dt={dt}", R.assert_within(dx, rdx, what="ln_backward dx"))
    assert (dm[:, :32] == rnd((B, ldm), F16, 5).float()[:, :32]).all()  # nothing written outside the modulation rows


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("workspace", [False, True])
@pytest.mark.parametrize("B", [2, 128])
@pytest.mark.parametrize("C,H", LN_CASES)
def test_weight_and_bias_gradient_through_atomics_and_workspace(C, H, B, workspace, dt):
    """c2w_conv_wgrad of the 384->384 @16^2 and 512->512 @8^2 convs; without a workspace dW and dbias are combined with fp32 atomics
    (wgrad_patch.hip:394,423; wgrad.hip:288,304)"""
    g = geom(B, H, C)
    x, dy = rnd((B * H * H, C), dt, 1), rnd((B * H * H, C), dt, 2)
    nw = C * 9 * C
    dw = rnd((nw,), F16, 3).float() * 0.1
    db = rnd((C,), F16, 4).float()
    ws = ops.new_workspace(dev()) if workspace else None
    rw, rb = R.wgrad(x, dy, g)
    rw = rw.view(-1)
    tw, tb = R.wgrad(x, dy, g, images=(0, 1), pixels=R.tile_mask(H, H, tw=min(16, H)))  # one 8x16 tile of image 0
    what = f"wgrad {C}->{C} @{H}^2 B={B} {'workspace' if workspace else 'atomics'} dt={dt}"

    def call():
        ops.conv_wgrad(x, dy, dw, g, dt, dbias=db, workspace=ws)

    # the two outputs of one call: dW checked through twice(), dbias after each of the same calls
    db_old = [db.clone()]
    worst_b = [0.0]

    def call_both():
        db_old[0] = db.clone()
        call()
        torch.cuda.synchronize()
        worst_b[0] = max(worst_b[0], R.assert_within(db, R.accumulated(db_old[0], rb), what=what + " bias"))

    want_w = twice(call_both, dw, rw, what, tw.v.reshape(-1))  # (the planted defect: the tile missing)
    R.report(what + " bias", worst_b[0])
    want_b = R.accumulated(db_old[0], rb)
    R.assert_rejects(dw.double() + tw.v.reshape(-1), want_w, what=what + ": one tile twice")
    R.assert_rejects(db.double() - tb.v, want_b, what=what + " bias: one tile missing")
    R.assert_rejects(db.double() + tb.v, want_b, what=what + " bias: one tile twice")


@pytest.mark.parametrize("dt", [F16, BF16])
def test_fused_layernorm_backward_modulation_gradient_at_the_bench_case(dt):
    """conv_epilogue.h:349-362: the column sums of a tile reduced in LDS, one atomic per channel and workgroup (res 128@64^2, B = 64)"""
    B, H, C = 64, 64, 128
    g = geom(B, H, C)
    assert ops.conv_lnbwd_supported(g, dt)
    npix = B * H * H
    x = rnd((npix, C), dt, 1)
    w = rnd((C, 9, C), dt, 2, scale=1.0 / math.sqrt(9 * C))
    lnx, res = rnd((npix, C), dt, 7), rnd((npix, C), dt, 4)
    m = rnd((B, C + 64), F16, 6).float()
    dm = rnd((B, C + 64), F16, 5).float()
    y = torch.empty((npix, C), dtype=TD[dt], device=dev())
    ln = dict(x=lnx, m=m.view(-1)[32:], ldm=C + 64, eps=1e-5, unbiased=True)
    ref = R.conv(x, w, g, dt, res=res, ln=ln)
    # defect: the first 8x16 tile of image 0 missing -- the sum of its rows, from the same reference on image 0 alone
    o = _ln_rows_of_image0(x, w, geom(1, H, C), dt, lnx, m, C)
    defect = torch.zeros_like(ref["dm"].v)
    defect[0] = o.v.view(H, H, C)[:8, :16].sum((0, 1))
    dmv = dm[:, 32:32 + C]

    def call():
        ops.conv(x, w, None, y, g, dt, res=res, ln=dict(ln, dm=dm.view(-1)[32:]))

    twice(call, dmv, ref["dm"], f"fused LN backward dm 128@64^2 B=64 dt={dt}", defect)
    R.report(f"fused LN backward dx 128@64^2 B=64 dt={dt}", R.assert_within(y, ref["y"], what="fused LN backward dx", layout=R.layout(g)))


def _ln_rows_of_image0(x, w, gi, dt, lnx, m, C):
    """the fp32 rows o of the fused LayerNorm backward on image 0 (before the residual): what dm sums"""
    H = gi["Hout"]
    a = R._rnd(R.conv_sum(x[:H * H], w, gi), TD[dt])
    u = R._add(R.exact(lnx[:H * H]), R.V(m[0, 32:32 + C].double().expand(H * H, C)))
    return R.ln_backward_rows(a, u, C, 1e-5, True)


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("C", [52, 65])
def test_fused_loss_sum_of_the_output_convolution(C, dt):
    """conv_patch3.hip:340-375: sum (prediction - eps)^2 with one atomic per workgroup (1024 workgroups at B = 16, 128^2)"""
    B, H = 16, 128
    g = dict(geom(B, H, 128), wrows=C)
    assert ops.conv_loss_supported(g, dt)
    npix, lde = B * H * H, (C + 7) // 8 * 8
    x = rnd((npix, 128), dt, 1)
    w = rnd((C, 9, 128), dt, 2, scale=1.0 / math.sqrt(9 * 128))
    bias = rnd((C,), F16, 3).float()
    er = torch.zeros((npix, lde), dtype=torch.float16, device=dev())
    er[:, :C] = rnd((npix, C), F16, 9)
    y = torch.empty((npix, 128), dtype=TD[dt], device=dev())
    ops.conv(x, w, bias, y, g, dt)  # the prediction as stored: the fused kernel squares the same values (test_gpu_bench_dispatch)
    ls = torch.full((1,), 1234.5, device=dev())
    dy = torch.empty_like(y)
    lf = dict(sum=ls, eps=er, lde=lde, gscale=2.0 / (B * C * H * H), C=C)
    ref = R.fused_loss_sum(y, er, C, lde, npix, B * (H // 16) * (H // 16))
    block = R.fused_loss_sum(y[:256], er[:256], C, lde, 256, 1).v  # one 256-pixel block
    twice(lambda: ops.conv(x, w, bias, dy, g, dt, loss=lf), ls, ref.view(1), f"fused loss sum C={C} dt={dt}", block.view(1))


@pytest.mark.parametrize("dt", [F16, BF16])
def test_loss_sums_colsum_and_sumsq(dt):
    """mse_loss_grad / sq_err (pointwise.hip:581/653, 2048 blocks: 8192 atomics on one address), colsum (pointwise.hip:230, 2048 row
    blocks per channel), sumsq (sampler.hip:80, 8192 atomics)"""
    B, C, HW, ldc = 16, 52, 128 * 128, 64
    y = rnd((B * HW, ldc), dt, 1)
    eps = rnd((B, C, HW), F16, 2).float()
    ref = R.mse_loss_sum(y, eps, B, C, HW, ldc).view(1)
    block = R.mse_loss_sum(y[:256], eps[:1, :, :256].contiguous(), 1, C, 256, ldc).v.view(1)
    ls = torch.full((1,), 777.25, device=dev())
    dy = torch.empty_like(y)
    gs = 2.0 / (B * C * HW)
    twice(lambda: ops.mse_loss_grad(y, eps, dy, ls, B, C, HW, ldc, gs, dt), ls, ref, f"mse_loss_grad loss sum dt={dt}", block)
    R.report(f"mse_loss_grad dy dt={dt}", R.assert_within(dy, R.mse_dy(y, eps, B, C, HW, ldc, gs, dt), what="mse_loss_grad dy"))
    out = torch.empty(B * C * HW, device=dev())
    ls2 = torch.full((1,), -55.5, device=dev())
    assert ops.sq_err(y, eps, out, ls2, B, C, HW, ldc, dt)
    ls2.fill_(-55.5)
    twice(lambda: ops.sq_err(y, eps, out, ls2, B, C, HW, ldc, dt), ls2, R.sq_err_sum(y, eps, B, C, HW, ldc).view(1),
          f"sq_err loss sum dt={dt}", block)
    rows, Cc = 1 << 22, 64
    a = rnd((rows, Cc), dt, 3)
    cs = rnd((Cc,), F16, 4).float()
    twice(lambda: ops.colsum(a, cs, rows, Cc, Cc, dt), cs, R.colsum(a, rows, Cc, Cc, dt), f"colsum {rows}x{Cc} dt={dt}",
          a[:256].double().sum(0))
    n = 1 << 20  # 2048 blocks of 4 waves: 8192 atomics; a 256-element block is 2.4e-4 of the sum
    v = rnd((n,), F16, 5).float()
    s = torch.full((1,), 3.0, device=dev())
    twice(lambda: ops.sumsq(v, s, n), s, R.sumsq(v, n).view(1), f"sumsq n={n}", (v[:256].double() ** 2).sum().view(1))


# ------------------------------------------------------------------------------ kept statistics and the chain form at small shapes

def _s1(B, H, W, C):
    return dict(B=B, Hin=H, Win=W, Cin=C, Hout=H, Wout=W, Cout=C, ldy=C, wrows=C, mode=S1)


KEPT_CASES = [  # (B, H, W, per-sample rows, kernel family, knob)
    (3, 16, 16, False, "PATCH_8X16", None),
    (2, 32, 48, True, "PATCH_8X16", None),
    (2, 32, 32, False, "PATCH_16X16", ("C2W_CONV_T3", "16")),
]


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("use_res", [True, False])
@pytest.mark.parametrize("unbiased", [True, False])
@pytest.mark.parametrize("case", KEPT_CASES, ids=["8x16-shared", "8x16-rows", "16x16"])
def test_fused_layernorm_backward_from_kept_statistics(case, unbiased, use_res, dt, monkeypatch):
    """finish_ln_rows_stored (conv_epilogue.h:311-359; EPI 6 of the 16x16-tile kernel and the same branch of the 8x16-tile kernel): the
    operands are the normalised rows and 1/sigma of a real LayerNorm of random rows; image 0 has constant rows (xhat = 0,
    rstd = 1/sqrt(eps)).  dx inside its bound; dm accumulated twice onto non-zero values, with one 8x16 tile of image 0 missing as the
    planted defect; nothing written outside the modulation rows.
    Measured worst err/bound: dx 0.855 (8x16-tile kernel), 0.772 (16x16); dm 0.102."""
    B, H, W, rows, fam, kn = case
    C = 128
    if kn:
        monkeypatch.setenv(*kn)
        ops.knobs_reload()
    g = _s1(B, H, W, C)
    assert ops.conv_lnbwd_supported(g, dt) and ops.conv_dispatch(g, dt, fused_ln=True) == getattr(_lib, "KERNEL_" + fam)
    npix, HW = B * H * W, H * W
    x = rnd((npix, C), dt, 1)
    w = rnd((C, 9, C), dt, 2, scale=1.0 / math.sqrt(9 * C))
    res = rnd((npix, C), dt, 4) if use_res else None
    u = rnd((npix, C), dt, 7).float()
    u[:HW] = 0.75
    var, mean = torch.var_mean(u, dim=1, unbiased=unbiased, keepdim=True)
    rs = (var + 1e-5).rsqrt()
    xh, rs = ((u - mean) * rs).to(TD[dt]), rs.view(-1).contiguous()
    assert rs[:HW].min().item() == pytest.approx(1e-5 ** -0.5, rel=1e-6) and xh[:HW].abs().max().item() == 0.0
    ldm = C + 64 if rows else 0
    buf = rnd((B if rows else 1, C + 64), ops.DTYPE_F32, 6)
    guard = buf.clone()
    dm = buf.view(-1)[32:]
    ln = dict(x=xh, rstd=rs, ldm=ldm, eps=1e-5, unbiased=unbiased)
    y = torch.full((npix, C), 7.0, dtype=TD[dt], device=dev())
    ref = R.conv(x, w, g, dt, res=res, ln=ln)
    tile = ref["o"].v.view(B, H, W, C)[0, :8, :16].sum((0, 1))
    defect = torch.zeros_like(ref["dm"].v)
    defect[0] = tile
    got = buf[:, 32:32 + C]
    what = f"kept statistics {case[:4]} unbiased={unbiased} res={use_res} dt={dt}"
    twice(lambda: ops.conv(x, w, None, y, g, dt, res=res, ln=dict(ln, dm=dm)), got, ref["dm"], what + " dm", defect)
    R.report(what + " dx", R.assert_within(y, ref["y"], what=what + " dx", layout=R.layout(g)))
    assert torch.equal(buf[:, :32], guard[:, :32]) and torch.equal(buf[:, 32 + C:], guard[:, 32 + C:])


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("shape", [(2, 32, 32), (1, 16, 48)])
@pytest.mark.parametrize("form", list(CB.CHAIN_FORMS))
def test_chain_form_at_small_shapes(form, shape, packed, dt, monkeypatch):
    """finish_lnf<RESN> (conv_epilogue.h:417-513; EPI 2 and 8 of the 16x16-tile kernel) under C2W_CONV_T3=16: the emitted LayerNorm rows,
    their 1/sigma and mean and -- where it is written -- the output, each element inside its float64 bound; with C2W_CONV_NO_Y the output
    buffer keeps its fill to the byte.  The last image's block input is constant (h = 0: the rebuilt residual is mean - m).
    Measured worst err/bound: hn 0.685, rstd 0.136, mean 0.162, y 0.978."""
    B, H, W = shape
    C = 128
    monkeypatch.setenv("C2W_CONV_T3", "16")
    ops.knobs_reload()
    g = _s1(B, H, W, C)
    assert ops.conv_lnfwd_chain_supported(g, dt) and ops.conv_dispatch(g, dt, fused_ln=True) == _lib.KERNEL_PATCH_16X16
    npix, HW = B * H * W, H * W
    x = rnd((npix, C), dt, 1)
    w = rnd((C, 9, C), dt, 2, scale=1.0 / math.sqrt(9 * C))
    bias = rnd((C,), ops.DTYPE_F32, 3)
    wop = w
    if packed:
        wop = torch.empty(ops.packed_conv_weights_numel(C, C), dtype=TD[dt], device=dev())
        ops.pack_conv_weights_batched(w, wop, torch.tensor([[0, 0, C, C]], dtype=torch.int64, device=dev()), 1, dt)
    const = slice(npix - HW, npix) if B > 1 else slice(npix // 2, npix // 2 + 32)
    co = tuple(t.to(dev()) for t in CB._chain_operands(npix, HW, C, dt, C + 64, const=const))
    assert co[0][const].abs().max().item() == 0.0
    y, hn, rstd, mu, kw = CB.chain_launch(lambda *a, **k: ops.conv(*a, wpacked=packed, **k), form, x, wop, bias, g, dt, co)
    torch.cuda.synchronize()
    ref = R.conv(x, w, g, dt, bias=bias, **kw)
    what = f"chain form [{form}] {shape} packed={packed} dt={dt}"
    if CB.CHAIN_FORMS[form]["no_y"]:
        assert "y" not in ref and bool((y == 3.0).all())  # not a byte of the output buffer was touched
    else:
        R.report(what + " y", R.assert_within(y, ref["y"], what=what + " y", layout=R.layout(g)))
    R.report(what + " hn", R.assert_within(hn, ref["hn"], what=what + " hn", layout=R.layout(g)))
    R.report(what + " rstd", R.assert_within(rstd, ref["rstd"], what=what + " rstd"))
    R.report(what + " mean", R.assert_within(mu, ref["mean"], what=what + " mean"))
