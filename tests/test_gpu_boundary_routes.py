"""The routes of the layout, loss, window and guidance launchers (csrc/pointwise.hip, csrc/sampler.hip) that no other kernel test takes:
the untiled kernels (ldc >= 256, or rows that are no multiple of the 16-byte vector), partial 64-pixel tiles, more tiles than the grid
cap (the second trip through a workgroup's tile loop), the device-resident loss scale, the per-thread window gather, and guidance /
pooling on non-square fields with cells of 1, 9 and 144 pixels.

Every output buffer sits between two guard regions that must keep their fill; padding channels [C, ldc) must be exactly zero.  Layout
changes are exact (torch's own casts round to nearest even, like v_cvt_pk_*); arithmetic is held to float64 bounds built with
fp64_ref's V rules.  The noise tensor the reading kernels get is the materialised stream (c2w_philox_normal, itself pinned to its float64
definition by tests/test_gpu_noise_stream.py), so that the regenerating twins can be required to give the same bits."""
import numpy as np
import pytest
import torch

import fp64_noise_ref as N
import fp64_ref as R
from fp64_guidance_ref import _cells, _chain, _div, _uncells, guidance_correction  # shared with tests/launch_replay.py
from climate2weather_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, F16 = ops.DTYPE_F32, ops.DTYPE_BF16, ops.DTYPE_F16
TD = ops.TORCH_DTYPE
ALL = [F32, BF16, F16]
GUARD = 512  # elements on either side of every output
FILL = 7.0

PARTIAL = [(3, 5, 100, 8), (2, 8, 100, 8), (2, 1, 36, 8), (2, 6, 225, 8)]  # HW = 100: tiles of 64 + 36; C == ldc; C = 1; HW % 4 != 0
UNTILED = [(2, 250, 100, 256), (2, 256, 49, 256)]                         # ldc * 65 * 4 bytes > 64 KiB of LDS
OVER_LOSS_CAP = (6, 3, 44820, 8)     # 701 tiles per image (the last: 20 pixels), 4206 in all: > 2048 (mse_loss_grad*) and > 4096 (sq_err*)
OVER_LAYOUT_CAP = (6, 2, 699076, 8)  # 10924 tiles per image (the last: 4 pixels), 65544 in all: > 65536


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else {F32: "fp32", BF16: "bf16", F16: "fp16"}.get(v, str(v))


def guarded(n, dtype, fill=FILL):
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return whole, whole[GUARD: GUARD + n]


def intact(whole, fill=FILL):
    return bool((whole[:GUARD] == fill).all() and (whole[-GUARD:] == fill).all())


def untouched(whole, fill=FILL):
    return bool((whole == fill).all())


def tiled(ldc):
    return ldc * 65 * 4 <= 64 * 1024


def make(B, C, HW, ldc, dt, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * C * HW, generator=g).view(B, C, HW).to(DEV)
    musig = (torch.rand(B, 2, generator=g) + 0.1).to(DEV)
    nseed = 0x5DEECE66D00000 + seed
    eps = torch.empty(B, C, HW, device=DEV)
    ops.philox_normal(eps, eps.numel(), nseed)
    return x, musig, eps, nseed


def rows_of(t, ldc, dtype):
    """(B, C, HW) -> NHWC rows (B * HW, ldc) of dtype with zero padding channels"""
    B, C, HW = t.shape
    out = torch.zeros(B * HW, ldc, dtype=dtype, device=t.device)
    out[:, :C] = t.permute(0, 2, 1).reshape(B * HW, C).to(dtype)
    return out


def random_rows(B, HW, ldc, dt, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(B * HW, ldc, generator=g, device=DEV).to(TD[dt])


# ------------------------------------------------------------------------------------------------------------ layout kernels

LAYOUT = [(s, dt) for s in PARTIAL + UNTILED for dt in ALL] + [(OVER_LAYOUT_CAP, dt) for dt in (F32, BF16)]


@pytest.mark.parametrize("shape,dt", LAYOUT, ids=[f"{_id(s)}-{_id(d)}" for s, d in LAYOUT])
def test_nchw_to_nhwc_routes(shape, dt):
    B, C, HW, ldc = shape
    x, musig, eps, nseed = make(B, C, HW, ldc, dt, 1)
    n = B * HW * ldc
    whole, y = guarded(n, TD[dt])
    ops.nchw_to_nhwc(x, None, None, y, B, C, HW, ldc, dt)
    assert torch.equal(y.view(B * HW, ldc), rows_of(x, ldc, TD[dt])) and intact(whole)
    del whole, y
    whole, y = guarded(n, TD[dt])
    ops.nchw_to_nhwc(x, eps, musig, y, B, C, HW, ldc, dt)
    yr = y.view(B * HW, ldc)
    want = N.xt_rows(x, eps, musig, dt, 0.0)
    R.report(f"nchw_to_nhwc(eps) {_id(shape)} {_id(dt)}", R.assert_within(yr[:, :C], want, what="nchw_to_nhwc(eps)"))
    assert (yr[:, C:] == 0).all() and intact(whole)
    R.assert_rejects(yr[:, :C], N.xt_rows(x.roll(1, 2), eps, musig, dt, 0.0), what="pixels shifted by one")
    del want
    whole2, y2 = guarded(n, TD[dt])
    off = torch.arange(B, dtype=torch.int64, device=DEV) * (C * HW)
    if tiled(ldc):  # the regenerating twin, dense and through window offsets: the same bits
        assert ops.nchw_to_nhwc_noise(x, nseed, musig, y2, B, C, HW, ldc, dt)
        assert torch.equal(y2, y) and intact(whole2)
        y2.fill_(FILL)
        assert ops.windows_to_nhwc_noise(x, off, nseed, musig, y2, B, C, HW, ldc, dt)
        assert torch.equal(y2, y) and intact(whole2)
    else:           # "unsupported": the caller materialises the stream; nothing may have been written
        assert ops.nchw_to_nhwc_noise(x, nseed, musig, y2, B, C, HW, ldc, dt) is False
        assert ops.windows_to_nhwc_noise(x, off, nseed, musig, y2, B, C, HW, ldc, dt) is False
        torch.cuda.synchronize()
        assert untouched(whole2)


BACK = LAYOUT + [((2, 52, 100, 52), BF16), ((2, 52, 100, 52), F16)]  # rows of 104 bytes: no multiple of the 16-byte vector


@pytest.mark.parametrize("shape,dt", BACK, ids=[f"{_id(s)}-{_id(d)}" for s, d in BACK])
def test_nhwc_to_nchw_routes(shape, dt):
    B, C, HW, ldc = shape
    y = random_rows(B, HW, ldc, dt, 2)  # live values in the padding channels too: a read past C shows
    whole, out = guarded(B * C * HW, torch.float32)
    ops.nhwc_to_nchw(y, out, B, C, HW, ldc, dt)
    want = y[:, :C].float().view(B, HW, C).permute(0, 2, 1)
    assert torch.equal(out.view(B, C, HW), want) and intact(whole)


# -------------------------------------------------------------------------------------------------------------- loss kernels

LOSS = [(s, dt) for s in PARTIAL + [OVER_LOSS_CAP] + UNTILED for dt in ALL]
GSCALE = 0.37


def _det_scratch():
    return torch.empty(ops.loss_det_scratch_bytes() // 4, device=DEV)


@pytest.mark.parametrize("shape,dt", LOSS, ids=[f"{_id(s)}-{_id(d)}" for s, d in LOSS])
def test_mse_loss_grad_routes(shape, dt):
    B, C, HW, ldc = shape
    _, _, eps, nseed = make(B, C, HW, ldc, dt, 3)
    y = random_rows(B, HW, ldc, dt, 4)
    n = B * HW * ldc
    want_dy = R.mse_dy(y, eps, B, C, HW, ldc, GSCALE, dt)  # padding channels: value 0, bound 0
    want_ls = R.mse_loss_sum(y, eps, B, C, HW, ldc)
    scratch = _det_scratch()
    whole, dy = guarded(n, TD[dt])
    ls = torch.zeros(1, device=DEV)
    ops.mse_loss_grad(y, eps, dy, ls, B, C, HW, ldc, GSCALE, dt)
    R.report(f"mse_loss_grad dy {_id(shape)} {_id(dt)}", R.assert_within(dy, want_dy, what="mse_loss_grad dy"))
    R.report(f"mse_loss_grad loss {_id(shape)} {_id(dt)}", R.assert_within(ls, want_ls, what="mse_loss_grad loss"))
    assert (dy.view(B * HW, ldc)[:, C:] == 0).all() and intact(whole)
    R.assert_rejects(dy, R.mse_dy(y, eps.roll(1, 2), B, C, HW, ldc, GSCALE, dt), what="noise shifted by one pixel")
    runs = []
    for _ in range(2):  # the deterministic twin: the same dy, a loss sum with the same bits launch after launch
        whole_d, dy_d = guarded(n, TD[dt])
        ls_d = torch.zeros(1, device=DEV)
        ops.mse_loss_grad(y, eps, dy_d, ls_d, B, C, HW, ldc, GSCALE, dt, det=scratch)
        assert torch.equal(dy_d, dy) and intact(whole_d)
        runs.append(ls_d)
    assert torch.equal(runs[0], runs[1])
    R.report(f"mse_loss_grad_det loss {_id(shape)} {_id(dt)}", R.assert_within(runs[0], want_ls, what="mse_loss_grad_det loss"))
    whole_n, dy_n = guarded(n, TD[dt])
    ls_n = torch.full((1,), 3.0, device=DEV)
    if not tiled(ldc):
        assert ops.mse_loss_grad_noise(y, nseed, dy_n, ls_n, B, C, HW, ldc, GSCALE, dt) is False
        assert ops.mse_loss_grad_noise(y, nseed, dy_n, ls_n, B, C, HW, ldc, GSCALE, dt, det=scratch) is False
        torch.cuda.synchronize()
        assert untouched(whole_n) and ls_n.item() == 3.0
        return
    ls_n.zero_()
    assert ops.mse_loss_grad_noise(y, nseed, dy_n, ls_n, B, C, HW, ldc, GSCALE, dt)
    assert torch.equal(dy_n, dy) and intact(whole_n)
    R.report(f"mse_loss_grad_noise loss {_id(shape)} {_id(dt)}", R.assert_within(ls_n, want_ls, what="mse_loss_grad_noise loss"))
    runs = []
    for _ in range(2):
        dy_n.fill_(FILL)
        ls_d = torch.zeros(1, device=DEV)
        assert ops.mse_loss_grad_noise(y, nseed, dy_n, ls_d, B, C, HW, ldc, GSCALE, dt, det=scratch)
        assert torch.equal(dy_n, dy) and intact(whole_n)
        runs.append(ls_d)
    assert torch.equal(runs[0], runs[1])
    R.report(f"mse_loss_grad_noise_det loss {_id(shape)} {_id(dt)}", R.assert_within(runs[0], want_ls, what="mse_loss_grad_noise_det loss"))


@pytest.mark.parametrize("shape,dt", LOSS, ids=[f"{_id(s)}-{_id(d)}" for s, d in LOSS])
def test_sq_err_routes(shape, dt):
    B, C, HW, ldc = shape
    _, _, eps, nseed = make(B, C, HW, ldc, dt, 5)
    y = random_rows(B, HW, ldc, dt, 6)
    scratch = _det_scratch()
    whole, out = guarded(B * C * HW, torch.float32)
    ls = torch.full((1,), 3.0, device=DEV)
    if not tiled(ldc) or HW % 4:
        for e in (eps, nseed):
            assert ops.sq_err(y, e, out, ls, B, C, HW, ldc, dt) is False
            assert ops.sq_err(y, e, out, ls, B, C, HW, ldc, dt, det=scratch) is False
        torch.cuda.synchronize()
        assert untouched(whole) and ls.item() == 3.0
        return
    want = (y[:, :C].float().view(B, HW, C).permute(0, 2, 1) - eps) ** 2  # two exact fp32 operations on the stored values
    want_ls = R.sq_err_sum(y, eps, B, C, HW, ldc)
    for e, name in ((eps, "sq_err"), (nseed, "sq_err(seed)")):
        out.fill_(FILL)
        ls.zero_()
        assert ops.sq_err(y, e, out, ls, B, C, HW, ldc, dt)
        assert torch.equal(out.view(B, C, HW), want) and intact(whole)
        R.report(f"{name} loss {_id(shape)} {_id(dt)}", R.assert_within(ls, want_ls, what=f"{name} loss"))
        runs = []
        for _ in range(2):
            out.fill_(FILL)
            ls_d = torch.zeros(1, device=DEV)
            assert ops.sq_err(y, e, out, ls_d, B, C, HW, ldc, dt, det=scratch)
            assert torch.equal(out.view(B, C, HW), want) and intact(whole)
            runs.append(ls_d)
        assert torch.equal(runs[0], runs[1])
        R.report(f"{name} det loss {_id(shape)} {_id(dt)}", R.assert_within(runs[0], want_ls, what=f"{name} det loss"))


@pytest.mark.parametrize("dt", ALL, ids=_id)
def test_mse_loss_grad_with_a_device_resident_loss_scale(dt):
    """scaler state {scale, tracker, found_inf, steps} = {512, 0, 0, 0}: dy carries gscale * 512, the loss sum does not"""
    B, C, HW, ldc = 3, 5, 100, 8
    _, _, eps, nseed = make(B, C, HW, ldc, dt, 7)
    y = random_rows(B, HW, ldc, dt, 8)
    state = torch.tensor([512.0, 0.0, 0.0, 0.0], device=DEV)
    want_dy = R.mse_dy(y, eps, B, C, HW, ldc, GSCALE * 512, dt)
    want_ls = R.mse_loss_sum(y, eps, B, C, HW, ldc)
    whole, dy = guarded(B * HW * ldc, TD[dt])
    ls = torch.zeros(1, device=DEV)
    ops.mse_loss_grad(y, eps, dy, ls, B, C, HW, ldc, GSCALE, dt, scaler=state)
    R.report(f"mse_loss_grad(scaler) dy {_id(dt)}", R.assert_within(dy, want_dy, what="mse_loss_grad(scaler) dy"))
    R.report(f"mse_loss_grad(scaler) loss {_id(dt)}", R.assert_within(ls, want_ls, what="mse_loss_grad(scaler) loss"))
    assert intact(whole)
    R.assert_rejects(dy, R.mse_dy(y, eps, B, C, HW, ldc, GSCALE, dt), what="the loss scale ignored")
    whole_n, dy_n = guarded(B * HW * ldc, TD[dt])
    ls_n = torch.zeros(1, device=DEV)
    assert ops.mse_loss_grad_noise(y, nseed, dy_n, ls_n, B, C, HW, ldc, GSCALE, dt, scaler=state)
    assert torch.equal(dy_n, dy) and intact(whole_n)
    R.report(f"mse_loss_grad_noise(scaler) loss {_id(dt)}", R.assert_within(ls_n, want_ls, what="mse_loss_grad_noise(scaler) loss"))
    assert torch.equal(state, torch.tensor([512.0, 0.0, 0.0, 0.0], device=DEV))  # only read


# ------------------------------------------------------------------------------------------------- window gather and scatter

WINDOWS = [  # (L, F, k, H, W, i0, nw, ldc or None: the next multiple of 8)
    (5, 1, 1, 7, 7, 1, 2, None),     # F HW = 49: the image stride is no multiple of 4 floats -> per-thread gather
    (6, 3, 1, 5, 5, 0, 4, None),     # F HW = 75: the same, three variables
    (6, 4, 1, 7, 7, 2, 2, None),     # F HW = 196, HW = 49: the tiled kernel's scalar loads on overlapping windows
    (9, 2, 1, 10, 10, 0, 7, None),   # HW = 100: tiles of 64 + 36 pixels
    (4, 20, 1, 6, 6, 0, 2, 256),     # ldc = 256: no LDS tile -> per-thread gather
]


@pytest.mark.parametrize("dt", ALL, ids=_id)
@pytest.mark.parametrize("case", WINDOWS, ids=_id)
def test_window_gather_and_scatter_routes(case, dt):
    L, F, k, H, W, i0, nw, ldc = case
    w, HW = 2 * k + 1, H * W
    ldc = ldc or (w * F + 7) // 8 * 8
    nwin = L - w + 1
    assert i0 + nw <= nwin
    x = torch.randn(L, F, HW, generator=torch.Generator().manual_seed(L * F + HW)).to(DEV)
    want = torch.zeros(nw, HW, ldc, dtype=TD[dt], device=DEV)
    for j in range(nw):  # window j: frames i0 + j .. i0 + j + w - 1, channel = tau F + c
        want[j, :, : w * F] = x[i0 + j: i0 + j + w].reshape(w * F, HW).t().to(TD[dt])
    whole, y = guarded(nw * HW * ldc, TD[dt])
    ops.window_gather(x, y, nw, F, HW, k, i0, ldc, dt)
    assert torch.equal(y.view(nw, HW, ldc), want) and intact(whole)
    # fold the gathered rows back: the centre frame of every window, the leading k of window 0, the trailing k of the last one
    whole_e, e = guarded(L * F * HW, torch.float32, -3.0)
    ops.window_scatter(y, e, nw, F, HW, k, i0, nwin, ldc, dt)
    back = torch.full((L, F, HW), -3.0, device=DEV)
    for gi in range(i0, i0 + nw):
        lo = gi if gi == 0 else gi + k
        hi = gi + w if gi == nwin - 1 else gi + k + 1
        back[lo:hi] = x[lo:hi].to(TD[dt]).float()
    assert torch.equal(e.view(L, F, HW), back) and intact(whole_e, -3.0)
    assert (back != -3.0).any()


# ------------------------------------------------------------------------------------- guidance and the measurement operator

@pytest.mark.parametrize("L,F,H,W,s,t", [(7, 3, 24, 36, 12, 3), (4, 2, 6, 9, 3, 1), (5, 1, 8, 16, 1, 2)])
def test_guidance_and_pooling_on_non_square_fields(L, F, H, W, s, t):
    """cells of 144 pixels (64 + 64 + 16 lanes of the wave), 9 (fewer lanes than the wave has) and 1; H != W"""
    nobs = (L + t - 1) // t
    g = torch.Generator().manual_seed(H * W + s)
    x = torch.randn(L, F, H, W, generator=g).to(DEV)
    eps = torch.randn(L, F, H, W, generator=g).to(DEV)
    yobs = torch.randn(nobs, F, H // s, W // s, generator=g).to(DEV)
    stdv = (torch.rand(F, generator=g) * 0.5 + 0.2).to(DEV)
    gvec = (torch.rand(F, generator=g) * 0.2 + 1e-3).to(DEV)
    mu, sigma, gamma = float(np.float32(0.83)), float(np.float32(0.57)), float(np.float32(0.013))
    tag = f"{L}x{F}x{H}x{W} s={s} t={t}"
    # the measurement operator
    whole, pooled = guarded(yobs.numel(), torch.float32)
    ops.pool_stride(x, pooled, nobs, F, H, W, s, t)
    tot = R._sum(R.exact(_cells(x[::t][:nobs], s)), -1, chain=_chain(s))
    R.report(f"pool_stride {tag}", R.assert_within(pooled, _div(tot, float(s * s)), what="pool_stride"))
    assert intact(whole)
    R.assert_rejects(pooled, _div(R._sum(R.exact(_cells(x[::t][:nobs].roll(1, 3), s)), -1, chain=_chain(s)), float(s * s)),
                     what="pool_stride, columns shifted by one")
    for gam, name in ((torch.full((F,), gamma, device=DEV), "guidance"), (gvec, "guidance_per_variable")):
        corr = guidance_correction(x, eps, yobs, stdv, gam, nobs, s, t, mu, sigma)
        spread = R.V(_uncells(corr.v.unsqueeze(-1).expand(*corr.v.shape, s * s), s), _uncells(corr.e.unsqueeze(-1).expand(*corr.e.shape, s * s), s))
        new = R._sub(R.exact(eps[::t][:nobs]), spread)
        want_v, want_e = eps.to(R.D), torch.zeros_like(eps, dtype=R.D)  # frames that are not observed: untouched, bound 0
        want_v[0: nobs * t: t], want_e[0: nobs * t: t] = new.v, new.e
        arg = gamma if name == "guidance" else gvec
        whole_e, fused = guarded(eps.numel(), torch.float32)
        fused.copy_(eps.view(-1))
        ops.guidance(x, fused.view_as(eps), yobs, stdv, nobs, F, H, W, s, t, mu, sigma, arg)
        R.report(f"{name} {tag}", R.assert_within(fused.view_as(eps), want_v, want_e, what=name))
        assert intact(whole_e)
        whole_d, delta = guarded(nobs * F * H * W, torch.float32)
        kept = eps.clone()
        ops.guidance_delta(x, eps, yobs, stdv, delta.view(nobs, F, H, W), nobs, F, H, W, s, t, mu, sigma, arg)
        assert torch.equal(eps, kept) and intact(whole_d)
        R.report(f"guidance_delta ({name}) {tag}", R.assert_within(delta.view(nobs, F, H, W), -spread.v, spread.e, what="guidance_delta"))
        both = eps.clone()
        both[::t][:nobs] += delta.view(nobs, F, H, W)
        assert torch.equal(both, fused.view_as(eps)) and not torch.equal(both, eps)
        # a transposed cell walk (q / s and q % s exchanged, or W for H in the row stride) moves the correction between cells
        if H // s != W // s:
            wrong = torch.zeros_like(want_v)
            wrong[0: nobs * t: t] = _uncells(corr.v.transpose(2, 3).reshape(nobs, F, H // s, W // s).unsqueeze(-1)
                                             .expand(nobs, F, H // s, W // s, s * s), s)
            R.assert_rejects(fused.view_as(eps), eps.to(R.D) - wrong, want_e, what=f"{name}, cells transposed")
