"""Float64 reference of the sampler's guidance kernels (csrc/sampler.hip: guidance_kernel, pool_stride) with fp64_ref's V arithmetic:
shared by tests/test_gpu_boundary_routes.py and the launch replay (tests/launch_replay.py).  Nothing here calls climate2weather_amd.ops."""
import torch

import fp64_ref as R


def _div(a, c):
    """a V over an exact fp32 scalar: one division (correctly rounded by default; K_ULP fp32 ulps allowed, as for fp64_ref's 1-ulp ops)"""
    v = a.v / c
    e = a.e / abs(c)
    return R.V(v, e + R.K_ULP * R.U32 * (v.abs() + e))


def _divv(a, b):
    a, b = R._v(a), R._v(b)
    v = a.v / b.v
    e = (a.e + v.abs() * b.e) / (b.v.abs() - b.e)
    return R.V(v, e + R.K_ULP * R.U32 * (v.abs() + e))


def _cells(t, s):
    """(n, F, H, W) -> (n, F, H / s, W / s, s * s)"""
    n, F, H, W = t.shape
    return t.reshape(n, F, H // s, s, W // s, s).permute(0, 1, 2, 4, 3, 5).reshape(n, F, H // s, W // s, s * s)


def _uncells(t, s):
    n, F, PH, PW, _ = t.shape
    return t.reshape(n, F, PH, PW, s, s).permute(0, 1, 2, 4, 3, 5).reshape(n, F, PH * s, PW * s)


def _chain(s):
    return -(-s * s // 64) + 6  # a lane's loop over the cell, then the six shuffle steps of the wave sum


def guidance_correction(x, eps, yobs, stdv, gam, nobs, s, t, mu, sigma):
    """sampler.hip, guidance_kernel, in float64 with the kernel's roundings: corr = sigma (err / var) / (mu s^2) per pooled cell, where
    x0 = (x - sigma eps) / mu, err = y - mean_cell(x0), var = std_c^2 + gamma_c (sigma / mu)^2.  V (nobs, F, PH, PW); mu, sigma fp32 values."""
    X, E = R.exact(x[::t][:nobs]), R.exact(eps[::t][:nobs])
    x0 = _div(R._sub(X, R._mul(sigma, E)), mu)
    tot = R._sum(R.V(_cells(x0.v, s), _cells(x0.e, s)), -1, chain=_chain(s))
    mean = _div(tot, float(s * s))
    ratio = _div(R._v(sigma), mu)
    sd = R.exact(stdv).view(1, -1, 1, 1)
    var = R._add(R._mul(sd, sd), R._mul(R._mul(R.exact(gam).view(1, -1, 1, 1), ratio), ratio))
    err = R._sub(R.exact(yobs), mean)
    q = _divv(err, R.V(var.v.expand_as(err.v), var.e.expand_as(err.v)))
    return _divv(R._mul(sigma, q), R._mul(mu, float(s * s)))


def guided_eps(x, eps, yobs, stdv, gam, nobs, F, H, W, s, t, mu, sigma):
    """(eps after c2w_guidance as (v, e) over all frames, the spread correction V on the observed frames): frames that are not observed
    keep their value with bound 0; c2w_guidance_delta writes -spread."""
    L = x.numel() // (F * H * W)
    X, E = x.reshape(-1)[: L * F * H * W].view(L, F, H, W), eps.reshape(-1)[: L * F * H * W].view(L, F, H, W)
    corr = guidance_correction(X, E, yobs.reshape(nobs, F, H // s, W // s), stdv.reshape(-1)[:F], gam, nobs, s, t, mu, sigma)
    spread = R.V(_uncells(corr.v.unsqueeze(-1).expand(*corr.v.shape, s * s), s), _uncells(corr.e.unsqueeze(-1).expand(*corr.e.shape, s * s), s))
    new = R._sub(R.exact(E[::t][:nobs]), spread)
    want_v, want_e = E.to(R.D), torch.zeros_like(E, dtype=R.D)
    want_v[0: nobs * t: t], want_e[0: nobs * t: t] = new.v, new.e
    return R.V(want_v, want_e), spread
