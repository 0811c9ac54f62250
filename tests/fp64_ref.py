"""Float64 references of the conv, weight-gradient, LayerNorm, reduction and attention kernels, each with an element-wise error bound.

Every function takes the kernel's own (storage-typed) operands, computes the exact operation in torch.float64 with torch's own ops on
the operands' device (F.conv2d, F.conv_transpose2d, F.interpolate, F.unfold, einsum; chunked by image) and returns V(ref, bound): two
float64 tensors of the output's shape.  A correct kernel satisfies |got - ref| <= bound element by element (assert_within).  This module
never calls climate2weather_amd.ops or tests/emu_ops.py.

Error model (u32 = 2^-24; u_T = 2^-8 bf16, 2^-11 fp16, 2^-24 fp32).  A value is carried as V(v, e): v its exact fp64 value, e a bound
on how far the kernel's fp32 / storage-typed value may be from v.  The kernels' arithmetic is restated operation by operation:

  * fp32 add / sub / mul (_add, _mul):   e = e_a + e_b (+ |a| e_b + |b| e_a + e_a e_b for a product) + u32 (|v| + e)
  * rounding to the storage type (_rnd): e += u_T (|v| + e) + floor_T; floor = 2^-25 for fp16 (half the subnormal spacing: results
    below 2^-14 keep fewer bits), 0 otherwise.  The conversions are v_cvt_pk_*_f32, round to nearest even (common.h:26-40).
  * transcendentals (_silu, _dsilu, _rsqrt): the propagated error times the function's largest slope (|silu'| <= 1.0998,
    |silu''| <= 0.5, rsqrt: 0.5 s^-1.5 e_s at s - e_s), plus K_ULP = 4 fp32 ulps of the magnitude of the result's terms
    (exp / rcp / rsq are 1-ulp instructions; silu = a * sigmoid(a) and dsilu = sg + h (1 - sg) add one rounding each).
  * an fp32 sum of N terms t_i done as a chain of at most L dependent additions (_sum):
        e = C_ACC u32 (sqrt(N) sqrt(sum t_i^2) + sqrt(L) |sum t_i|)  +  (propagated errors of the terms)
    The first term is the rounding model for zero-mean terms (partial sums grow like sqrt(k)).  The second is the chain of
    same-sign partial sums: with positive terms (loss sums, sum of squares) every partial sum is close to the total, and a chain of L
    additions (per-thread loop + wave tree + one atomicAdd per wave or workgroup onto one address; pointwise.hip:375/581/653,
    sampler.hip:80, conv_patch3.hip:375) rounds L times at that size.  L is taken from the kernels' launch geometry (_loss_chain);
    where it is not, L = N.  sum t_i^2 is the same fp64 op on squared operands (conv(x^2, w^2), dW(x^2, dy^2)).  C_ACC = 8.
    Propagated errors of the terms add up worst case inside a row (they share the row's statistics), and in quadrature
    (C_ACC sqrt(sum e_i^2)) across pixels, where they come from independent roundings (the modulation gradients dm).
  * conv K-sums: N = L = taps * Cin (kvalid when given); the bias is added in fp32 (conv_epilogue.h:46).

Roundings counted from conv_epilogue.h: the accumulator (+ bias, + SiLU) is rounded to T into the LDS tile (:53 / :91; fp32 tiles keep
fp32, :51); the multiplier (plain or dSiLU of it, :537/:540) and the residual (:547) are applied in fp32 to that rounded value and the
sum is rounded again (:549); the SiLU pair takes silu / silu' of that stored value and rounds each (:551-562); the second output is
silu of the stored value (:578-583); pool2 adds the four stored values in fp32 ((g00 + g01) + g10) + g11 and rounds (:469-491); the
fused LayerNorm forward reads the stored sum (:429-436) and runs ln_fwd_kernel's arithmetic (two-pass variance, :438-455); the fused
LayerNorm backward reads the conv tile as stored (:256), restates ln_bwd_kernel's arithmetic (:258-283) and rounds y once (:293);
dm receives the fp32 rows before the residual (:283, :362).  LayerNorm (pointwise.hip:24-72, 80-195): u = x + m, mean, c = u - mean,
q = sum c^2, rs = 1/sqrt(q/den + eps), out = c rs -- the statistics' errors propagate through these same rules, so (x - mean) * rstd
carries the error of the mean in c and the error of q in rs.

ReLU adds no rounding and is 1-Lipschitz, so the error of its argument passes through unchanged: C2W_ACT_RELU is max(v, 0) on the
accumulator + bias before the rounding into the tile (conv_epilogue.h:48 / :86; the split-K reduction conv_patch.hip:1199; the direct
kernel conv_igemm.hip:281); C2W_ACT_RELU_PAIR is y = max(a, 0) of the value a as stored, after the multiplier / residual and the rounding
of :599 (:614-625; conv_igemm.hip:295-300).  Its second output y2 = (a > 0) is discontinuous and gets no numeric bound: the rule is
consistency with the first, y2 == (y > 0) on every element (assert_mask_consistent) -- with y held to its bound the mask is determined.
NaN passes through max(., 0) as it does through torch.relu (common.h relu_f); assert_nan_footprint holds the kernel to the reference's NaNs.

Kept statistics (finish_ln_rows_stored, conv_epilogue.h:311-359): the operands are the normalised rows xhat and their 1/sigma rs, exact as
given; g is the tile as stored (:330).  sum g and sum g * xhat are fp32 sums over the row's 128 channels (:335-336, the 16 lanes by
sub16); c0 = sum g * (1/128) * rs and c2 = sum(g xhat) * (1/den) * rs are two products each (:339-340); o = g * rs - c0 - xhat * c2
(:344-345: two products, two subtractions -- where the compiler fuses a product with its subtraction one rounding leaves, so the bound
holds either way); dm receives the fp32 rows (:346), the residual is added in fp32 (:352) and the sum rounded once (:356).

Chain form (finish_lnf<RESN>, conv_epilogue.h:417-513): the residual is rebuilt from the normalised rows h (exact operands) as
x = h * rcp(rstd) + (mean - m): rcp is a 1-ulp instruction, counted as K_ULP ulps (:454), one subtraction and a product + a sum (:475;
fused into one fma it rounds once less).  u = tile + x in fp32 (:478).  Where y is written it is u rounded to T (:481) and the LayerNorm
reads that value back (:486); with C2W_CONV_NO_Y nothing is rounded and the LayerNorm sees the fp32 sum (:479-487).  The LayerNorm is the
arithmetic above (:488-504); its mean (:494) and 1/sigma (:501) are stored as fp32 (:509-510).

Attention (attention.hip, attention_mfma.hip): three routes with different arithmetic -- VALU (fp32 P / dP / dS, expf), T64 (one
64-key block: P normalised then rounded to T, delta inside the kernel) and BLOCKS (online softmax: P rounded unnormalised, accumulators
rescaled by alpha, delta from rowdot) -- each restated in attention_forward / attention_backward, whose docstrings cite every rounding
counted.  Errors shared by a softmax row (lse, delta, the fp32 scale) are summed worst case over the keys, one-per-element roundings
(the K-sums of S and dP, the exponentials, P and dS stored as T) in quadrature with C_ACC.  Two rules are local to that section: a
value stored as T is off by at most u_T |v| + floor_T and never by more than |v| (_store_err); a K-sum's error never exceeds the
classical n u32 sum |t_i| (_ksum_err).  The backward reference is the exact gradient at (qkv, do); the o / lse the kernel was given
enter through their actual distance from the exact ones, so one function serves emulated and kernel-produced inputs.

Bench-size cases: the reference is computed for every image and every reduction in full (no subset); the GPU tier's budget note is in
tests/test_gpu_fp64_bounds.py.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
UT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
FLOOR = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
C_ACC = 8.0
K_ULP = 4.0
SILU_SLOPE, DSILU_SLOPE = 1.0998, 0.5
CONV_1X1, CONV_S1, CONV_S2, CONV_UP, CONV_TS2 = 0, 1, 2, 3, 4  # include/c2w_hip.h
ACT_NONE, ACT_SILU, ACT_SILU_PAIR, ACT_RELU, ACT_RELU_PAIR = 0, 1, 2, 3, 4
MUL_PLAIN, MUL_DSILU = 0, 1
STORAGE = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}  # the library's dtype codes
D = torch.float64
CHUNK_ELEMS = 1 << 26  # doubles per image chunk of an im2col / conv intermediate


class V:
    """an fp64 value and the bound on the kernel's distance from it"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    def __iter__(self):
        return iter((self.v, self.e))

    def view(self, *shape):
        return V(self.v.reshape(*shape), self.e.reshape(*shape))


def exact(t):
    return V(t.to(D))


def _T(dtype):
    return STORAGE[dtype] if isinstance(dtype, int) else dtype


def _v(a):
    return a if isinstance(a, V) else V(torch.as_tensor(a, dtype=D))


def _add(a, b, sign=1.0):
    a, b = _v(a), _v(b)
    v = a.v + sign * b.v
    e = a.e + b.e
    return V(v, e + U32 * (v.abs() + e))


def _sub(a, b):
    return _add(a, b, -1.0)


def _mul(a, b):
    a, b = _v(a), _v(b)
    v = a.v * b.v
    e = a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e
    return V(v, e + U32 * (v.abs() + e))


def _scale(a, c):
    """a times an fp32 constant that is itself one rounding away from c (1/C, 1/den)"""
    v = a.v * c
    e = a.e * abs(c) + 2 * U32 * (v.abs() + a.e * abs(c))
    return V(v, e)


def _rnd(a, dtype):
    T = _T(dtype)
    return V(a.v, a.e + UT[T] * (a.v.abs() + a.e) + FLOOR[T])


def _sigmoid(x):
    return torch.sigmoid(x)


def _silu(a):
    s = _sigmoid(a.v)
    v = a.v * s
    return V(v, SILU_SLOPE * a.e + K_ULP * U32 * v.abs())


def _relu(a):
    """max(v, 0): 1-Lipschitz and exact, so the argument's error passes through; NaN stays NaN (torch.relu)"""
    return V(torch.relu(a.v), a.e)


def _rcp(a):
    """v_rcp_f32 of an exact operand: a 1-ulp instruction under K_ULP"""
    v = 1.0 / a.v
    return V(v, K_ULP * U32 * v.abs())


def _dsilu(a):
    s = _sigmoid(a.v)
    h = a.v * s
    v = s + h * (1 - s)
    return V(v, DSILU_SLOPE * a.e + K_ULP * U32 * (s + h.abs()))


def _rsqrt(a):
    v = a.v.rsqrt()
    lo = (a.v - a.e).clamp_min(a.v * 1e-3)
    return V(v, 0.5 * a.e * lo.pow(-1.5) + K_ULP * U32 * v)


def _acc(total, sumsq, n, chain):
    return C_ACC * U32 * (math.sqrt(n) * sumsq.clamp_min(0).sqrt() + math.sqrt(chain) * total.abs())


def _sum(a, dim, chain=None, indep=False):
    """fp32 sum of a V along dim; indep: the terms' propagated errors are independent roundings (added in quadrature)"""
    n = a.v.shape[dim]
    s = a.v.sum(dim)
    sq = (a.v * a.v).sum(dim)
    pe = C_ACC * (a.e * a.e).sum(dim).sqrt() if indep else a.e.sum(dim)
    if indep:
        pe = torch.minimum(pe, a.e.sum(dim))
    return V(s, _acc(s, sq, n, n if chain is None else chain) + pe)


# ---------------------------------------------------------------------------------------------------------------- convolution

def _rows(t, n, ld):
    return t.reshape(-1)[: n * ld].view(n, ld)


def _chunks(B, per_image):
    step = max(1, CHUNK_ELEMS // max(per_image, 1))
    return [(b0, min(B, b0 + step)) for b0 in range(0, B, step)]


def _core(X, W4, g):
    """X (b, Cin, Hin, Win) fp64, W4 (rows, Cin, 3, 3) or (rows, Cin) fp64 -> (b, rows, Hout, Wout)"""
    mode = g["mode"]
    if mode == CONV_1X1:
        return torch.einsum("bchw,oc->bohw", X, W4)
    if mode == CONV_S1:
        return F.conv2d(X, W4, padding=1)
    if mode == CONV_S2:
        return F.conv2d(X, W4, stride=2, padding=1)
    if mode == CONV_UP:
        return F.conv2d(F.interpolate(X, scale_factor=2.0, mode="nearest"), W4, padding=1)
    if mode == CONV_TS2:
        op = (g["Hout"] - (2 * g["Hin"] - 1), g["Wout"] - (2 * g["Win"] - 1))
        return F.conv_transpose2d(X, W4.permute(1, 0, 2, 3), stride=2, padding=1, output_padding=op)
    raise ValueError(mode)


def _weights(w, g):
    taps = 1 if g["mode"] == CONV_1X1 else 9
    rows = min(g["wrows"], g["Cout"])
    Wt = w.reshape(-1)[: g["wrows"] * taps * g["Cin"]].view(g["wrows"], taps, g["Cin"])[:rows].to(D)
    return Wt[:, 0] if taps == 1 else Wt.view(rows, 3, 3, -1).permute(0, 3, 1, 2)


def conv_sum(x, w, g, bias=None, kvalid=0, images=None):
    """The fp32 accumulator of c2w_conv_forward (+ bias) as V rows (npix, Cout); rows >= wrows are exact zeros.  images: (b0, b1)."""
    B, Hin, Win, Cin, Hout, Wout, Cout = (g[k] for k in ("B", "Hin", "Win", "Cin", "Hout", "Wout", "Cout"))
    taps = 1 if g["mode"] == CONV_1X1 else 9
    b0, b1 = images or (0, B)
    X = _rows(x, B * Hin * Win, Cin).view(B, Hin, Win, Cin)[b0:b1]
    W4 = _weights(w, g)
    rows = W4.shape[0]
    K = taps * (kvalid or Cin)
    out_v = torch.zeros((b1 - b0, Hout, Wout, Cout), dtype=D, device=x.device)
    out_e = torch.zeros_like(out_v)
    per = max(Hin * Win * Cin, Hout * Wout * Cin) * (9 if taps == 9 else 1) * (4 if g["mode"] == CONV_UP else 1)
    for c0, c1 in _chunks(b1 - b0, per):
        Xc = X[c0:c1].to(D).permute(0, 3, 1, 2)
        v = _core(Xc, W4, g)
        sq = _core(Xc * Xc, W4 * W4, g)
        e = _acc(v, sq, K, K)
        out_v[c0:c1, :, :, :rows] = v.permute(0, 2, 3, 1)
        out_e[c0:c1, :, :, :rows] = e.permute(0, 2, 3, 1)
    return add_bias(V(out_v.view(-1, Cout), out_e.view(-1, Cout)), bias, g)


def _mrows(m, npix, HW, C, ldm):
    if m is None:
        return None
    if ldm == 0:
        return m.reshape(-1)[:C].to(D).view(1, C).expand(npix, C)
    nb = npix // HW
    return torch.as_strided(m.reshape(-1), (nb, C), (ldm, 1)).to(D).repeat_interleave(HW, dim=0)


def _ln_stats(u, C, eps, unbiased):
    """ln_fwd_kernel / ln_bwd_kernel / finish_lnf: mean, centred rows, 1/sigma (pointwise.hip:44-60, 118-137)"""
    mean = _scale(_sum(u, 1), 1.0 / C)
    c = _sub(u, V(mean.v.unsqueeze(1).expand_as(u.v), mean.e.unsqueeze(1).expand_as(u.v)))
    q = _sum(_mul(c, c), 1)
    var = _scale(q, 1.0 / (C - 1 if unbiased else C))
    rs = _rsqrt(_add(var, float(np.float32(eps))))
    return mean, c, rs


def _bc(a, like):
    return V(a.v.unsqueeze(1).expand_as(like.v), a.e.unsqueeze(1).expand_as(like.v))


def layernorm(u, C, eps, unbiased, dtype):
    """LN of V rows u (already + m): returns (y rounded to T, rstd V, mean V)"""
    mean, c, rs = _ln_stats(u, C, eps, unbiased)
    return _rnd(_mul(c, _bc(rs, c)), dtype), rs, mean


def ln_backward_rows(g, u, C, eps, unbiased):
    """the fp32 rows o = (g - mean(g) - xhat * sum(g xhat)/den) * rs of ln_bwd_kernel (pointwise.hip:118-160), g and u as V rows"""
    mean, c, rs = _ln_stats(u, C, eps, unbiased)
    xh = _mul(c, _bc(rs, c))
    gmean = _scale(_sum(g, 1), 1.0 / C)
    dot = _scale(_sum(_mul(g, xh), 1), 1.0 / (C - 1 if unbiased else C))
    o = _mul(_sub(_sub(g, _bc(gmean, g)), _mul(xh, _bc(dot, xh))), _bc(rs, g))
    return o


def ln_backward_rows_stored(g, xh, rs, C, unbiased):
    """the fp32 rows o = rs * (g - mean(g) - xhat * sum(g xhat) / den) of finish_ln_rows_stored (conv_epilogue.h:335-346): g the stored
    tile as V rows, xh (rows, C) and rs (rows,) the kept operands in fp64, exact as given"""
    xh, rs = V(xh), V(rs.unsqueeze(1).expand_as(g.v))
    c0 = _mul(_bc(_scale(_sum(g, 1), 1.0 / C), g), rs)                                          # :339
    c2 = _mul(_bc(_scale(_sum(_mul(g, xh), 1), 1.0 / (C - 1 if unbiased else C)), g), rs)        # :340
    return _sub(_sub(_mul(g, rs), c0), _mul(xh, c2))                                              # :344-345


def dm_sums(o, npix, HW, C, ldm):
    """dm[b] (or dm) += the pixel sum of the rows o: per image with ldm, all pixels into one row without"""
    if ldm:
        return _sum(o.view(npix // HW, HW, C), 1, indep=True)
    return _sum(o, 0, indep=True).view(1, C)


def add_bias(acc, bias, g):
    """the fp32 bias add of the epilogue (conv_epilogue.h:46) onto an accumulator V from conv_sum(..., bias=None)"""
    if bias is None:
        return acc
    rows = min(g["wrows"], g["Cout"])
    bv = torch.zeros(g["Cout"], dtype=D, device=acc.v.device)
    bv[:rows] = bias.reshape(-1)[:rows].to(D)
    s = _add(acc, V(bv.expand_as(acc.v)))
    live = torch.arange(g["Cout"], device=acc.v.device) < rows
    return V(torch.where(live, s.v, acc.v), torch.where(live, s.e, acc.e))


def conv(x, w, g, dtype, bias=None, act=ACT_NONE, res=None, mul=None, mulmode=MUL_PLAIN, y2=False, pool2=False, lnf=None, ln=None,
         kvalid=0, pre=None, resn=None, no_y=False):
    """c2w_conv_forward's outputs as V: dict with 'y' (rows (npix or npix/4, Cout); absent with no_y), and where asked 'y2', 'hn' + 'rstd'
    + 'mean' (lnf), 'dm' + 'o' (ln).
    lnf / ln: dict(m, ldm, eps, unbiased[, x]) as in ops.conv (ln['x'] = the LayerNorm input rows, recomputed statistics; with ln['rstd']
    the normalised rows the forward kept and their 1/sigma).  resn: dict(rstd, mean[, m]) -- `res` holds normalised rows and the residual
    is rebuilt from them; no_y: the sum is not written and the LayerNorm sees it unrounded (the chain form).
    act = ACT_RELU_PAIR returns 'y' only: the mask y2 is held by assert_mask_consistent.
    pre: conv_sum(x, w, g, kvalid=...) computed once for several epilogues of the same operands."""
    T = _T(dtype)
    B, Hout, Wout, Cout, ldy = g["B"], g["Hout"], g["Wout"], g["Cout"], g["ldy"]
    npix, HW = B * Hout * Wout, Hout * Wout
    a = add_bias(pre if pre is not None else conv_sum(x, w, g, None, kvalid), bias, g)
    if act == ACT_SILU:
        a = _silu(a)
    if act == ACT_RELU:
        a = _relu(a)  # conv_epilogue.h:48 / :86
    a = _rnd(a, T)  # the LDS tile (conv_epilogue.h:53; fp32 tiles :51)
    out = {}
    if ln is not None:  # fused LayerNorm backward: g = the stored tile, u = ln_x + m (conv_epilogue.h:256-283)
        if ln.get("rstd") is not None:  # the forward kept xhat and 1/sigma (:311-359): ln_m is not read
            o = ln_backward_rows_stored(a, _rows(ln["x"], npix, ldy)[:, :Cout].to(D), ln["rstd"].reshape(-1)[:npix].to(D), Cout, ln["unbiased"])
        else:
            u = exact(_rows(ln["x"], npix, ldy)[:, :Cout])
            m = _mrows(ln.get("m"), npix, HW, Cout, ln.get("ldm", 0))
            if m is not None:
                u = _add(u, V(m))
            o = ln_backward_rows(a, u, Cout, ln["eps"], ln["unbiased"])
        out["o"] = o  # the fp32 rows dm is summed from (the planted "tile missing from dm" takes its pixels' rows from here)
        out["dm"] = dm_sums(o, npix, HW, Cout, ln.get("ldm", 0))
        if res is not None:
            o = _add(o, exact(_rows(res, npix, ldy)[:, :Cout]))
        out["y"] = _rnd(o, T)
        return out
    f = a
    if resn is not None or no_y:  # the chain form: conv_epilogue.h:437-487
        assert lnf is not None and mul is None and act == ACT_NONE and not y2 and not pool2
        if resn is not None:
            h = exact(_rows(res, npix, ldy)[:, :Cout])
            col = lambda t: t.reshape(-1)[:npix].to(D).unsqueeze(1).expand(npix, Cout)  # noqa: E731
            rm = _mrows(resn.get("m"), npix, HW, Cout, lnf.get("ldm", 0))
            shift = _sub(V(col(resn["mean"])), V(rm)) if rm is not None else V(col(resn["mean"]))   # :475 (rmean - rm2)
            f = _add(f, _add(_mul(h, _rcp(V(col(resn["rstd"])))), shift))                            # :454, :475, :478
        elif res is not None:
            f = _add(f, exact(_rows(res, npix, ldy)[:, :Cout]))                                      # :478
        if not no_y:
            f = _rnd(f, T)  # :481, read back :486
            out["y"] = f
        m = _mrows(lnf.get("m"), npix, HW, Cout, lnf.get("ldm", 0))
        u = _add(f, V(m)) if m is not None else f
        out["hn"], out["rstd"], out["mean"] = layernorm(u, Cout, lnf["eps"], lnf["unbiased"], T)
        return out
    if mul is not None or res is not None:
        if mul is not None:
            mm = exact(_rows(mul, npix, ldy)[:, :Cout])
            f = _mul(f, _dsilu(mm) if mulmode == MUL_DSILU else mm)
        if res is not None:
            f = _add(f, exact(_rows(res, npix, ldy)[:, :Cout]))
        f = _rnd(f, T)  # conv_epilogue.h:549
    if act == ACT_SILU_PAIR:
        out["y"], out["y2"] = _rnd(_silu(f), T), _rnd(_dsilu(f), T)
        return out
    if act == ACT_RELU_PAIR:  # max(a, 0) of the stored value: representable, no rounding (conv_epilogue.h:614-625)
        out["y"] = _relu(f)
        return out
    if pool2:
        q = f.view(B, Hout // 2, 2, Wout // 2, 2, Cout)
        p = _add(_add(_add(V(q.v[:, :, 0, :, 0], q.e[:, :, 0, :, 0]), V(q.v[:, :, 0, :, 1], q.e[:, :, 0, :, 1])),
                      V(q.v[:, :, 1, :, 0], q.e[:, :, 1, :, 0])), V(q.v[:, :, 1, :, 1], q.e[:, :, 1, :, 1]))
        out["y"] = _rnd(p, T).view(npix // 4, Cout)
        return out
    out["y"] = f
    if y2:
        out["y2"] = _rnd(_silu(f), T)
    if lnf is not None:  # LN of the stored result (+ the consumer's modulation): conv_epilogue.h:429-455
        m = _mrows(lnf.get("m"), npix, HW, Cout, lnf.get("ldm", 0))
        u = _add(f, V(m)) if m is not None else f
        out["hn"], out["rstd"], out["mean"] = layernorm(u, Cout, lnf["eps"], lnf["unbiased"], T)
    return out


# ------------------------------------------------------------------------------------------------------------ weight gradient

def _unfold(X, g):
    """(b, Cin, Hin, Win) -> (b, taps * Cin, Hout * Wout) patches in the [tap][ci] order of the weight rows"""
    mode = g["mode"]
    b, Cin = X.shape[:2]
    if mode == CONV_1X1:
        return X.reshape(b, Cin, -1)
    if mode == CONV_UP:
        X = F.interpolate(X, scale_factor=2.0, mode="nearest")
    P = F.unfold(X, 3, padding=1, stride=2 if mode == CONV_S2 else 1)  # (b, Cin * 9, L) in [ci][tap] order
    return P.view(b, Cin, 9, -1).transpose(1, 2).reshape(b, 9 * Cin, -1)


def wgrad(x, dy, g, images=None, pixels=None):
    """c2w_conv_wgrad: (dW V rows (Cout, taps * Cin), dbias V (Cout,)) -- sums over all B * Hout * Wout pixels.
    images = (b0, b1) and pixels = a boolean (Hout, Wout) mask restrict the sum (the planted defects)."""
    B, Hin, Win, Cin, Hout, Wout, Cout, ldy = (g[k] for k in ("B", "Hin", "Win", "Cin", "Hout", "Wout", "Cout", "ldy"))
    taps = 1 if g["mode"] == CONV_1X1 else 9
    b0, b1 = images or (0, B)
    X = _rows(x, B * Hin * Win, Cin).view(B, Hin, Win, Cin)
    G = _rows(dy, B * Hout * Wout, ldy)[:, :Cout].view(B, Hout * Wout, Cout)
    dw = torch.zeros((Cout, taps * Cin), dtype=D, device=x.device)
    dw2 = torch.zeros_like(dw)
    db = torch.zeros(Cout, dtype=D, device=x.device)
    db2 = torch.zeros_like(db)
    mask = None if pixels is None else pixels.reshape(-1).to(x.device)
    per = Hout * Wout * Cin * taps * (4 if g["mode"] == CONV_UP else 1)
    for c0, c1 in _chunks(b1 - b0, per):
        Xc = X[b0 + c0:b0 + c1].to(D).permute(0, 3, 1, 2)
        Gc = G[b0 + c0:b0 + c1].to(D)
        if mask is not None:
            Gc = Gc * mask.view(1, -1, 1)
        P = _unfold(Xc, g)
        dw += torch.einsum("bkl,blo->ok", P, Gc)
        dw2 += torch.einsum("bkl,blo->ok", P * P, Gc * Gc)
        db += Gc.sum((0, 1))
        db2 += (Gc * Gc).sum((0, 1))
    N = B * Hout * Wout
    return V(dw, _acc(dw, dw2, N, N)), V(db, _acc(db, db2, N, N))


# --------------------------------------------------------------------------------------------------------- pointwise kernels

def ln_forward(x, m, npix, HW, C, ldm, eps, unbiased, dtype):
    """ln_fwd_kernel: (y V rows, rstd V)"""
    u = exact(_rows(x, npix, C))
    mm = _mrows(m, npix, HW, C, ldm)
    if mm is not None:
        u = _add(u, V(mm))
    y, rs, _ = layernorm(u, C, eps, unbiased, dtype)
    return y, rs


def ln_backward(dy, x, m, dres, npix, HW, C, ldm, eps, unbiased, dtype):
    """ln_bwd_kernel: (dx V rows, dm V (images or 1, C))"""
    u = exact(_rows(x, npix, C))
    mm = _mrows(m, npix, HW, C, ldm)
    if mm is not None:
        u = _add(u, V(mm))
    o = ln_backward_rows(exact(_rows(dy, npix, C)), u, C, eps, unbiased)
    dm = dm_sums(o, npix, HW, C, ldm)
    if dres is not None:
        o = _add(o, exact(_rows(dres, npix, C)))
    return _rnd(o, dtype), dm


def colsum(a, rows, C, lda, dtype):
    """colsum_kernel (pointwise.hip:200-232): per-thread row loop, the row groups in LDS, one atomic per block and channel"""
    P = 4 if _T(dtype) == torch.float32 else 8
    ngrp = 256 // min(C // P, 256)
    chain = -(-2048 // ngrp) + ngrp + -(-rows // 2048)
    A = _rows(a, rows, lda)[:, :C].to(D)
    s, sq = A.sum(0), (A * A).sum(0)
    return V(s, _acc(s, sq, rows, chain))


def _loss_chain(n, nblk, per_atomic_blocks=4):
    """a grid-stride loop of nblk blocks of 256 threads, a wave tree, one atomicAdd per wave (or per block) onto one address"""
    per_thread = 2 * -(-n // (nblk * 256)) + 8
    return per_thread + 6 + per_atomic_blocks * nblk


def _nchw(eps, B, C, HW):
    return eps.reshape(-1)[: B * C * HW].view(B, C, HW).permute(0, 2, 1).reshape(B * HW, C).to(D)


def mse_loss_sum(y, eps, B, C, HW, ldc):
    """the loss sum of c2w_mse_loss_grad (tiled kernel, pointwise.hip:538-582: at most 2048 blocks, one atomic per wave)"""
    d = _rows(y, B * HW, ldc)[:, :C].to(D) - _nchw(eps, B, C, HW)
    t = d * d
    s, sq = t.sum(), (t * t).sum()
    nblk = min(B * -(-HW // 64), 2048)
    return V(s, _acc(s, sq, t.numel(), _loss_chain(t.numel(), nblk)))


def mse_dy(y, eps, B, C, HW, ldc, gscale, dtype):
    """dY rows of c2w_mse_loss_grad: (y - eps) * gscale rounded to T, padding channels exact zeros"""
    d = _sub(exact(_rows(y, B * HW, ldc)[:, :C]), V(_nchw(eps, B, C, HW)))
    o = _rnd(_scale(d, gscale), dtype)
    z = torch.zeros((B * HW, ldc), dtype=D, device=y.device)
    zv, ze = z.clone(), z.clone()
    zv[:, :C], ze[:, :C] = o.v, o.e
    return V(zv, ze)


def sq_err_sum(y, eps, B, C, HW, ldc):
    """the loss sum of sq_err_tiled_kernel (pointwise.hip:615-655) -- same grid rule as the loss tail"""
    return mse_loss_sum(y, eps, B, C, HW, ldc)


def fused_loss_sum(y, erows, C, lde, npix, workgroups):
    """conv_patch3.hip:340-375: per-thread squares of (stored prediction - fp16 noise row), a wave tree, one atomic per workgroup"""
    d = _rows(y, npix, y.shape[-1])[:, :C].to(D) - _rows(erows, npix, lde)[:, :C].to(D)
    t = d * d
    s, sq = t.sum(), (t * t).sum()
    return V(s, _acc(s, sq, t.numel(), _loss_chain(t.numel(), workgroups, 1)))


def sumsq(v, n):
    """sampler.hip:76-81: grid_for(n, 256, 2048) blocks, a grid-stride loop, one atomic per wave"""
    a = v.reshape(-1)[:n].to(D)
    t = a * a
    s, sq = t.sum(), (t * t).sum()
    nblk = min(-(-n // 256), 2048)
    return V(s, _acc(s, sq, n, _loss_chain(n, nblk)))


# ------------------------------------------------------------------------------------------------------------------ attention

VALU, T64, BLOCKS = "valu", "t64", "blocks"  # the three code paths of c2w_attention_forward / _backward
KB = 64  # key block of the matrix-core kernels (attention_mfma.hip:23)


def _qkv(qkv, B, T, C):
    X = _rows(qkv, B * T, 3 * C).to(D).view(B, T, 3 * C)
    return X[..., :C], X[..., C:2 * C], X[..., 2 * C:]


def _quad(x, dim=-1):
    """independent roundings along dim: C_ACC standard deviations, never more than the worst case"""
    return torch.minimum(C_ACC * (x * x).sum(dim).sqrt(), x.sum(dim))


def _mixv(W, M, coh, ind, n):
    """out[b,t,c] = sum_s W[b,t,s] M[b,s,c] as an fp32 chain of n terms; coh / ind: absolute errors of W that add up coherently
    (shared by the row: worst case) / independently (one rounding per element: quadrature)"""
    v = torch.einsum("bts,bsc->btc", W, M)
    Ma, M2 = M.abs(), M * M
    worst = torch.einsum("bts,bsc->btc", ind, Ma)
    e = torch.einsum("bts,bsc->btc", coh, Ma) + torch.minimum(C_ACC * torch.einsum("bts,bsc->btc", ind * ind, M2).clamp_min(0).sqrt(), worst)
    return V(v, e + _acc(v, torch.einsum("bts,bsc->btc", W * W, M2), n, n))


def _store_err(mag, T_):
    """the rounding of a value of magnitude <= mag to T: u_T mag + floor_T, and never more than mag itself (zero is on the grid: what
    rounds to zero is off by exactly its own size -- most weights of a peaked row, most dS s^2 of a 2^-12 gradient in fp16)"""
    return torch.minimum(UT[T_] * mag + FLOOR[T_], mag)


def attention_exact(qkv, B, T, C, do=None):
    """the textbook operation in float64: dict of S (scaled scores), m, l, P, lse, o and, given do, dP, delta, dS, dq, dk, dv"""
    q, k, v = _qkv(qkv, B, T, C)
    s2 = 1.0 / math.sqrt(C)
    S = torch.einsum("btc,bsc->bts", q, k) * s2
    m = S.amax(-1, keepdim=True)
    e = (S - m).exp()
    l = e.sum(-1, keepdim=True)
    P = e / l
    x = dict(q=q, k=k, v=v, s2=s2, S=S, m=m, l=l, P=P, lse=(m + l.log()).squeeze(-1), o=torch.einsum("bts,bsc->btc", P, v))
    if do is not None:
        dO = _rows(do, B * T, C).to(D).view(B, T, C)
        dP = torch.einsum("btc,bsc->bts", dO, v)
        delta = (dO * x["o"]).sum(-1)
        dS = P * (dP - delta.unsqueeze(-1))
        x.update(dO=dO, dP=dP, delta=delta, dS=dS, dq=s2 * torch.einsum("bts,bsc->btc", dS, k),
                 dk=s2 * torch.einsum("bts,btc->bsc", dS, q), dv=torch.einsum("bts,btc->bsc", P, dO))
    return x


def _ksum_err(total, sumsq, sumabs, n):
    """an fp32 fma chain of n products: the module's _acc rule, and never more than the classical worst case n u32 sum |t_i| (short
    chains of same-sign products -- logits that share an offset -- where C_ACC sqrt(n) exceeds n)"""
    return torch.minimum(_acc(total, sumsq, n, n), n * U32 * (1 + n * U32) * sumabs)


def _score_err(x, C):
    """the fp32 K-sum of S before the scale (attention.hip:58, attention_mfma.hip:79/269: N = L = C), times s^2"""
    raw = x["S"] / x["s2"]
    q, k = x["q"], x["k"]
    return _ksum_err(raw, torch.einsum("btc,bsc->bts", q * q, k * k), torch.einsum("btc,bsc->bts", q.abs(), k.abs()), C) * x["s2"]


def _running_max(S, T):
    """the running row maximum after each 64-key block (attention_mfma.hip:282, 291), spread over the block's keys: (B, T, T)"""
    B = S.shape[0]
    nb = T // KB
    M = S.view(B, T, nb, KB).amax(-1).cummax(-1).values
    return M, M.repeat_interleave(KB, dim=-1)


def attention_forward(qkv, B, T, C, dtype, route, parts=None):
    """c2w_attention_forward: (o V rows (B * T, C), lse V (B * T,)).

    Weights.  S~ = s2~ * (fp32 K-sum): the sum's rounding is independent per (query, key); s2~ = 1.0f / sqrtf(C) is up to two roundings
    from C^-1/2 and multiplies every score of the tensor alike: S~ - m~ = (1 + d)(S - m), an error d |S - m| in the exponent that is
    shared (coherent) along the row.  m~, the row maximum of S~, is an arbitrary shift: softmax and lse = m~ + log sum exp(S~ - m~)
    do not depend on it, so only the roundings of S~ s2~ (u32 |S|, attention.hip:62, attention_mfma.hip:142/279), of the subtraction
    (u32 |x|, :121, mfma :149/287) and of the exponential count.  expf (attention.hip:121) is K_ULP ulps; __expf(x) (mfma :149, :283,
    :287) is exp2(x log2 e): the product's rounding is an absolute error u32 |x| log2 e in the exponent of 2, i.e. a relative 2 u32 |x|
    of the result once the constant's own rounding is counted.  The row sum is a chain of T / 16 + 8 additions (attention.hip:120-126;
    mfma :150-152, :288-290) of positive terms; 1 / sum and the product (attention.hip:127-128, mfma :153-156, :313-316) 2 u32.
    Routes:  VALU: P stays fp32 in LDS, o = fp32 chain over the T keys (attention.hip:79-95), one rounding to T (:95).
    T64: P normalised, then rounded to T (mfma :156): an independent u_T P + floor_T per element; o rounded (:109).
    BLOCKS: P_j = exp(s - running max) rounded to T unnormalised (:293) -- in units of the final weights u_T P + floor_T A / l, with
    A = exp(running max - final max) <= 1 the later rescales; the row sum is taken from the fp32 values (:290); every later block
    multiplies accumulator and sum by alpha = __expf(m_old - m_new) (:283, :290, :303): per transition 2 u32 |m_old - m_new| + K_ULP ulps
    + two product roundings, shared by the row; o = oacc / l rounded (:313-316).  lse = m + logf / __logf(sum) (attention.hip:129,
    mfma :157, :317): the sum's relative error, K_ULP ulps of |log sum| + 1, one addition."""
    T_ = _T(dtype)
    x = parts or attention_exact(qkv, B, T, C)
    S, m, l, P, v = x["S"], x["m"], x["l"], x["P"], x["v"]
    fast = route != VALU
    if route == BLOCKS:
        M, Mj = _running_max(S, T)
        xa = (S - Mj).abs()
        a = (M[..., :-1] - M[..., 1:]).abs()  # the transitions' exponents (the first block's alpha multiplies zeros)
        ralpha = (U32 * (2 * a + K_ULP + 2)).sum(-1, keepdim=True)
        A = (Mj - m).exp()
    else:
        xa = (S - m).abs()
        ralpha = torch.zeros_like(m)
    rc = 2 * U32 * (S - m).abs()
    ri = _score_err(x, C) + U32 * S.abs() + U32 * xa * (3 if fast else 1) + K_ULP * U32
    chain = T // 16 + 8
    rel_l = (P * (rc + ri)).sum(-1, keepdim=True) + ralpha + C_ACC * U32 * (math.sqrt(T) * (P * P).sum(-1, keepdim=True).sqrt() + math.sqrt(chain))
    coh = P * (rc + rel_l + ralpha + 2 * U32)
    ind = P * ri
    if route == T64:
        ind = ind + _store_err(P + coh + ind, T_)
    elif route == BLOCKS:  # the stored value is P l / A
        ind = ind + _store_err((P + coh + ind) * l / A, T_) * A / l
    o = _rnd(_mixv(P, v, coh, ind, T), T_)
    lse = x["lse"]
    e_lse = rel_l.squeeze(-1) + K_ULP * U32 * (l.squeeze(-1).log().abs() + 1) + U32 * (lse.abs() + m.squeeze(-1).abs())
    return o.view(B * T, C), V(lse.reshape(-1), e_lse.reshape(-1))


def rowdot(a, b, rows, C):
    """rowdot_kernel (attention.hip:192-209): 16 lanes per row, each an fma chain over C / 16 elements, four shuffle additions"""
    A, Bm = _rows(a, rows, C).to(D), _rows(b, rows, C).to(D)
    t = A * Bm
    s = t.sum(-1)
    return V(s, _acc(s, (t * t).sum(-1), C, -(-C // 16) + 4))


def attention_backward(qkv, o_in, do, lse_in, B, T, C, dtype, route, parts=None):
    """c2w_attention_backward: dqkv V rows (B * T, 3 C); the reference is the exact gradient at (qkv, do); o_in / lse_in are the
    tensors the kernel was given and enter through their ACTUAL distance from the exact o / lse.

    P~ = exp(S~ s2~ - lse_in) (attention.hip:162/181 expf; mfma :202, :364 __expf): the exponent is off by |lse_in - lse| (shared by
    the row), by 2 u32 |S| for s2~ (shared by the tensor: here nothing cancels it, S~ and lse are two large numbers when the logits
    share an offset), and independently by the K-sum of S, u32 |S| (the product), u32 |S - lse| (the subtraction) and the exponential
    (K_ULP ulps; __expf 2 u32 |S - lse| more).  dP = dO v^T is an fp32 K-sum over C (attention.hip:157/177, mfma :189, :400, :450).
    delta: VALU and BLOCKS read rowdot(dO, o_in) (attention.hip:226, :259-260): its distance from the exact delta is the actual
    |sum_c dO (o_in - o)| plus rowdot's own chain.  T64 sums P~ dP~ over the row's 64 keys in fp32 (mfma :203-205) and never reads o_in.
    dS = P~ (dP~ - delta~): the errors of delta and lse are the same for every key of the row and add up coherently in dq_i
    (s2 e sum_j P_ij |k_j|); so does, here, the part of P~'s error that s2~ causes.  VALU keeps P and dS fp32 in LDS and applies s2~
    after the key sum (attention.hip:169, :187; 2 u32); the matrix-core routes round P and dS s2~ to T (mfma :209-210, :365-366), an
    independent u_T |.| + floor_T per element, summed over T keys (dq, :220/:460) or T queries (dk :231/:415, dv :224/:411).
    Each output is one more rounding to T (attention.hip:95, mfma :109, :349)."""
    T_ = _T(dtype)
    x = parts or attention_exact(qkv, B, T, C, do)
    S, P, q, k, s2, dO, dP, delta, dS = (x[n] for n in ("S", "P", "q", "k", "s2", "dO", "dP", "delta", "dS"))
    fast = route != VALU
    dl = (_rows(lse_in, B, T).to(D) - x["lse"]).abs().unsqueeze(-1)
    xa = (S - x["lse"].unsqueeze(-1)).abs()
    rc = dl + 2 * U32 * S.abs()
    ri = _score_err(x, C) + U32 * S.abs() + U32 * xa * (3 if fast else 1) + K_ULP * U32
    eDP = _ksum_err(dP, torch.einsum("btc,bsc->bts", dO * dO, x["v"] ** 2), torch.einsum("btc,bsc->bts", dO.abs(), x["v"].abs()), C)
    if route == T64:
        dd = (P * dP.abs() * rc).sum(-1) + _quad(P * (dP.abs() * ri + eDP)) + _acc(delta, (P * P * dP * dP).sum(-1), T, 8)
    else:
        oin = _rows(o_in, B * T, C).to(D).view(B, T, C)
        dd = (dO * (oin - x["o"])).sum(-1).abs() + rowdot(do, o_in, B * T, C).e.view(B, T)
    dev = (dP - delta.unsqueeze(-1)).abs()
    coh = P * (dev * rc + dd.unsqueeze(-1))
    ind = P * (dev * ri + eDP) + 3 * U32 * dS.abs()
    g = dS * s2
    gc, gi = coh * s2 + 2 * U32 * g.abs(), ind * s2
    Pc, Pi = P * rc, P * ri
    if route != VALU:
        gi = gi + _store_err(g.abs() + gc + gi, T_)
        Pi = Pi + _store_err(P + Pc + Pi, T_)
    tr = lambda t: t.transpose(1, 2)
    dq = _rnd(_mixv(g, k, gc, gi, T), T_)
    dk = _rnd(_mixv(tr(g), q, tr(gc), tr(gi), T), T_)
    dv = _rnd(_mixv(tr(P), dO, tr(Pc), tr(Pi), T), T_)
    return V(torch.cat((dq.v, dk.v, dv.v), -1).view(B * T, 3 * C), torch.cat((dq.e, dk.e, dv.e), -1).view(B * T, 3 * C))


def attn_layout(B, T, C, sections):
    """assert_within's layout of attention rows (B * T, len(sections) * C): sections 'o' or 'qkv'; () for lse / delta (B * T,)"""
    return dict(attn=True, B=B, T=T, C=C, sections=tuple(sections))


def _where_attn(idx, lay):
    T, C, sec = lay["T"], lay["C"], lay["sections"]
    row, col = divmod(idx, max(len(sec), 1) * C) if sec else (idx, 0)
    b, t = divmod(row, T)
    reg = [f"16-row strip {t // 16} of {-(-T // 16)}", f"64-token block {t // KB} of {-(-T // KB)}"]
    if t < 16 or t >= (T - 1) // 16 * 16:
        reg.append(("first" if t < 16 else "last") + " 16-row strip")
    if t < KB or t >= (T - 1) // KB * KB:
        reg.append(("first" if t < KB else "last") + " 64-key block")
    if not sec:
        return f"image {b}, token {t}", reg
    s, c = divmod(col, C)
    reg.append(("upper" if c // 16 >= (C // 16) // 2 else "lower") + " wave half's column tiles")
    return f"image {b}, token {t}, section {sec[s]}, channel {c}", reg


# ---------------------------------------------------------------------------------------------------------------- the checks

def _where(idx, layout):
    """(image, row, column, channel) of a flat index into rows (B * H * W, C), and the regions it lies in"""
    if not layout:
        return f"flat index {idx}", []
    if layout.get("attn"):
        return _where_attn(idx, layout)
    B, H, W, C = layout["B"], layout["H"], layout["W"], layout["C"]
    pix, c = divmod(idx, C)
    b, r = divmod(pix, H * W)
    h, w = divmod(r, W)
    th, tw = layout.get("tile", (8, 16))
    reg = []
    if h in (0, H - 1) or w in (0, W - 1):
        reg.append("border row/column")
    if h % th in (0, th - 1) or w % tw in (0, tw - 1):
        reg.append("tile seam")
    ct = layout.get("ctile", 128)
    if C % ct and c >= C // ct * ct:
        reg.append("last partial channel tile")
    if c >= layout.get("creal", C):
        reg.append("padded channels")
    return f"image {b}, row {h}, column {w}, channel {c}", reg or ["interior"]


def ratio(got, ref, bound=None):
    if bound is None:
        ref, bound = ref
    err = (got.to(D).reshape(ref.shape) - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return torch.where(torch.isnan(err), torch.full_like(err, math.inf), r)


def assert_within(got, ref, bound=None, what="", layout=None):
    """|got - ref| <= bound element by element; returns the largest err / bound (printed by the callers).
    layout = dict(B, H, W, C[, tile, ctile, creal]) names the failing location for rows (B * H * W, C); attn_layout(...) for attention rows."""
    if isinstance(ref, V):
        ref, bound = ref.v, ref.e
    r = ratio(got, ref, bound).reshape(-1)
    worst = r.max().item()
    if not worst <= 1.0:
        i = int(r.argmax().item())
        loc, reg = _where(i, layout)
        g = got.to(D).reshape(-1)[i].item()
        raise AssertionError(f"{what}: err/bound {worst:.3g} at {loc} ({', '.join(reg)}): got {g:.6g}, fp64 {ref.reshape(-1)[i].item():.6g}, "
                             f"bound {bound.reshape(-1)[i].item():.3g}; {int((r > 1).sum().item())} of {r.numel()} elements violate the bound")
    return worst


def assert_mask_consistent(y, y2, what=""):
    """the rule of C2W_ACT_RELU_PAIR's second output: y2 == (y > 0) exactly, on every element (so 1 or 0, and 0 where y is -0, +0 or NaN).
    The mask is discontinuous in the pre-activation and gets no numeric bound of its own; y is held to its bound by assert_within."""
    want = (y > 0).to(y2.dtype)
    bad = y2 != want
    n = int(bad.sum().item())
    if n:
        i = int(bad.reshape(-1).nonzero()[0].item())
        raise AssertionError(f"{what}: mask and output disagree on {n} of {bad.numel()} elements; first at flat index {i}: "
                             f"y {y.reshape(-1)[i].item():.6g}, y2 {y2.reshape(-1)[i].item():.6g}")


def assert_nan_footprint(got, ref, bound=None, what="", layout=None):
    """got is NaN on exactly the elements where the float64 reference is; everywhere else it is finite and within the bound.
    Returns (largest err / bound outside the footprint, number of NaN elements)."""
    if isinstance(ref, V):
        ref, bound = ref.v, ref.e
    g = got.to(D).reshape(ref.shape)
    foot = torch.isnan(ref)
    miss = foot != torch.isnan(g)
    if bool(miss.any()):
        i = int(miss.reshape(-1).nonzero()[0].item())
        loc, reg = _where(i, layout)
        raise AssertionError(f"{what}: NaN where the reference has none, or none where it has: {int(miss.sum().item())} elements, first at {loc} "
                             f"({', '.join(reg)}): got {g.reshape(-1)[i].item():.6g}, fp64 {ref.reshape(-1)[i].item():.6g}")
    assert bool(torch.isfinite(g[~foot]).all()), f"{what}: non-finite values outside the NaN footprint"
    z = torch.zeros_like(ref)
    return assert_within(torch.where(foot, z, g), torch.where(foot, z, ref), torch.where(foot, z, bound), what, layout), int(foot.sum().item())


def assert_rejects(got_with_defect, ref, bound=None, what=""):
    """the power check: a planted defect must push some element past its bound"""
    if isinstance(ref, V):
        ref, bound = ref.v, ref.e
    worst = ratio(got_with_defect, ref, bound).max().item()
    assert worst > 1.0, f"{what}: the bound does not see the planted defect (largest err/bound {worst:.3g})"
    return worst


def layout(g):
    """assert_within's layout of a conv output's rows"""
    return dict(B=g["B"], H=g["Hout"], W=g["Wout"], C=g["Cout"], creal=min(g["wrows"], g["Cout"]))


def accumulated(prev, add):
    """the fp32 destination of an accumulating call: prev (a tensor the kernel read, or a V) plus the call's result"""
    return _add(prev if isinstance(prev, V) else exact(prev), add)


def report(what, worst):
    print(f"fp64 bound {what}: max err/bound {worst:.3e}")
    return worst


# --------------------------------------------------------------------------------------------------------- planted defects

def border_mask(H, W, device=None):
    m = torch.zeros(H, W, dtype=torch.bool, device=device)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
    return m


def tile_mask(H, W, h0=0, w0=0, th=8, tw=16, device=None):
    m = torch.zeros(H, W, dtype=torch.bool, device=device)
    m[h0:h0 + th, w0:w0 + tw] = True
    return m


def conv_term(x, w, g, image, channels, tap=None, pixels=None):
    """rows (npix, Cout) fp64: the contribution of input channels `channels` (a slice) at one tap (None: all) of one image, limited to
    the output pixels of `pixels` ((Hout, Wout) mask, None: all) -- subtracted from a kernel's output it plants a missing term"""
    B, Hin, Win, Cin, Hout, Wout, Cout = (g[k] for k in ("B", "Hin", "Win", "Cin", "Hout", "Wout", "Cout"))
    X = _rows(x, B * Hin * Win, Cin).view(B, Hin, Win, Cin)[image:image + 1].to(D).permute(0, 3, 1, 2)
    W4 = _weights(w, g)
    keep = torch.zeros(Cin, dtype=D, device=x.device)
    keep[channels] = 1
    if W4.dim() == 2:
        W4 = W4 * keep
    else:
        W4 = W4 * keep.view(1, -1, 1, 1)
        if tap is not None:
            tm = torch.zeros(9, dtype=D, device=x.device)
            tm[tap] = 1
            W4 = W4 * tm.view(1, 1, 3, 3)
    t = _core(X, W4, g)[0].permute(1, 2, 0)  # (Hout, Wout, rows)
    if pixels is not None:
        t = t * pixels.to(x.device).view(Hout, Wout, 1)
    out = torch.zeros((B, Hout, Wout, Cout), dtype=D, device=x.device)
    out[image, :, :, : t.shape[-1]] = t
    return out.view(-1, Cout)
