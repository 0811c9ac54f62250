"""Float64 references, each with an element-wise error bound, of the kernels that consume the gradients and of the ones that condition the
network on time: the fused AdamW + EMA + shadow update, the EMA alone, the dynamic loss scale, the timestep embedding, the noise schedule,
the one-row Linear, the sampler's predictor / corrector and the remaining pointwise kernels (SiLU, sum-pool, upsample, cast).

Same contract as tests/fp64_ref.py, whose value-and-bound algebra this module reuses (V, _add, _mul, _rnd, _ksum_err ...): every function
takes the kernel's own operands, computes the operation in float64 and returns V(ref, bound); a correct kernel satisfies
|got - ref| <= bound element by element.  The module imports neither climate2weather_amd.ops nor tests/emu_ops.py.

Definitions the bounds are built on
  * The hyper-parameters are the fp32 values the C ABI receives: float(np.float32(lr)) and so on.  `1 - beta1`, `1 - beta2` and
    `1 - ema_rate` are formed FROM THOSE fp32 values in exact arithmetic (the kernel's `1.f - beta2`; for beta >= 0.5 that fp32
    subtraction is exact by Sterbenz' lemma, otherwise its one rounding is counted).  torch.optim.AdamW and the reference's ema.py form
    `1 - beta` in Python double from the double hyper-parameter and round afterwards: a second definition, u32 beta / (1 - beta) away in
    relative terms (tests/test_update_ref_cpu.py measures it).
  * The bias corrections are 1 - beta1^step and sqrt(1 - beta2^step) in double, rounded once to fp32 (pointwise.hip:1298-1299; on the
    device from state[3] + 1 with a scaler state, :793-795).  They enter as exact fp32 constants.
  * A product followed by a sum may be contracted into one fma or rounded twice; the two-rounding bound _add(_mul(a, b), c) contains the
    fused result, so it covers both (_mad).
  * sqrtf and fp32 division are correctly rounded (one u32 each, _sqrt / _div); below the fp32 normal range a result keeps fewer bits:
    every product / sum that can underflow adds DEN = 2^-150, half the denormal spacing (_den).
  * The fp32 SiLU (common.h:155-162): sigmoid(a) = rcp(1 + exp2(-1.4427f a)) with the raw instructions.  The product -1.4427f a is
    rounded (u32 |a| log2 e absolute in the exponent of 2) and the constant is itself ULOG2E away from log2 e: together a relative error
    |a| (u32 + ULOG2E) of the exponential, which reaches the sigmoid through d sigmoid / d exp = -(1 - s) s.  fp64_ref._silu / _dsilu
    (K_ULP fp32 ulps) omit it because it vanishes under a bf16 / fp16 rounding; silu32 / dsilu32 add it.  exp2 and rcp flush denormal
    results: sigmoid is off by up to FLUSH = 2^-126 absolutely where it underflows (a < -87), every route.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from fp64_ref import D, DSILU_SLOPE, K_ULP, SILU_SLOPE, U32, V, _T, _add, _dsilu, _ksum_err, _mul, _rnd, _silu, _sub, _v, exact

DEN = 2.0 ** -150  # half the spacing of fp32 denormals
FLUSH = 2.0 ** -126  # the smallest fp32 normal: what v_exp_f32 / v_rcp_f32 flush to zero
LOG2E_F = float(np.float32(1.44269504088896341))
ULOG2E = abs(LOG2E_F - math.log2(math.e)) / math.log2(math.e)
ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 3  # include/c2w_hip.h
GRID_CAP = 8192  # grid_for's default cap (pointwise.hip:860, sampler.hip:13)
PASS = GRID_CAP * 256  # elements (or 16-byte vectors) one pass of a grid-stride loop covers
CHECK_PASS = 4096 * 256 * 4  # scaler_check_kernel: 4096 blocks, one float4 per thread (pointwise.hip:1325)
UPSAMPLE_PASS = 16384 * 256  # upsample2_kernel: 16384 blocks, one 16-byte vector per thread (pointwise.hip:1008)


def f32(x):
    """the fp32 value a Python float becomes in the C ABI, as a Python float"""
    return float(np.float32(x))


def one_minus(beta):
    """(the exact 1 - beta of the fp32 beta, the distance of the kernel's fp32 `1.f - beta` from it)"""
    b = f32(beta)
    return 1.0 - b, abs(float(np.float32(1.0) - np.float32(b)) - (1.0 - b))


def bias_corrections(beta1, beta2, step):
    """pointwise.hip:1298-1299 / :793-795: double arithmetic on the fp32 betas, rounded once to fp32"""
    return f32(1.0 - f32(beta1) ** float(step)), f32(math.sqrt(1.0 - f32(beta2) ** float(step)))


def _s(x, like, e=0.0):
    """a scalar V on the device of `like`"""
    t = like.v if isinstance(like, V) else like
    return V(torch.tensor(float(x), dtype=D, device=t.device), torch.tensor(float(e), dtype=D, device=t.device))


def _den(a):
    return V(a.v, a.e + DEN)


def _mulf(a, b):
    """an fp32 product that may land below the normal range"""
    return _den(_mul(a, b))


def _mad(a, b, c, sign=1.0):
    """c + sign * a * b, fused or rounded twice: the two-rounding bound contains the fused result"""
    return _den(_add(c, _mulf(a, b), sign))


def _sqrt(a):
    """correctly rounded sqrtf of a non-negative V: the propagated error by the function's own values (it is concave: the lower side is
    the wider one unless the radicand's bound reaches zero), plus one rounding"""
    v = a.v.clamp_min(0).sqrt()
    lo = (a.v - a.e).clamp_min(0).sqrt()
    hi = (a.v + a.e).clamp_min(0).sqrt()
    e = torch.maximum(v - lo, hi - v)
    return V(v, e + U32 * (v + e))


def _div(a, b):
    """correctly rounded fp32 a / b, b bounded away from zero by its own bound"""
    a, b = _v(a), _v(b)
    v = a.v / b.v
    lo = (b.v.abs() - b.e).clamp_min(1e-300)
    e = (a.e + v.abs() * b.e) / lo
    return _den(V(v, e + U32 * (v.abs() + e)))


# ------------------------------------------------------------------------------------------------------------ parameter update

def ema_step(ema, p, rate):
    """ema_kernel (pointwise.hip:857) and the EMA line of adamw_ema_kernel (:800, :813): rate * ema + (1.f - rate) * p.  ema: the fp32
    tensor before the call; p: fp32 tensor or V (the updated parameter)."""
    ema = exact(ema) if not isinstance(ema, V) else ema
    p = exact(p) if not isinstance(p, V) else p
    om, om_e = one_minus(rate)
    return _mad(_s(om, ema, om_e), p, _mulf(_s(f32(rate), ema), ema))


def adamw_step(p, g, m, v, ema, hyper, step, grad_scale, scaler_state=None, shadow_dtype=None, shadow_prev=None, variant=None):
    """adamw_ema_kernel (pointwise.hip:784-816) restated statement by statement: returns (p', m', v', ema', shadow') as V (ema' / shadow'
    None where the call has none).  p, g, m, v, ema: the fp32 tensors BEFORE the call.  hyper: dict(lr, beta1, beta2, eps, wd, ema_rate).
    scaler_state: None or the four floats {scale, tracker, found_inf, steps taken} before the call -- then step = state[3] + 1 and the
    gradient is multiplied by the fp32 value grad_scale / state[0]; with found_inf set the step is skipped: p, m, v (and the shadow,
    shadow_prev) come back with bound 0 and only the EMA moves.
    variant: a planted defect as a variant reference -- ('bc', +1 / -1) bias corrections one step off, 'eps_inside' (eps added before
    the division by bc2_sqrt), 'coupled_wd' (g + wd p), 'ema_old_p', 'no_unscale'."""
    lr, b1, b2, eps, wd, rate = (f32(hyper[k]) for k in ("lr", "beta1", "beta2", "eps", "wd", "ema_rate"))
    P, G, M, Vv = exact(p), exact(g), exact(m), exact(v)
    gs = f32(grad_scale)
    skip = False
    if scaler_state is not None:
        st = [float(x) for x in scaler_state]
        if variant != "no_unscale":
            gs = float(np.float32(gs) / np.float32(st[0]))  # :791, one fp32 division: the value the definition multiplies by
        skip = st[2] != 0.0
        step = int(st[3]) + 1
    if skip:  # :797-802
        e2 = ema_step(ema, P, rate) if ema is not None else None
        return P, M, Vv, e2, (exact(shadow_prev) if shadow_prev is not None else None)
    if isinstance(variant, tuple) and variant[0] == "bc":
        step = step + variant[1]
    bc1, bc2 = bias_corrections(b1, b2, step)
    om1, om1_e = one_minus(b1)
    om2, om2_e = one_minus(b2)
    gi = _mulf(G, _s(gs, G))  # :804
    if variant == "coupled_wd":
        gi = _mad(_s(wd, G), P, gi)
        pi = P
    else:
        decay = 1.0 - lr * wd  # :805, `1.f - lr * wd`: the product and the difference round once each (or once, fused)
        pi = _mulf(P, _s(decay, P, U32 * (abs(lr * wd) + abs(decay))))
    mi = _mad(_s(om1, G, om1_e), gi, _mulf(_s(b1, M), M))  # :806
    vi = _add(_mulf(_s(b2, Vv), Vv), _mulf(_mulf(_s(om2, G, om2_e), gi), gi))  # :807, ((1 - beta2) * gi) * gi
    vi = _den(V(vi.v, vi.e))
    if variant == "eps_inside":
        denom = _div(_add(_sqrt(vi), _s(eps, G)), _s(bc2, G))
    else:
        denom = _add(_div(_sqrt(vi), _s(bc2, G)), _s(eps, G))  # :808
    rate_s = lr / bc1
    upd = _mulf(_s(rate_s, G, U32 * abs(rate_s)), _div(mi, denom))  # :809, (lr / bc1) * (mi / denom)
    pn = _den(_sub(pi, upd))
    e2 = ema_step(ema, P if variant == "ema_old_p" else pn, rate) if ema is not None else None  # :813
    sh = _rnd(pn, shadow_dtype) if shadow_dtype is not None else None  # :814
    return pn, mi, vi, e2, sh


def scaler_model(flags, init, growth, backoff, interval):
    """scaler_update_kernel (pointwise.hip:836-852) after each step of a found-inf flag sequence, from scaler_init_kernel's state: a list of
    [scale, tracker, 0, steps taken] per step.  Every scale is init times a power of two (growth, backoff powers of two): exact in fp32."""
    scale, tracker, taken = f32(init), 0.0, 0.0
    out = []
    for bad in flags:
        if bad:
            scale, tracker = f32(scale * f32(backoff)), 0.0
        else:
            taken += 1.0
            tracker += 1.0
            if tracker >= float(interval):
                scale, tracker = f32(scale * f32(growth)), 0.0
        out.append([scale, tracker, 0.0, taken])
    return out


# ------------------------------------------------------------------------------------------------------------ time conditioning

def timestep_embedding(t, dim, max_period=10000.0):
    """timestep_embedding_kernel (pointwise.hip:676-689): out[b] = [cos(t f_k) | sin(t f_k)], f_k = exp(-ln(P) k / half); (n, dim) V.
    The argument t * expf(-logf(P) * k / half) carries logf (K_ULP ulps), the product and the division (u32 each) as an absolute error of
    the exponent, expf's K_ULP ulps, and the final product; cos and sin have slope at most 1 and K_ULP ulps of their own.  An odd dim
    leaves its last column exactly 0."""
    half = dim // 2
    T = t.reshape(-1).to(D)
    k = torch.arange(half, dtype=D, device=t.device)
    L = math.log(f32(max_period))
    x = -L * k / half
    e_x = x.abs() * (K_ULP + 2) * U32
    f = x.exp()
    freq = V(f, f * (torch.expm1(e_x) + K_ULP * U32))
    a = _mulf(V(T.unsqueeze(1).expand(-1, half)), V(freq.v.unsqueeze(0), freq.e.unsqueeze(0)))
    c, s = a.v.cos(), a.v.sin()
    out_v = torch.zeros((T.numel(), dim), dtype=D, device=t.device)
    out_e = torch.zeros_like(out_v)
    out_v[:, :half], out_v[:, half:2 * half] = c, s
    out_e[:, :half] = a.e + K_ULP * U32 * c.abs() + DEN
    out_e[:, half:2 * half] = a.e + K_ULP * U32 * s.abs() + DEN
    return V(out_v, out_e)


def mu_sigma(t, eta):
    """mu_sigma_kernel (pointwise.hip:692-699): (mu V, sigma V) with mu = a = cos^2(acos(sqrt(eta)) t), sigma = sqrt(1 - a^2 + eta^2).
    sqrtf, acosf and cosf are K_ULP ulps each; acos has slope 1 / sqrt(1 - r^2) at r = sqrt(eta), cos slope at most 1.  The radicand
    1 - a^2 + eta^2 cancels towards eta^2 as t -> 0: its absolute error 2 |a| e_a + ... does not shrink with it, and the square root
    divides it by 2 sigma (_sqrt takes the function's own values, so the bound stays finite where it reaches the radicand)."""
    T = t.reshape(-1).to(D)
    et = f32(eta)
    r = math.sqrt(et)
    e_r = K_ULP * U32 * r
    w = math.acos(r)
    e_w = e_r / math.sqrt(1 - r * r) + K_ULP * U32 * w
    x = _mulf(_s(w, T, e_w), V(T))
    c = x.v.cos()
    cv = V(c, x.e + K_ULP * U32 * c.abs())
    a = _mulf(cv, cv)
    rad = _mad(_s(et, T), _s(et, T), _mad(a, a, _s(1.0, T), -1.0))  # (1.f - a * a) + eta * eta
    return a, _sqrt(rad)


# The conditioning of sigma(t) at eta = 1e-3, as the largest relative error of the kernel's fp32 statement order with sqrtf, acosf and
# cosf rounded correctly (tests/test_update_ref_cpu.py measures it and holds these figures): t < 1e-3, 1e-3 <= t < 1e-2, t >= 0.1.
SIGMA_BANDS_CPU = (5.10e-2, 9.68e-3, 1.97e-6)


def sigma_bands(t, rel):
    """the largest of rel over the three bands of t"""
    t = t.reshape(-1).to(rel.device)
    return [rel[m].max().item() for m in (t < 1e-3, (t >= 1e-3) & (t < 1e-2), t >= 0.1)]


def _sig32_rel(a, s):
    """relative error of sigmoid_f at fp32 (common.h:155-157): K_ULP ulps, plus the exponent's rounding |a| (u32 + ULOG2E) (1 - s)"""
    return K_ULP * U32 + a.abs() * (U32 + ULOG2E) * (1 - s)


def silu32(a):
    """silu_f at fp32: a * sigmoid(a), the sigmoid's relative error times |a s|, plus the flush of a denormal sigmoid"""
    s = torch.sigmoid(a.v)
    v = a.v * s
    return V(v, SILU_SLOPE * a.e + v.abs() * _sig32_rel(a.v, s) + a.v.abs() * FLUSH + DEN)


def dsilu32(a):
    """dsilu_f at fp32 (common.h:159-162): s (1 + a (1 - s)); d/ds = 1 + a (1 - 2 s) carries the sigmoid's argument term"""
    s = torch.sigmoid(a.v)
    h = a.v * s
    v = s + h * (1 - s)
    arg = a.v.abs() * (U32 + ULOG2E) * (1 - s) * s
    return V(v, DSILU_SLOPE * a.e + K_ULP * U32 * (s + h.abs()) + (1 + a.v * (1 - 2 * s)).abs() * arg + (1 + a.v.abs()) * FLUSH + DEN)


def _flushed(o, k):
    """o with the flush of a denormal sigmoid, which reaches the result with weight k"""
    return V(o.v, o.e + k * FLUSH)


def silu(x, dtype):
    """c2w_silu: silu_kernel<T, 0> (pointwise.hip:249): fp32 through silu32; the 16-bit routes keep fp64_ref._silu (plus the flush of a
    denormal sigmoid, which the instruction performs on every route), then one rounding to T"""
    a = exact(x)
    if _T(dtype) == torch.float32:
        return silu32(a)
    return _rnd(_flushed(_silu(a), a.v.abs()), dtype)


def silu_backward(x, dy, dtype):
    """c2w_silu_backward: silu_kernel<T, 1> (pointwise.hip:254): dy * silu'(x), rounded to T"""
    a = exact(x)
    d = dsilu32(a) if _T(dtype) == torch.float32 else _flushed(_dsilu(a), 1 + a.v.abs())
    o = _mulf(exact(dy), d)
    return o if _T(dtype) == torch.float32 else _rnd(o, dtype)


def gemv_chain(K, ldk):
    """the longest dependent chain of gemv_f32_kernel (pointwise.hip:1215-1226): the lane's fma chain and the 6-level wave tree"""
    vec = K % 4 == 0 and ldk % 4 == 0
    return (4 * -(-K // 256) if vec else -(-K // 64)) + 6


def gemv_lane_mask(K, ldk, lane, device=None):
    """the k a lane of the wave owns: float4 k = 4 lane + 256 j .. + 3 in the vector route, k = lane + 64 j in the scalar one"""
    k = torch.arange(K, device=device)
    return (k % 256) // 4 == lane if (K % 4 == 0 and ldk % 4 == 0) else k % 64 == lane


def gemv_partial(x, W, rows, K, ldk, mask):
    """fp64 sum over the k of `mask` of W[r][k] x[k]: subtracted from a kernel's output it plants the missing terms"""
    Wm = W.reshape(-1)[: rows * ldk].view(rows, ldk)[:, :K].to(D)
    return (Wm * (x.reshape(-1)[:K].to(D) * mask.to(D))).sum(1)


def gemv(x, W, bias, rows, K, ldk, act):
    """gemv_f32_kernel: y[r] = act(bias[r] + W[r][:K] . x) as V (rows,).  The dot product is a chain of gemv_chain(K, ldk) dependent
    fp32 operations; ACT_SILU goes through silu32, ACT_RELU is exact on the sum."""
    Wm = W.reshape(-1)[: rows * ldk].view(rows, ldk)[:, :K].to(D)
    t = Wm * x.reshape(-1)[:K].to(D)
    s = t.sum(1)
    acc = V(s, _ksum_err(s, (t * t).sum(1), t.abs().sum(1), gemv_chain(K, ldk)) + DEN)
    if bias is not None:
        acc = _add(acc, exact(bias.reshape(-1)[:rows]))
    if act == ACT_SILU:
        return silu32(acc)
    if act == ACT_RELU:
        return V(acc.v.clamp_min(0), acc.e)
    return acc


# --------------------------------------------------------------------------------------------------------------------- sampler

def predict(x, eps, a, b):
    """predict_kernel (sampler.hip:165): a * x + b * eps with the fp32 scalars a, b"""
    X, E = exact(x), exact(eps)
    return _mad(_s(f32(b), X), E, _mulf(_s(f32(a), X), X))


def correct_scalars(sumsq, n, tau, like):
    """correct_kernel (sampler.hip:183-184): delta = tau / (sumsq / (float) n), sd = sqrtf(2 delta) as scalar V.  sumsq: the fp32 tensor
    the kernel reads, or a V (fp64_ref.sumsq of the same eps: its bound enters delta)."""
    S = sumsq if isinstance(sumsq, V) else exact(sumsq.reshape(-1)[0])
    S = V(S.v.reshape(()), S.e.reshape(()))
    nf = f32(n)
    mean = _div(S, _s(nf, like, abs(nf - n)))
    delta = _div(_s(f32(tau), like), mean)
    return delta, _sqrt(V(2 * delta.v, 2 * delta.e))


def correct(x, eps, z, sumsq, n, tau, sigma_next):
    """correct_kernel (sampler.hip:187): x - (delta * eps + sd * z) * sigma_next"""
    X, E, Z = exact(x), exact(eps), exact(z)
    delta, sd = correct_scalars(sumsq, n, tau, X)
    return _den(_sub(X, _mulf(_mad(sd, Z, _mulf(delta, E)), _s(f32(sigma_next), X))))


# ------------------------------------------------------------------------------------------------------------------- pointwise

def sumpool2(g, B, H, W, C, dtype, order=(0, 1, 2, 3)):
    """sumpool2_kernel (pointwise.hip:273-285): ((g00 + g01) + g10) + g11 in fp32 (the first addition onto 0 is exact), one rounding to T.
    g: (B, 2H, 2W, C) rows -> V (B * H * W, C).  order: another summation order, for the planted defect."""
    q = g.reshape(-1)[: B * 4 * H * W * C].view(B, H, 2, W, 2, C).to(D)
    t = [V(q[:, :, 0, :, 0]), V(q[:, :, 0, :, 1]), V(q[:, :, 1, :, 0]), V(q[:, :, 1, :, 1])]
    s = _add(_add(_add(t[order[0]], t[order[1]]), t[order[2]]), t[order[3]])
    return _rnd(s, dtype).view(B * H * W, C)


def sumpool2_fp32_chain(g, B, H, W, C, order):
    """the fp32 chain itself in another order (numpy float32): what a kernel that sums differently would store at fp32"""
    q = g.reshape(-1)[: B * 4 * H * W * C].view(B, H, 2, W, 2, C).float().cpu().numpy()
    t = [q[:, :, 0, :, 0], q[:, :, 0, :, 1], q[:, :, 1, :, 0], q[:, :, 1, :, 1]]
    return torch.from_numpy(((t[order[0]] + t[order[1]]) + t[order[2]]) + t[order[3]]).reshape(B * H * W, C)


def upsample2(x, B, H, W, C):
    """upsample2_kernel (pointwise.hip:296-304): y[b][2h+i][2w+j] = x[b][h][w], exact; (B * 2H * 2W, C) in x's own dtype"""
    q = x.reshape(-1)[: B * H * W * C].view(B, H, 1, W, 1, C)
    return q.expand(B, H, 2, W, 2, C).reshape(B * 4 * H * W, C)


def cast_bits(a, dtype):
    """fp32 -> bf16 / fp16 by round-to-nearest-even on the bit pattern (numpy integers, no conversion instruction of any library):
    returns the uint16 bit patterns; NaN becomes the quiet NaN 0x7fc0 / 0x7e00 with the sign kept.  fp16: values of magnitude >= 65520
    overflow to inf, results below 2^-14 are subnormal, magnitudes <= 2^-25 round to zero."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    sign = (b >> np.uint64(31)) & np.uint64(1)
    expo = (b >> np.uint64(23)) & np.uint64(0xFF)
    man = b & np.uint64(0x7FFFFF)
    nan = (expo == 255) & (man != 0)
    inf = (expo == 255) & (man == 0)
    T = _T(dtype)
    if T == torch.bfloat16:
        mag = b & np.uint64(0x7FFFFFFF)
        out = (mag + np.uint64(0x7FFF) + ((mag >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
        out = np.where(nan, np.uint64(0x7FC0), out)
        return (out | (sign << np.uint64(15))).astype(np.uint16)
    if T != torch.float16:
        raise ValueError(dtype)
    e = expo.astype(np.int64) - 127 + 15
    normal = e >= 1
    # normal results drop 13 mantissa bits under the exponent field; subnormal ones shift the 24-bit significand by 14 - e more
    sig = np.where(normal, man, man | np.uint64(0x800000))
    shift = np.where(normal, 13, np.clip(14 - e, 14, 40)).astype(np.uint64)
    q = sig >> shift
    rem = sig & ((np.uint64(1) << shift) - np.uint64(1))
    halfway = np.uint64(1) << (shift - np.uint64(1))
    up = (rem > halfway) | ((rem == halfway) & ((q & np.uint64(1)) == 1))
    out = np.where(normal, (np.clip(e, 0, 31).astype(np.uint64) << np.uint64(10)) + q, q) + up.astype(np.uint64)  # a carry moves into the exponent
    out = np.where((e >= 31) | inf | (out > 0x7C00), np.uint64(0x7C00), out)
    out = np.where(expo == 0, np.uint64(0), out)  # fp32 zeros and denormals
    out = np.where(nan, np.uint64(0x7E00), out)
    return (out | (sign << np.uint64(15))).astype(np.uint16)


def cast(src, dtype):
    """cast_f32_kernel (pointwise.hip:702-705): a tensor of the storage type holding cast_bits of the fp32 tensor src"""
    bits = cast_bits(src.detach().float().cpu().numpy(), dtype)
    return torch.from_numpy(bits.view(np.int16).copy()).view(_T(dtype)).to(src.device)


def truncate(src, dtype):
    """fp32 -> T by dropping bits (round towards zero): the planted shadow defect"""
    T = _T(dtype)
    h = src.to(T)
    over = h.to(torch.float32).abs() > src.abs()
    bits = h.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(T)


def cast_edge_values():
    """fp32 inputs at which a conversion goes wrong: every tie pattern around 1.0 for both 16-bit types, the fp16 overflow boundary, fp16
    subnormals and the largest value that rounds to zero, +-0, +-inf, NaN, the largest finite float, an fp32 denormal"""
    bits = []
    for drop in (16, 13):  # bf16 / fp16 drop this many mantissa bits
        half = 1 << (drop - 1)
        for base in (0x3F800000, 0x3F800000 + (1 << drop), 0x3F800000 - (1 << drop), 0x3F7FFFFF & ~((1 << drop) - 1)):
            bits += [base + d for d in (0, 1, half - 1, half, half + 1, (1 << drop) - 1)]
    vals = np.array(bits, dtype=np.uint32).view(np.float32).tolist()
    vals += [65504.0, 65519.0, 65519.996, 65520.0, 65520.004, 65536.0, 1e5, 3.4028234663852886e38, 3.3895313892515355e38]
    vals += [2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -11), 2.0 ** -14 * (1 - 2.0 ** -12), 2.0 ** -24, 2.0 ** -24 * 1.5, 2.0 ** -24 * 2.5, 2.0 ** -25,
             float(np.nextafter(np.float32(2.0 ** -25), np.float32(1))), float(np.nextafter(np.float32(2.0 ** -25), np.float32(0))), 2.0 ** -26,
             3 * 2.0 ** -25, 1e-30, 1e-40, 0.0]
    v = np.array(vals, dtype=np.float32)
    v = np.concatenate([v, -v, np.array([np.inf, -np.inf, np.nan], dtype=np.float32)])
    return torch.from_numpy(v)
