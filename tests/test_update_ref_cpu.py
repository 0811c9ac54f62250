"""tests/fp64_update_ref.py checked without a GPU: the references equal the textbook formulas in a scalar Python-float loop; a float32 numpy
restatement of each kernel's statement order stays inside the bound and fills a visible part of it; every planted defect of the GPU tier
is rejected on that restatement; torch.optim.AdamW and ema.py's update -- the SECOND definition of `1 - beta` / `1 - rate` -- are measured
against the reference; the numpy cast reference equals torch's conversion on the edge tensor."""
import math

import numpy as np
import pytest
import torch

import fp64_ref as R
import fp64_update_ref as U

f4 = np.float32
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-3, ema_rate=0.9999)
U32 = R.U32


def _state(n, seed, step):
    g_ = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g_) * torch.tensor([0.0, 0.05, 30.0]).repeat(-(-n // 3))[:n]
    g = torch.randn(n, generator=g_).sign() * 10 ** (torch.rand(n, generator=g_) * 16 - 12)
    g[::17] = 0
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        gp = g * (0.5 + torch.rand(n, generator=g_))
        m, v = gp * 0.3, gp * gp * 0.7
    return p.float(), g.float(), m.float(), v.float(), (p + 0.01 * torch.randn(n, generator=g_)).float()


def adamw_np(p, g, m, v, ema, h, step, gs, scaler=None, defect=None):
    """adamw_ema_kernel's statements in numpy float32, unfused; returns (p, m, v, ema).  defect 'double_consts': 1 - beta and 1 - rate
    formed in Python double and rounded, as torch.optim.AdamW and ema.py form them"""
    p, g, m, v, ema = (x.numpy().astype(f4) for x in (p, g, m, v, ema))
    lr, b1, b2, eps, wd, rate = (f4(h[k]) for k in ("lr", "beta1", "beta2", "eps", "wd", "ema_rate"))
    gs = f4(gs)
    if scaler is not None:
        if defect != "no_unscale":
            gs = gs / f4(scaler[0])
        step = int(scaler[3]) + 1
        if scaler[2] != 0:
            return p, m, v, rate * ema + (f4(1) - rate) * p
    if isinstance(defect, tuple):
        step += defect[1]
    bc1 = f4(1.0 - float(b1) ** step)
    bc2 = f4(math.sqrt(1.0 - float(b2) ** step))
    gi = g * gs
    if defect == "coupled_wd":
        gi = gi + wd * p
        pi = p.copy()
    else:
        pi = p * (f4(1) - lr * wd)
    om1, om2, omr = f4(1) - b1, f4(1) - b2, f4(1) - rate
    if defect == "double_consts":
        om1, om2, omr = f4(1 - h["beta1"]), f4(1 - h["beta2"]), f4(1 - h["ema_rate"])
    mi = b1 * m + om1 * gi
    vi = b2 * v + om2 * gi * gi
    denom = (np.sqrt(vi) + eps) / bc2 if defect == "eps_inside" else np.sqrt(vi) / bc2 + eps
    pi = pi - (lr / bc1) * (mi / denom)
    e2 = rate * ema + omr * (p if defect == "ema_old_p" else pi)
    return pi, mi, vi, e2


# ------------------------------------------------------------------------------------------------- the reference is the textbook

@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_adamw_reference_equals_the_textbook_scalar_loop(step, wd):
    h = dict(HYPER, wd=wd)
    p, g, m, v, ema = _state(12, 3, step)
    pn, mn, vn, en, _ = U.adamw_step(p, g, m, v, ema, h, step, 0.5)
    lr, b1, b2, eps, wdf, rate = (U.f32(h[k]) for k in ("lr", "beta1", "beta2", "eps", "wd", "ema_rate"))
    bc1, bc2 = U.f32(1 - b1 ** step), U.f32(math.sqrt(1 - b2 ** step))
    for i in range(12):
        gi = float(g[i]) * 0.5
        mi = b1 * float(m[i]) + (1 - b1) * gi
        vi = b2 * float(v[i]) + (1 - b2) * gi * gi
        pi = float(p[i]) * (1 - lr * wdf) - (lr / bc1) * mi / (math.sqrt(vi) / bc2 + eps)
        ei = rate * float(ema[i]) + (1 - rate) * pi
        for name, ref, want in (("p", pn, pi), ("m", mn, mi), ("v", vn, vi), ("ema", en, ei)):
            assert abs(ref.v[i].item() - want) <= 1e-13 * max(abs(want), 1e-30), (name, i, ref.v[i].item(), want)


def test_ema_schedule_embedding_gemv_references_equal_scalar_loops():
    ema, p = torch.randn(12), torch.randn(12)
    r = U.ema_step(ema, p, 0.9999)
    rate = U.f32(0.9999)
    for i in range(12):
        assert abs(r.v[i].item() - (rate * float(ema[i]) + (1 - rate) * float(p[i]))) < 1e-15
    t = torch.tensor([0.0, 1e-5, 1e-3, 0.1, 0.25, 0.5, 0.7, 0.9, 0.99, 1.0, 0.33, 0.66])
    for eta in (1e-3, 1e-2):
        mu, sg = U.mu_sigma(t, eta)
        et = U.f32(eta)
        for i in range(12):
            a = math.cos(math.acos(math.sqrt(et)) * float(t[i])) ** 2
            assert abs(mu.v[i].item() - a) < 1e-15 and abs(sg.v[i].item() - math.sqrt(1 - a * a + et * et)) < 1e-12
    for dim in (8, 9):
        emb = U.timestep_embedding(t, dim, 10000.0)
        half = dim // 2
        for i in range(12):
            for k in range(half):
                a = float(t[i]) * math.exp(-math.log(10000.0) * k / half)
                assert abs(emb.v[i, k].item() - math.cos(a)) < 1e-14 and abs(emb.v[i, half + k].item() - math.sin(a)) < 1e-14
        if dim % 2:
            assert (emb.v[:, -1] == 0).all() and (emb.e[:, -1] == 0).all()
    rows, K, ldk = 5, 7, 9
    x, W, b = torch.randn(K), torch.randn(rows * ldk), torch.randn(rows)
    for act in (U.ACT_NONE, U.ACT_SILU, U.ACT_RELU):
        y = U.gemv(x, W, b, rows, K, ldk, act)
        for r_ in range(rows):
            s = float(b[r_]) + sum(float(W[r_ * ldk + k]) * float(x[k]) for k in range(K))
            want = s / (1 + math.exp(-s)) if act == U.ACT_SILU else (max(s, 0.0) if act == U.ACT_RELU else s)
            assert abs(y.v[r_].item() - want) < 1e-13


def test_scaler_model_follows_gradscalers_rule():
    got = U.scaler_model([0, 0, 1, 0, 0, 0, 1, 1, 0], 1024.0, 2.0, 0.5, 3)
    assert got[1] == [1024.0, 2.0, 0.0, 2.0] and got[2] == [512.0, 0.0, 0.0, 2.0]
    assert got[5] == [1024.0, 0.0, 0.0, 5.0] and got[7] == [256.0, 0.0, 0.0, 5.0] and got[8] == [256.0, 1.0, 0.0, 6.0]


# ----------------------------------------------------------------------- float32 restatements: inside the bound, and filling it

def _gemv_np(x, W, b, rows, K, ldk, act, drop=None):
    """gemv_f32_kernel in numpy float32: per-lane chains in the kernel's k order (products rounded: unfused), the xor tree, bias, act"""
    vec = K % 4 == 0 and ldk % 4 == 0
    Wm = W.numpy().reshape(-1)[: rows * ldk].reshape(rows, ldk)
    xn = x.numpy()
    out = np.zeros(rows, dtype=f4)
    for r in range(rows):
        lanes = np.zeros(64, dtype=f4)
        for lane in range(64):
            ks = [k + e for k in range(lane * 4, K, 256) for e in range(4)] if vec else list(range(lane, K, 64))
            s = f4(0)
            for k in ks:
                if drop is not None and drop(lane, k):
                    continue
                s = f4(s + f4(Wm[r, k] * xn[k]))
            lanes[lane] = s
        for o in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[np.arange(64) ^ o]
        s = lanes[0] + (b.numpy()[r] if b is not None else f4(0))
        out[r] = _silu_np(s) if act == U.ACT_SILU else (max(s, f4(0)) if act == U.ACT_RELU else s)
    return out


def _sig_np(a):
    a = np.asarray(a, dtype=f4)
    with np.errstate(over="ignore"):
        return (f4(1) / (f4(1) + np.exp2(f4(-1.44269504088896341) * a).astype(f4))).astype(f4)


def _silu_np(a):
    return (np.asarray(a, dtype=f4) * _sig_np(a)).astype(f4)


def _dsilu_np(a):
    a = np.asarray(a, dtype=f4)
    s = _sig_np(a)
    return (s * (f4(1) + a * (f4(1) - s))).astype(f4)


def _mu_sigma_np(t, eta):
    """mu_sigma_kernel with sqrtf / acosf / cosf rounded correctly (float64 functions rounded once): independent of the host's libm"""
    t = np.asarray(t, dtype=f4)
    w = f4(math.acos(float(f4(math.sqrt(float(f4(eta)))))))
    c = np.cos((w * t).astype(np.float64)).astype(f4)
    a = c * c
    return a, np.sqrt(f4(1) - a * a + f4(eta) * f4(eta))


@pytest.mark.parametrize("step,gs,scaler", [(1, 0.5, None), (2, 1.0, None), (1000, 1.0, None), (7, 1.0, [1024.0, 1.0, 0.0, 999.0]),
                                            (7, 1.0, [65536.0, 0.0, 1.0, 0.0])])
def test_adamw_restatement_within_the_bound_and_the_bound_is_not_vacuous(step, gs, scaler):
    n = 6000
    p, g, m, v, ema = _state(n, step, step)
    if scaler is not None:
        g = g * scaler[0]
    got = adamw_np(p, g, m, v, ema, HYPER, step, gs, scaler)
    ref = U.adamw_step(p, g, m, v, ema, HYPER, step, gs, scaler, torch.bfloat16, shadow_prev=p.to(torch.bfloat16))
    worst = [R.assert_within(torch.from_numpy(got[i]), ref[i], what=f"adamw restatement {name} step {step}") for i, name in enumerate("pmv")]
    worst.append(R.assert_within(torch.from_numpy(got[3]), ref[3], what="adamw restatement ema"))
    print(f"adamw restatement step {step}: err/bound p {worst[0]:.3g} m {worst[1]:.3g} v {worst[2]:.3g} ema {worst[3]:.3g}")
    if scaler is not None and scaler[2]:
        assert all((ref[i].e == 0).all() and np.array_equal(got[i], x.numpy()) for i, x in enumerate((p, m, v)))
        assert (ref[4].e == 0).all() and torch.equal(ref[4].v, p.to(torch.bfloat16).double())
    else:
        assert min(worst[:3]) > 1e-3
        sh = torch.from_numpy(got[0]).to(torch.bfloat16)
        R.assert_within(sh, ref[4], what="shadow")
    assert worst[3] > 1e-3


def test_pointwise_restatements_within_the_bound():
    g_ = torch.Generator().manual_seed(5)
    ema, p = torch.randn(4000, generator=g_), torch.randn(4000, generator=g_)
    for rate in (0.9999, 0.999, 0.0, 1.0):
        got = f4(rate) * ema.numpy() + (f4(1) - f4(rate)) * p.numpy()
        R.assert_within(torch.from_numpy(got), U.ema_step(ema, p, rate), what=f"ema rate {rate}")
    t = torch.cat([torch.tensor([0.0, 1.0, 2.0 ** -126, 1e-4]), torch.linspace(0, 1, 200)])
    for dim, P in ((32, 10000.0), (33, 10.0)):
        half = dim // 2
        k = np.arange(half, dtype=f4)
        freq = np.exp((-np.log(f4(P)) * k / f4(half)).astype(f4)).astype(f4)
        a = t.numpy()[:, None] * freq[None, :]
        got = np.zeros((t.numel(), dim), dtype=f4)
        got[:, :half], got[:, half:2 * half] = np.cos(a), np.sin(a)
        R.assert_within(torch.from_numpy(got), U.timestep_embedding(t, dim, P), what=f"embedding dim {dim}")
    x = torch.cat([torch.randn(5000, generator=g_) * 3, torch.tensor([0.0, 1e-30, 20.0, 40.0, 88.0, 100.0]), -torch.tensor([0.0, 1e-30, 20.0, 40.0, 88.0, 100.0])])
    dy = torch.randn(x.numel(), generator=g_)
    w1 = R.assert_within(torch.from_numpy(_silu_np(x.numpy())), U.silu(x, torch.float32), what="silu fp32")
    w2 = R.assert_within(torch.from_numpy(dy.numpy() * _dsilu_np(x.numpy())), U.silu_backward(x, dy, torch.float32), what="dsilu fp32")
    print(f"fp32 silu restatement err/bound {w1:.3g}, silu' {w2:.3g}")
    assert w1 > 1e-3 and w2 > 1e-3
    for T in (torch.bfloat16, torch.float16):
        xt = x.to(T)
        R.assert_within(torch.from_numpy(_silu_np(xt.float().numpy())).to(T), U.silu(xt, T), what=f"silu {T}")
        R.assert_within(torch.from_numpy(dy.to(T).float().numpy() * _dsilu_np(xt.float().numpy())).to(T), U.silu_backward(xt, dy.to(T), T), what=f"dsilu {T}")
    n = 3000
    xs, es, zs = (torch.randn(n, generator=g_) for _ in range(3))
    a, b = U.f32(0.97), U.f32(-0.013)
    R.assert_within(torch.from_numpy(f4(a) * xs.numpy() + f4(b) * es.numpy()), U.predict(xs, es, a, b), what="predict")
    ss = torch.tensor([float((es.numpy() * es.numpy()).sum(dtype=f4))])
    delta = f4(0.7) / (ss.numpy()[0] / f4(n))
    got = xs.numpy() - (delta * es.numpy() + np.sqrt(f4(2) * delta) * zs.numpy()) * f4(0.05)
    R.assert_within(torch.from_numpy(got), U.correct(xs, es, zs, ss, n, 0.7, 0.05), what="correct, the kernel's own sumsq")
    R.assert_within(torch.from_numpy(got), U.correct(xs, es, zs, R.sumsq(es, n), n, 0.7, 0.05), what="correct, sumsq as a bounded value")


def test_the_fp32_silu_argument_term_is_needed_and_sufficient():
    """at |a| of a few units the product -1.4427f a alone moves the fp32 sigmoid past K_ULP ulps: the old model rejects the restatement
    somewhere on [-30, -5], the new one holds it"""
    a = torch.linspace(-30, -5, 20001)
    got = torch.from_numpy(_silu_np(a.numpy()))
    assert R.ratio(got, *R._silu(R.exact(a))).max().item() > 1.0
    R.assert_within(got, U.silu32(R.exact(a)), what="silu32 on [-30, -5]")


@pytest.mark.parametrize("shape", [(7, 33, 33), (64, 5, 32), (5, 252, 252), (6, 512, 520), (3, 1024, 1024)])
def test_gemv_restatement_within_the_bound_not_vacuous_and_defects_rejected(shape):
    rows, K, ldk = shape
    g_ = torch.Generator().manual_seed(K)
    x, W, b = torch.randn(K, generator=g_), torch.randn(rows * ldk, generator=g_), torch.randn(rows, generator=g_)
    worst = 0.0
    for scale in (1.0, 30.0 / math.sqrt(K)):
        for act in (U.ACT_NONE, U.ACT_SILU, U.ACT_RELU):
            for bias in (b, None):
                ref = U.gemv(x, W * scale, bias, rows, K, ldk, act)
                worst = max(worst, R.assert_within(torch.from_numpy(_gemv_np(x, W * scale, bias, rows, K, ldk, act)), ref, what=f"gemv {shape} act {act}"))
    print(f"gemv restatement {shape}: worst err/bound {worst:.3g}")
    assert worst > 1e-3
    ref = U.gemv(x, W, b, rows, K, ldk, U.ACT_NONE)
    R.assert_rejects(torch.from_numpy(_gemv_np(x, W, b, rows, K, ldk, U.ACT_NONE, drop=lambda lane, k: lane == 1)), ref, what="lane 1 missing")
    good = torch.from_numpy(_gemv_np(x, W, b, rows, K, ldk, U.ACT_NONE)).double()
    R.assert_rejects(good - U.gemv_partial(x, W, rows, K, ldk, U.gemv_lane_mask(K, ldk, 1)), ref, what="lane 1 missing (fp64 term)")
    if K % 4:
        R.assert_rejects(torch.from_numpy(_gemv_np(x, W, b, rows, K, ldk, U.ACT_NONE, drop=lambda lane, k: k >= K - K % 4)), ref, what="K mod 4 tail missing")


# ------------------------------------------------------------------------------------------------------------ planted defects

@pytest.mark.parametrize("step", [2, 1000])
def test_planted_update_defects_are_rejected_on_the_restatement(step):
    n = 6000
    p, g, m, v, ema = _state(n, 40 + step, step)
    ref = U.adamw_step(p, g, m, v, ema, HYPER, step, 1.0, None, torch.bfloat16)
    for defect, where in ((("bc", 1), 0), (("bc", -1), 0), ("eps_inside", 0), ("coupled_wd", 0), ("ema_old_p", 3)):
        bad = adamw_np(p, g, m, v, ema, HYPER, step, 1.0, None, defect)
        R.assert_rejects(torch.from_numpy(bad[where]), ref[where], what=f"{defect} at step {step}")
    st = [1024.0, 0.0, 0.0, float(step - 1)]
    ref_s = U.adamw_step(p, g * 1024, m, v, ema, HYPER, 1, 1.0, st)
    R.assert_rejects(torch.from_numpy(adamw_np(p, g * 1024, m, v, ema, HYPER, 1, 1.0, st, "no_unscale")[2]), ref_s[2], what="unscale left out")
    R.assert_within(torch.from_numpy(adamw_np(p, g * 1024, m, v, ema, HYPER, 1, 1.0, st)[0]), ref_s[0], what="bias correction follows state[3]")
    good = adamw_np(p, g, m, v, ema, HYPER, step, 1.0)
    half = good[0].copy()
    half[n // 2:] = p.numpy()[n // 2:]
    R.assert_rejects(torch.from_numpy(half), ref[0], what="second half left untouched")
    for T in (torch.bfloat16, torch.float16):
        sref = U.adamw_step(p, g, m, v, ema, HYPER, step, 1.0, None, T)[4]
        R.assert_within(torch.from_numpy(good[0]).to(T), sref, what=f"shadow {T}")
        R.assert_rejects(U.truncate(torch.from_numpy(good[0]), T), sref, what=f"shadow {T} truncated")


def test_another_summation_order_is_rejected_at_fp32():
    B, H, W, C = 2, 3, 5, 8
    g_ = torch.Generator().manual_seed(9)
    g = torch.randn(B, 2 * H, 2 * W, C, generator=g_)
    g[:, 0::2, 0::2] = 1e8 * (1 + torch.rand(B, H, W, C, generator=g_))  # g00 large, g01 = -g00 + small: the order decides what survives
    g[:, 0::2, 1::2] = -g[:, 0::2, 0::2]
    for T in (torch.float32, torch.bfloat16, torch.float16):
        gt = (g if T == torch.float32 else torch.randn(B, 2 * H, 2 * W, C, generator=g_)).to(T)
        ref = U.sumpool2(gt, B, H, W, C, T)
        R.assert_within(U.sumpool2_fp32_chain(gt, B, H, W, C, (0, 1, 2, 3)).to(T), ref, what=f"sumpool2 {T}")
    ref = U.sumpool2(g, B, H, W, C, torch.float32)
    R.assert_rejects(U.sumpool2_fp32_chain(g, B, H, W, C, (0, 2, 3, 1)), ref, what="sumpool2 in the order (g00 + g10) + g11) + g01")
    up = U.upsample2(g, B, 2 * H, 2 * W, C).view(B, 4 * H, 4 * W, C)
    assert torch.equal(up[:, 1::2, 0::2], g) and torch.equal(up[:, 0::2, 1::2], g)


# ------------------------------------------------------------------------------------------------------- the second definition

def test_torch_adamw_is_a_second_definition_of_one_minus_beta():
    """torch.optim.AdamW forms 1 - beta2 in Python double and rounds the result; the kernel (and the reference) form it from the fp32
    beta2.  fl32(beta) = beta (1 + d), |d| <= u32, so the fp32 form is (1 - beta) - beta d: the two constants differ by at most
    u32 beta / (1 - beta) relative to 1 - beta.  After one step from v = 0 the second moment IS that constant times g^2."""
    n = 4000
    g_ = torch.Generator().manual_seed(1)
    p, g = torch.randn(n, generator=g_), torch.randn(n, generator=g_) + 3.0
    q = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([q], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3)
    q.grad = g.clone()
    opt.step()
    ref = U.adamw_step(p, g, torch.zeros(n), torch.zeros(n), None, HYPER, 1, 1.0)
    rel = (opt.state[q]["exp_avg_sq"].double() - ref[2].v) / ref[2].v
    allowed = U32 * 0.999 / (1 - 0.999)
    const_kernel, const_torch = float(f4(1) - f4(0.999)), float(f4(1 - 0.999))
    dp = (q.detach().double() - ref[0].v).abs().max().item()
    print(f"1 - beta2: kernel {const_kernel:.7e}, torch {const_torch:.7e}, relative distance {(const_torch - const_kernel) / const_kernel:.3e} "
          f"(allowed u32 beta/(1-beta) = {allowed:.3e}); v after one step: torch - reference in [{rel.min().item():.3e}, {rel.max().item():.3e}]; "
          f"max |p_torch - p_ref| {dp:.3e}")
    assert abs(rel).max().item() <= allowed + 3 * U32  # + the roundings of g * g, the product and the fp32 store
    assert rel.min().item() > 0 and abs((const_torch - const_kernel) / const_kernel - 1.29e-5) < 0.01e-5
    assert dp < 1e-6  # the update itself: both constants cancel against their own bias correction at step 1


def test_torch_ema_is_a_second_definition_of_one_minus_rate():
    """ema.py: ema.mul_(rate).add_(p, alpha=1 - rate) with 1 - rate in double; the same derivation with beta = rate: within
    u32 rate / (1 - rate) = 5.96e-4 at 0.9999.  torch's constant is the SMALLER one: rate + (1 - rate) sums to 0.999834 of a constant
    parameter in torch and to 1 in the kernel."""
    n = 4000
    p = torch.randn(n, generator=torch.Generator().manual_seed(2)) + 3.0
    ema = torch.zeros(n)
    ema.mul_(0.9999).add_(p, alpha=1 - 0.9999)
    ref = U.ema_step(torch.zeros(n), p, 0.9999)
    rel = (ema.double() - ref.v) / ref.v
    allowed = U32 * 0.9999 / (1 - 0.9999)
    ck, ct = float(f4(1) - f4(0.9999)), float(f4(1 - 0.9999))
    fix_torch = float(f4(1 - 0.9999)) / (1 - float(f4(0.9999)))
    print(f"1 - rate: kernel {ck:.7e}, torch {ct:.7e}, relative distance {(ct - ck) / ck:.3e} (allowed {allowed:.3e}); ema after one step from 0: "
          f"torch - reference in [{rel.min().item():.3e}, {rel.max().item():.3e}]; torch's fixed point {fix_torch:.6f} of a constant parameter")
    assert abs(rel).max().item() <= allowed + 2 * U32
    assert rel.max().item() < 0 and abs((ct - ck) / ck + 1.66e-4) < 0.01e-4
    assert abs(fix_torch - 0.999834) < 1e-6
    assert abs(ck - 1.0001659e-4) < 1e-11 and abs(float(f4(1) - f4(0.999)) - 9.999871e-4) < 1e-10


def test_a_rewrite_that_switched_to_the_double_constants_is_rejected():
    """the bound is two or three fp32 roundings wide: the second definition lies outside it for every one of the three constants"""
    p, g, m, v, ema = _state(6000, 77, 1000)
    ref = U.adamw_step(p, g, m, v, ema, HYPER, 1000, 1.0)
    bad = adamw_np(p, g, m, v, ema, HYPER, 1000, 1.0, None, "double_consts")
    w = [R.assert_rejects(torch.from_numpy(bad[i]), ref[i], what=f"double constants, {name}") for i, name in ((1, "m"), (2, "v"), (3, "ema"))]
    print(f"the double-formed constants over the bound: m (beta1 0.9) {w[0]:.3g}, v (beta2 0.999) {w[1]:.3g}, ema (rate 0.9999) {w[2]:.3g}")


# ------------------------------------------------------------------------------------------------------------------ schedule

def test_sigma_conditioning_bands_and_the_bound_that_carries_them():
    t = torch.cat([torch.linspace(0, 1, 100001), torch.tensor([1e-5, 1e-4, 3e-4])])
    for eta in (1e-3, 1e-2):
        mu, sg = U.mu_sigma(t, eta)
        a, s = _mu_sigma_np(t.numpy(), eta)
        w_mu = R.assert_within(torch.from_numpy(a), mu, what=f"mu eta {eta}")
        w_sg = R.assert_within(torch.from_numpy(s), sg, what=f"sigma eta {eta}")
        rel = ((torch.from_numpy(s).double() - sg.v) / sg.v).abs()
        bands = U.sigma_bands(t, rel)
        print(f"eta {eta}: restatement err/bound mu {w_mu:.3g} sigma {w_sg:.3g}; sigma relative error t<1e-3 {bands[0]:.3e}, t<1e-2 {bands[1]:.3e}, "
              f"t>=0.1 {bands[2]:.3e}; relative bound at t=0 {(sg.e[0] / sg.v[0]).item():.3g}, at t=1 {(sg.e[100000] / sg.v[100000]).item():.3g}")
        if eta == 1e-3:
            for got, want in zip(bands, U.SIGMA_BANDS_CPU):
                assert 0.95 * want <= got <= want, (bands, U.SIGMA_BANDS_CPU)
            assert (sg.e[0] / sg.v[0]).item() > 100 * (sg.e[100000] / sg.v[100000]).item()  # wide where the definition is ill-conditioned
            assert ((mu.v - torch.from_numpy(a).double()).abs()[t > 0.9]).max().item() < 1e-5


# ---------------------------------------------------------------------------------------------------------------------- cast

@pytest.mark.parametrize("T", [torch.bfloat16, torch.float16])
def test_numpy_cast_reference_equals_torch_on_the_edge_tensor(T):
    src = torch.cat([U.cast_edge_values(), torch.randn(20000, generator=torch.Generator().manual_seed(4)) * 100,
                     torch.randn(20000, generator=torch.Generator().manual_seed(5)) * 1e-6])
    got, want = U.cast(src, T), src.to(T)
    nan = torch.isnan(src)
    assert torch.equal(torch.isnan(got), nan) and torch.equal(torch.isnan(want), nan) and nan.sum() == 1
    assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])
    if T == torch.float16:
        f = lambda x: U.cast(torch.tensor([x]), T).float().item()
        assert f(65519.996) == 65504.0 and math.isinf(f(65520.0)) and f(2.0 ** -25) == 0.0 and f(3 * 2.0 ** -25) == 2.0 ** -23
        assert f(float(np.nextafter(f4(2.0 ** -25), f4(1)))) == 2.0 ** -24 and f(-1e-40) == 0.0 and math.copysign(1, f(-1e-40)) == -1
