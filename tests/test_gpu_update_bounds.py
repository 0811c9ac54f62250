"""The kernels that consume the gradients (fused AdamW + EMA + shadow, EMA, dynamic loss scale), the ones that condition the network on time
(timestep embedding, noise schedule, the one-row Linear), the sampler's predictor / corrector and the remaining pointwise kernels, each
against its float64 definition with a derived element-wise bound (tests/fp64_update_ref.py), at the smallest sizes that reach the edge:

  * every grid-stride loop runs past its first pass.  The grid caps are read from the launchers: grid_for's default 8192 blocks
    (pointwise.hip:860, sampler.hip:13) -- U.PASS = 8192 * 256 elements for adamw_ema / ema / cast_f32 / predict / correct, the same number
    of 16-byte vectors for silu and sumpool2; 4096 blocks of float4 for scaler_check (U.CHECK_PASS, pointwise.hip:1325); 16384 blocks
    for upsample2 (U.UPSAMPLE_PASS, pointwise.hip:1008).  N = one pass plus a ragged remainder of 4099.  The first pass and the rest
    are checked and reported separately, so that a stride defect names itself.
  * the update is held in its own ulps: a third of the parameters are exactly 0 (p' is minus the update), gradients are log-uniform over
    1e-12 .. 1e4 with exact zeros, the moments are seeded for steps 1000 and 100 000, and every call is compared against the reference
    fed with the kernel's actual state before that call (bounds do not compound).
  * every planted defect is rejected on the kernel's own output.

Measured on an MI355X (profiles/update_bounds.md lists every report() line of this file): the file runs in 5.1 s, its slowest test in
1.2 s; every bound held without a kernel change -- worst err/bound 0.999 for the update (the 16-bit shadow; p itself 0.59), 0.45 for the
embedding, 0.42 for the schedule, 0.29 for gemv_f32, 0.998 for the sampler, 0.998 for SiLU, 0.999 for sumpool2.  Every planted defect is
rejected at every step it is planted at (steps 2 and 1000); the smallest margin is the truncated shadow, 1.98 times its bound (truncation
is at most twice round-to-nearest), the next one the bias corrections one step off at step 1000, 4.9e2.  By their own arithmetic the
bias-correction and eps-placement defects vanish once bc1 and bc2_sqrt round to 1 in fp32 (step 100 000), which is why they are planted
at 2 and 1000."""
import math

import pytest
import torch

import fp64_ref as R
import fp64_update_ref as U
from climate2weather_amd import ops
from climate2weather_amd.pipelines import SDAPipeline

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, F16 = ops.DTYPE_F32, ops.DTYPE_BF16, ops.DTYPE_F16
TD = ops.TORCH_DTYPE
PASS = U.PASS
N = PASS + 4099  # one pass of an 8192-block grid-stride loop plus a ragged remainder
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-3, ema_rate=0.9999)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(n, seed, scale=1.0):
    return torch.randn(n, generator=_gen(seed), device=DEV) * scale


def _params(n, seed):
    """a third exactly 0, a third about 0.05, a third about 30"""
    p = (_randn(n, seed) * torch.tensor([0.0, 0.05, 30.0], device=DEV).repeat(-(-n // 3))[:n]).contiguous()
    p[0::3] = 0.0  # +0: a product with a negative random number would leave -0
    return p


def _grads(n, seed):
    """log-uniform magnitude 1e-12 .. 1e4, random sign, some exact zeros"""
    g_ = _gen(seed)
    g = torch.randn(n, generator=g_, device=DEV).sign() * 10 ** (torch.rand(n, generator=g_, device=DEV) * 16 - 12)
    g[::17] = 0
    return g.float().contiguous()


def _moments(n, seed):
    """seeded non-zero moments of a run in progress: m of either sign, v = g_prev^2-like, non-negative"""
    gp = _grads(n, seed)
    k = torch.rand(n, generator=_gen(seed + 1), device=DEV)
    return (gp * (0.6 * k - 0.1)).contiguous(), (gp * gp * (0.2 + k)).contiguous()


def _passes(got, ref, what, first=PASS, report=True):
    """assert_within on the first pass of the grid-stride loop and on the rest, reported separately: (worst of [0, pass), of [pass, n))"""
    g, rv, re = got.reshape(-1), ref.v.reshape(-1), ref.e.reshape(-1)
    a = R.assert_within(g[:first], rv[:first], re[:first], what=f"{what} [0, pass)")
    b = R.assert_within(g[first:], rv[first:], re[first:], what=f"{what} [pass, n)")
    if report:
        R.report(f"{what} [0, pass)", a)
        R.report(f"{what} [pass, n)", b)
    return a, b


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16), b.view(torch.int32 if b.dtype == torch.float32 else torch.int16))


class _Run:
    """one parameter buffer with its moments, EMA and shadow; step() calls the kernel and returns the reference of that call, computed
    from the state the kernel found"""

    def __init__(self, seed, shadow, ema_on, n=N):
        self.n = n
        self.p = _params(n, seed)
        self.m, self.v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        self.ema = (self.p + _randn(n, seed + 7, 0.01)) if ema_on else None
        self.sh = torch.full((n,), 3.0, dtype=shadow, device=DEV) if shadow is not None else None

    def seed_moments(self, seed):
        self.m, self.v = _moments(self.n, seed)

    def snapshot(self):
        return [None if x is None else x.clone() for x in (self.p, self.m, self.v, self.ema, self.sh)]

    def step(self, g, hyper, step, gs, scaler=None, host_step=None, variant=None):
        self.before = self.snapshot()
        st = None if scaler is None else scaler.tolist()
        ops.adamw_ema(self.p, g, self.m, self.v, self.ema, self.sh, self.n, hyper["lr"], hyper["beta1"], hyper["beta2"], hyper["eps"], hyper["wd"],
                      host_step if host_step is not None else step, hyper["ema_rate"], gs, scaler=scaler)
        return self.reference(g, hyper, step, gs, st, variant)

    def reference(self, g, hyper, step, gs, st=None, variant=None, shadow_dtype="own"):
        b = self.before
        sdt = (None if self.sh is None else self.sh.dtype) if shadow_dtype == "own" else shadow_dtype
        return U.adamw_step(b[0], g, b[1], b[2], b[3], hyper, step, gs, st, sdt, shadow_prev=b[4], variant=variant)

    def got(self):
        return (self.p, self.m, self.v, self.ema, self.sh)

    def check(self, ref, what):
        """every tensor of the call inside its bound, pass by pass; one report line per pass, naming each tensor's worst ratio"""
        w = {name: _passes(got, r, f"{what} {name}", report=False) for name, got, r in zip(("p", "m", "v", "ema", "shadow"), self.got(), ref)
             if got is not None}
        for i, span in enumerate(("[0, pass)", "[pass, n)")):
            R.report(f"{what} {span} (" + ", ".join(f"{k} {v[i]:.3f}" for k, v in w.items()) + ")", max(v[i] for v in w.values()))


# --------------------------------------------------------------------------------------------------------------------- AdamW

@pytest.mark.parametrize("ema_on", [True, False], ids=["ema", "noema"])
@pytest.mark.parametrize("shadow", [None, torch.bfloat16, torch.float16], ids=["noshadow", "bf16", "fp16"])
def test_adamw_update_within_its_own_ulps(shadow, ema_on):
    tag = f"adamw[{str(shadow).replace('torch.', '') if shadow is not None else 'no shadow'}, {'ema' if ema_on else 'no ema'}]"
    for wd, gs in ((1e-3, 1.0), (1e-3, 0.5), (0.0, 1.0), (0.0, 0.5)):
        h = dict(HYPER, wd=wd)
        run = _Run(11, shadow, ema_on)
        for step in (1, 2, 3):  # m = v = 0 at step 1, then the previous call's
            ref = run.step(_grads(N, 20 + step), h, step, gs)
            run.check(ref, f"{tag} step {step} wd {wd} grad_scale {gs}")
        for step in (1000, 100000):
            run.seed_moments(step)
            ref = run.step(_grads(N, 30 + step % 97), h, step, gs)
            run.check(ref, f"{tag} step {step} wd {wd} grad_scale {gs}")
        assert torch.isfinite(run.p).all()
        if shadow is not None:  # the refresh is the conversion of the parameter just written, bit for bit
            assert _bits_equal(run.sh, U.cast(run.p, shadow))


def test_adamw_with_a_zero_learning_rate_leaves_p_bit_unchanged():
    run = _Run(12, torch.bfloat16, True)
    run.seed_moments(5)
    h = dict(HYPER, lr=0.0)
    ref = run.step(_grads(N, 6), h, 1000, 1.0)
    assert _bits_equal(run.p, run.before[0])
    assert not torch.equal(run.m, run.before[1]) and not torch.equal(run.v, run.before[2])
    run.check(ref, "adamw lr 0")


@pytest.mark.parametrize("taken", [0, 999])
@pytest.mark.parametrize("scale", [1.0, 1024.0, 65536.0])
def test_adamw_with_a_scaler_state_unscales_and_counts_the_steps_taken(scale, taken):
    run = _Run(13, torch.float16, True)
    if taken:
        run.seed_moments(8)
    st = torch.tensor([scale, 1.0, 0.0, float(taken)], device=DEV)
    g = _grads(N, 9) * scale
    ref = run.step(g, HYPER, taken + 1, 1.0, scaler=st, host_step=500)  # the host's step is NOT the one the bias corrections use
    run.check(ref, f"adamw scale {scale:g} state[3] {taken}")
    assert st.tolist() == [scale, 1.0, 0.0, float(taken)]
    host = run.reference(g, HYPER, 500, 1.0 / scale)  # the defect: the bias corrections follow the host step
    R.assert_rejects(run.p, host[0], what="bias corrections from the host step")
    if scale != 1.0:
        bad = run.reference(g, HYPER, taken + 1, 1.0, st.tolist(), "no_unscale")
        R.report(f"planted: unscale left out, scale {scale:g}", R.assert_rejects(run.v, bad[2], what="the unscale left out"))


@pytest.mark.parametrize("shadow", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_adamw_skipped_step_moves_only_the_ema(shadow):
    run = _Run(14, shadow, True)
    run.seed_moments(3)
    st = torch.tensor([1024.0, 2.0, 1.0, 41.0], device=DEV)  # found-inf set
    g = _grads(N, 4) * 1024
    g[PASS + 5] = float("inf")
    ref = run.step(g, HYPER, 42, 1.0, scaler=st)
    for name, got, was, r in zip(("p", "m", "v"), run.got(), run.before, ref):
        assert (r.e == 0).all() and _bits_equal(got, was), name
    assert _bits_equal(run.sh, run.before[4]) and (ref[4].e == 0).all()
    _passes(run.ema, ref[3], f"skipped step ema (shadow {shadow})")
    assert not torch.equal(run.ema, run.before[3])


@pytest.mark.parametrize("step", [2, 1000])
def test_adamw_planted_defects_are_rejected_on_the_kernels_output(step):
    run = _Run(15, torch.bfloat16, True)
    if step > 1:
        run.seed_moments(step)
    g = _grads(N, 16)
    ref = run.step(g, HYPER, step, 1.0)
    run.check(ref, f"adamw step {step} before the defects")
    for variant, idx in ((("bc", 1), 0), (("bc", -1), 0), ("eps_inside", 0), ("coupled_wd", 0), ("ema_old_p", 3)):
        bad = run.reference(g, HYPER, step, 1.0, variant=variant)
        R.report(f"planted {variant} at step {step}", R.assert_rejects(run.got()[idx], bad[idx], what=f"{variant} at step {step}"))
    for name, got, was, r in zip(("p", "m", "v", "ema"), run.got(), run.before, ref):
        half = got.clone()
        half[PASS:] = was[PASS:]
        R.report(f"planted: second pass of {name} untouched, step {step}", R.assert_rejects(half, r, what=f"second pass of {name} left untouched"))
        assert R.ratio(half[:PASS], r.v[:PASS], r.e[:PASS]).max().item() <= 1.0  # ... and the first pass does not show it
    for T in (torch.bfloat16, torch.float16):
        sref = run.reference(g, HYPER, step, 1.0, shadow_dtype=T)[4]
        R.assert_within(U.cast(run.p, T), sref, what=f"shadow {T} rounded to nearest")
        R.report(f"planted: shadow {T} truncated, step {step}", R.assert_rejects(U.truncate(run.p, T), sref, what=f"shadow {T} rounded by truncation"))


# ----------------------------------------------------------------------------------------------------------------------- EMA

@pytest.mark.parametrize("rate", [0.9999, 0.999, 0.0, 1.0])
def test_ema_update(rate):
    ema, p = _randn(N, 1) + 0.5, _params(N, 2)
    before = ema.clone()
    ops.ema_update(ema, p, N, rate)
    ref = U.ema_step(before, p, rate)
    _passes(ema, ref, f"ema_update rate {rate}")
    if rate == 1.0:
        assert _bits_equal(ema, before)
    if rate == 0.0:
        assert _bits_equal(ema, p)
    half = ema.clone()
    half[PASS:] = before[PASS:]
    if rate != 1.0:
        R.assert_rejects(half, ref, what="second pass left untouched")


# --------------------------------------------------------------------------------------------------------------- loss scale

_check_buf = {}


def _check_grads():
    """finite values only: randn, the largest finite float and denormals among them"""
    if "g" not in _check_buf:
        g = _randn(U.CHECK_PASS + 8, 3)
        fmax = torch.finfo(torch.float32).max
        g[1::1000] = fmax
        g[2::1000] = -fmax
        g[3::1000] = 1e-40
        g[4::1000] = -1.4e-45
        g[U.CHECK_PASS - 2: U.CHECK_PASS + 8] = torch.tensor([fmax, 1e-40, -fmax, -1e-45, fmax, 1e-39, 2e-45, -fmax, 1e-41, fmax], device=DEV)
        _check_buf["g"] = g
    return _check_buf["g"]


@pytest.mark.parametrize("n", [U.CHECK_PASS + 4 + r for r in range(4)] + [1, 3, 4, 5, 4099])
def test_grad_scaler_check_sees_one_non_finite_value_anywhere(n):
    g = _check_grads()
    init = [1024.0, 5.0, 0.0, 7.0]
    st = torch.tensor(init, device=DEV)
    ops.grad_scaler_check(g, n, st)
    assert st.tolist() == init, "finite gradients (largest finite float, denormals) tripped the check, or another field was written"
    positions = sorted({0, n - 1} | ({U.CHECK_PASS, U.CHECK_PASS - 1} if n > U.CHECK_PASS else set()))
    for pos in positions:
        for bad in (float("inf"), float("-inf"), float("nan")):
            keep = g[pos].clone()
            g[pos] = bad
            st.copy_(torch.tensor(init, device=DEV))
            ops.grad_scaler_check(g, n, st)
            got = st.tolist()
            g[pos] = keep
            assert got == [1024.0, 5.0, 1.0, 7.0], (n, pos, bad, got)
    if n < 4099:  # a non-finite value just past n is not the call's business
        keep = g[n].clone()
        g[n] = float("nan")
        st.copy_(torch.tensor(init, device=DEV))
        ops.grad_scaler_check(g, n, st)
        g[n] = keep
        assert st.tolist() == init


def test_grad_scaler_update_follows_the_model_exactly_for_200_steps():
    flags = (torch.rand(200, generator=torch.Generator().manual_seed(6)) < 0.3).tolist()
    fl = torch.tensor([1.0 if f else 0.0 for f in flags], device=DEV)
    st = torch.zeros(4, device=DEV)
    rec = torch.zeros((200, 4), device=DEV)
    ops.grad_scaler_init(st, 65536.0)
    for i in range(200):
        st[2:3].copy_(fl[i:i + 1])
        ops.grad_scaler_update(st, 2.0, 0.5, 3)
        rec[i].copy_(st)
    got = rec.tolist()  # one readback
    want = U.scaler_model(flags, 65536.0, 2.0, 0.5, 3)
    for i in range(200):
        assert got[i] == want[i], (i, got[i], want[i])
    assert any(flags) and not all(flags) and len({w[0] for w in want}) > 4


# --------------------------------------------------------------------------------------------------------- time conditioning

def _embedding_t():
    return torch.cat([torch.tensor([0.0, 1.0, 2.0 ** -126, 1e-4]), torch.linspace(0, 1, 296)]).to(DEV)


@pytest.mark.parametrize("max_period", [10.0, 10000.0])
@pytest.mark.parametrize("dim", [32, 64, 33])
def test_timestep_embedding(dim, max_period):
    t = _embedding_t()
    n = t.numel()
    out = torch.full((n * dim + 3,), 7.0, device=DEV)
    ops.timestep_embedding(t, out, n, dim, max_period)
    assert (out[n * dim:] == 7.0).all()
    ref = U.timestep_embedding(t, dim, max_period)
    R.report(f"timestep_embedding dim {dim} max_period {max_period:g}", R.assert_within(out[: n * dim].view(n, dim), ref, what="timestep_embedding"))
    if dim % 2:
        assert (out[: n * dim].view(n, dim)[:, -1] == 0).all()
    half = dim // 2
    swapped = out[: n * dim].view(n, dim).clone()
    swapped[:, :half], swapped[:, half:2 * half] = out[: n * dim].view(n, dim)[:, half:2 * half], out[: n * dim].view(n, dim)[:, :half]
    R.assert_rejects(swapped, ref, what="cos and sin halves swapped")
    other = U.timestep_embedding(t, dim, max_period * (1 + 1e-4))
    R.assert_rejects(out[: n * dim].view(n, dim), other, what="max_period off by 1e-4")


@pytest.mark.parametrize("eta", [1e-3, 1e-2])
def test_mu_sigma_schedule_and_its_conditioning_near_zero(eta):
    t = torch.cat([torch.linspace(0, 1, 100001), torch.tensor([1e-5, 1e-4, 3e-4])]).to(DEV)
    n = t.numel()
    out = torch.full((2 * n + 3,), 7.0, device=DEV)
    ops.mu_sigma(t, out, n, eta)
    assert (out[2 * n:] == 7.0).all()
    ms = out[: 2 * n].view(n, 2)
    mu, sg = U.mu_sigma(t, eta)
    R.report(f"mu_sigma eta {eta:g} mu", R.assert_within(ms[:, 0], mu, what="mu"))
    R.report(f"mu_sigma eta {eta:g} sigma", R.assert_within(ms[:, 1], sg, what="sigma"))
    rel = ((ms[:, 1].double() - sg.v) / sg.v).abs()
    bands = U.sigma_bands(t, rel)
    print(f"sigma(t) eta {eta:g}: worst relative error t < 1e-3 {bands[0]:.3e}, 1e-3 <= t < 1e-2 {bands[1]:.3e}, t >= 0.1 {bands[2]:.3e}; "
          f"mu near t = 1: {(ms[:, 0].double() - mu.v).abs()[t > 0.9].max().item():.3e}")
    if eta == 1e-3:
        # The CPU figures have cosf rounded correctly (at most u32 |c|); the kernel's cosf may be K_ULP u32 |c| off.  The radicand's error
        # is 2 |a| e_a with e_a = 2 |c| e_c + one rounding, so no band can exceed K_ULP times its CPU figure with a cosf inside K_ULP ulps.
        for got, cpu in zip(bands, U.SIGMA_BANDS_CPU):
            assert got <= R.K_ULP * cpu, (bands, U.SIGMA_BANDS_CPU)
    assert torch.isfinite(ms).all() and (ms[:, 1] > 0).all()
    R.assert_rejects(ms[:, 1], U.mu_sigma(t, eta * (1 + 1e-3))[1], what="eta off by 1e-3")


@pytest.mark.parametrize("shape", [(7, 33, 33), (64, 5, 32), (5, 252, 252), (513, 512, 520), (8448, 512, 512), (3, 1024, 1024)])
def test_gemv_f32(shape):
    rows, K, ldk = shape
    x = _randn(K, K)
    W0 = _randn(rows * ldk, K + 1)
    b = _randn(rows, K + 2)
    worst = {}
    for tag, scale in (("unit variance", 1.0), ("pre-activations over +-30", 10.0 / math.sqrt(K))):
        W = (W0 * scale).contiguous()
        for bias in (b, None):
            for act, an in ((ops.ACT_NONE, "none"), (ops.ACT_SILU, "silu"), (ops.ACT_RELU, "relu")):
                y = torch.full((rows + 3,), 7.0, device=DEV)
                ops.gemv_f32(x, W, bias, y, rows, K, ldk, act)
                assert (y[rows:] == 7.0).all(), "gemv wrote past its rows"
                ref = U.gemv(x, W, bias, rows, K, ldk, act)
                w = R.assert_within(y[:rows], ref, what=f"gemv {shape} {tag} act {an} bias {bias is not None}")
                worst[(tag, an)] = max(worst.get((tag, an), 0.0), w)
                if act == ops.ACT_NONE and bias is not None:
                    lane = U.gemv_partial(x, W, rows, K, ldk, U.gemv_lane_mask(K, ldk, 1, DEV))
                    R.report(f"planted: gemv {shape} {tag} lane 1 missing", R.assert_rejects(y[:rows].double() - lane, ref, what="one lane's partial sum missing"))
                    if K % 4:
                        tail = U.gemv_partial(x, W, rows, K, ldk, torch.arange(K, device=DEV) >= K - K % 4)
                        R.report(f"planted: gemv {shape} {tag} K mod 4 tail missing", R.assert_rejects(y[:rows].double() - tail, ref, what="the K mod 4 tail missing"))
    for (tag, an), w in worst.items():
        R.report(f"gemv_f32 {shape} {tag} act {an}", w)
    if rows >= 513:
        pre = U.gemv(x, (W0 * 10.0 / math.sqrt(K)).contiguous(), None, rows, K, ldk, U.ACT_NONE).v
        assert pre.abs().max().item() > 20.0 and pre.min().item() < -20.0  # the SiLU argument term is exercised on both sides


# ------------------------------------------------------------------------------------------------------------------- sampler

@pytest.mark.parametrize("leg", ["first", "last"])
def test_sampler_predict_and_correct(leg):
    pipe = SDAPipeline(1e-3)
    t, tn = (1.0, 1.0 - 1.0 / 64) if leg == "first" else (1.0 / 64, 0.0)  # the last step: mu near 1, sigma near eta
    mu_t, sg_t = pipe._mu_sigma_f(t)
    mu_n, sg_n = pipe._mu_sigma_f(tn)
    a, b = mu_n / mu_t, sg_n - mu_n * sg_t / mu_t
    tau = 1.0 if leg == "first" else 0.3
    x, eps, z = _randn(N, 1, 1.0 if leg == "last" else 1e-2), _randn(N, 2), _randn(N, 3)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    x0 = x.clone()
    ops.sampler_predict(x, eps, flag, N, a, b)
    ref = U.predict(x0, eps, a, b)
    _passes(x, ref, f"sampler_predict {leg} step (a {a:.4g}, b {b:.4g})")
    half = x.clone()
    half[PASS:] = x0[PASS:]
    R.assert_rejects(half, ref, what="predict: second pass left untouched")
    ss = torch.zeros(1, device=DEV)
    ops.sumsq(eps, ss, N)
    ss_ref = R.sumsq(eps, N)
    R.report(f"sumsq feeding the corrector ({leg})", R.assert_within(ss, ss_ref, what="sumsq"))
    x1 = x.clone()
    ops.sampler_correct(x, eps, z, ss, flag, N, tau, sg_n)
    ref_c = U.correct(x1, eps, z, ss_ref, N, tau, sg_n)
    _passes(x, ref_c, f"sampler_correct {leg} step (tau {tau}, sigma' {sg_n:.4g}), delta from the bounded sumsq")
    _passes(x, U.correct(x1, eps, z, ss, N, tau, sg_n), f"sampler_correct {leg} step, delta from the kernel's own sumsq")
    assert flag.item() == 0
    R.assert_rejects(x, U.correct(x1, eps, z, ss, N, tau * (1 + 1e-3), sg_n), what="tau off by 1e-3")
    R.assert_rejects(x, U.correct(x1, eps, z, ss, N + 1000, tau, sg_n), what="the mean of eps^2 over another n")
    half = x.clone()
    half[PASS:] = x1[PASS:]
    R.assert_rejects(half, ref_c, what="correct: second pass left untouched")
    x[PASS + 17] = float("inf")  # a data value in the second pass: the flag must see it
    ops.sampler_predict(x, eps, flag, N, a, b)
    assert flag.item() == 1
    flag.zero_()
    x.copy_(x1)
    x[N - 1] = float("inf")
    ops.sampler_correct(x, eps, z, ss, flag, N, tau, sg_n)
    assert flag.item() == 1


# ----------------------------------------------------------------------------------------------------------------- pointwise

def _silu_inputs(dt):
    P = 4 if dt == F32 else 8
    n = (2 * PASS + 1) * P  # two passes of 16-byte vectors plus one
    x = _randn(n, 40 + dt, 3.0)
    edges = [0.0, 1e-30, 20.0, 40.0, 88.0, 100.0] + ([65504.0] if dt == F16 else [])
    e = torch.tensor(edges + [-v for v in edges], device=DEV)
    x[-e.numel():] = e  # the last vectors: the one past the second pass among them
    x[: e.numel()] = e
    return x.to(TD[dt]).contiguous(), n, P


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
def test_silu_and_its_backward(dt):
    x, n, P = _silu_inputs(dt)
    y = torch.full((n + P,), 7.0, dtype=TD[dt], device=DEV)
    ops.silu(x, y, n, dt)
    assert (y[n:] == 7.0).all() and not torch.isnan(y).any()
    _passes(y[:n], U.silu(x, TD[dt]), f"silu dtype {dt}", first=PASS * P)
    dy = _randn(n, 50 + dt).to(TD[dt])
    dx = torch.full((n + P,), 7.0, dtype=TD[dt], device=DEV)
    ops.silu_backward(x, dy, dx, n, dt)
    assert (dx[n:] == 7.0).all() and not torch.isnan(dx).any()
    ref = U.silu_backward(x, dy, TD[dt])
    _passes(dx[:n], ref, f"silu_backward dtype {dt}", first=PASS * P)
    half = dx[:n].clone()
    half[PASS * P:] = 0
    R.assert_rejects(half, ref, what="second pass left untouched")


def test_fp32_silu_needs_the_argument_term():
    """on the kernel's own output: how far the fp32 route is from the K_ULP model that the 16-bit epilogues use (reported), inside the
    fp32 model; an argument off by 2^-20 relative is rejected"""
    a = torch.linspace(-30, 30, 400000, device=DEV)
    y = torch.empty_like(a)
    ops.silu(a, y, a.numel(), F32)
    old = R.ratio(y, *R._silu(R.exact(a))).max().item()
    new = R.assert_within(y, U.silu32(R.exact(a)), what="silu fp32 on [-30, 30]")
    R.report("silu fp32 on [-30, 30] against the K_ULP model without the argument term (not asserted)", old)
    R.report("silu fp32 on [-30, 30]", new)
    R.assert_rejects(y, U.silu32(R.exact(a.double() * (1 + 2.0 ** -20))), what="the argument off by 2^-20")


def _pool_shapes(dt):
    P = 4 if dt == F32 else 8
    cv = 8 * -(-(PASS // (4 * 65 * 65) + 1) // 8)  # 128 vectors per pixel: B H W C / P = 2 163 200 vectors, past a pass of 2 097 152
    return [(1, 1, 1, 8), (3, 5, 7, 64), (4, 65, 65, cv * P)]


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
def test_sumpool2_adds_in_the_fixed_order(dt):
    for B, H, W, C in _pool_shapes(dt):
        g = _randn(B * 4 * H * W * C, 60 + C).to(TD[dt])
        dx = torch.full((B * H * W * C + 8,), 7.0, dtype=TD[dt], device=DEV)
        ops.sumpool2(g, dx, B, H, W, C, dt)
        assert (dx[B * H * W * C:] == 7.0).all()
        ref = U.sumpool2(g, B, H, W, C, TD[dt])
        P = 4 if dt == F32 else 8
        if B * H * W * C // P > PASS:
            _passes(dx[: B * H * W * C], ref, f"sumpool2 {(B, H, W, C)} dtype {dt}", first=PASS * P)
        else:
            R.report(f"sumpool2 {(B, H, W, C)} dtype {dt}", R.assert_within(dx[: B * H * W * C], ref, what="sumpool2"))
        if dt == F32:  # unrounded fp32: the chain itself must come out bit for bit
            assert _bits_equal(dx[: B * H * W * C].view(-1, C), U.sumpool2_fp32_chain(g, B, H, W, C, (0, 1, 2, 3)).to(DEV))
    if dt == F32:  # values built so that the order matters: g00 + g01 cancel exactly, so the fixed order keeps g10 + g11 in full
        B, H, W, C = 3, 5, 7, 64
        q = _randn(B * 4 * H * W * C, 61).view(B, H, 2, W, 2, C)
        q[:, :, 0, :, 0] = 1e8 * (1 + torch.rand(B, H, W, C, generator=_gen(62), device=DEV))
        q[:, :, 0, :, 1] = -q[:, :, 0, :, 0]
        g = q.reshape(-1).contiguous()
        dx = torch.empty(B * H * W * C, device=DEV)
        ops.sumpool2(g, dx, B, H, W, C, dt)
        ref = U.sumpool2(g, B, H, W, C, torch.float32)
        R.report("sumpool2 fp32 on cancelling values", R.assert_within(dx, ref, what="sumpool2 on cancelling values"))
        R.report("planted: sumpool2 in the order ((g00 + g10) + g11) + g01",
                 R.assert_rejects(U.sumpool2_fp32_chain(g, B, H, W, C, (0, 2, 3, 1)).to(DEV), ref, what="another summation order"))


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
def test_upsample2_is_exact(dt):
    P = 4 if dt == F32 else 8
    cv = 8 * -(-(U.UPSAMPLE_PASS // (5 * 4 * 33 * 31) + 1) // 8)  # 208 vectors per pixel: 4 255 680 output vectors, past 16384 * 256
    for B, H, W, C in [(1, 1, 1, 8), (2, 3, 5, 24), (5, 33, 31, cv * P)]:
        x = _randn(B * H * W * C, 70 + C).to(TD[dt])
        y = torch.full((B * 4 * H * W * C + 8,), 7.0, dtype=TD[dt], device=DEV)
        ops.upsample2(x, y, B, H, W, C, dt)
        assert (y[B * 4 * H * W * C:] == 7.0).all()
        assert _bits_equal(y[: B * 4 * H * W * C].view(-1, C), U.upsample2(x, B, H, W, C).contiguous())
    assert 5 * 4 * 33 * 31 * cv > U.UPSAMPLE_PASS


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
def test_cast_f32_is_bit_exact_past_a_pass(dt):
    edge = U.cast_edge_values().to(DEV)
    src = _randn(N, 80) * 10 ** (torch.rand(N, generator=_gen(81), device=DEV) * 12 - 8)
    for at in (0, PASS - 7, N - edge.numel()):  # the edge tensor in the first pass, across the seam, at the ragged end
        src[at: at + edge.numel()] = edge
    out = torch.full((N + 5,), 7.0, dtype=TD[dt], device=DEV)
    ops.cast_f32(src, out, N, dt)
    assert (out[N:] == 7.0).all()
    nan = torch.isnan(src)
    assert torch.equal(torch.isnan(out[:N]), nan) and nan.sum() == 3
    want = src.clone() if dt == F32 else U.cast(src, TD[dt])
    assert _bits_equal(out[:N][~nan].contiguous(), want[~nan].contiguous())
