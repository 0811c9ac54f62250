"""Held-out validation on the MI355X: the two kernels of csrc/evaluation.hip against float64 with element-wise bounds
(tests/fp64_eval_ref.py), then evaluation.evaluate / Trainer.validate end to end -- against the CPU oracle, against the training step's
own loss, and for what they must leave untouched."""
import hashlib
import os

import numpy as np
import pytest
import torch

import fp64_eval_ref as E
import fp64_ref as R
from climate2weather_amd import _lib, ops
from climate2weather_amd.data import DeviceWindowFeed, SyntheticWindowDataset
from climate2weather_amd.evaluation import evaluate, level_bins, validation_plan
from climate2weather_amd.pipelines import SDAPipeline
from climate2weather_amd.score import ScoreUNet
from climate2weather_amd.training import Trainer
from oracle import diffusion as od
from oracle import unet as ou

pytestmark = pytest.mark.gpu

F32, BF16, F16 = ops.DTYPE_F32, ops.DTYPE_BF16, ops.DTYPE_F16
TD = ops.TORCH_DTYPE
T_CYCLE = [0.0, 1.0, 0.7, 0.9]  # 0.7f / 0.9f: where the fp32 bin rule and a double evaluation of it disagree

# (B, C, ldc, HW).  1-4: the issue's table.  5: 65 tiles per image in slabs of 2 -- 33 slabs, the last one a single tile of 60 pixels (several
# tiles per slab only starts where B * tiles exceeds the 2048-workgroup target).  6: rows too wide for the LDS tile (any-shape kernel, HW % 4 == 0).
CASES = {1: (3, 6, 64, 16 * 16), 2: (2, 65, 128, 8 * 16), 3: (5, 75, 128, 24 * 8), 4: (1, 4, 64, 9 * 7), 5: (33, 6, 64, 4156), 6: (2, 200, 256, 8 * 8)}

# evaluate in 16-bit against the fp32 table of the same weights and draws, scale-relative max|a - b| / max|b| over the table; asserted =
# twice the worst value observed over three seeds on MI355X (the rule the project's other 16-bit bounds were set by)
TABLE_TOL = {BF16: 2.8e-3, F16: 2e-4}  # observed 1.41e-3 / 9.97e-5 (tiny net, 32 x 32, B = 8, seeds 1-3)
# DESIGN section 5, column "loss": how far a 16-bit evaluation of the loss may be from the fp32 one
LOSS_PARITY = {BF16: 3e-4, F16: 3e-5}


def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _knobs_follow_the_environment():
    yield
    ops.knobs_reload()


def _operands(case, dt):
    B, C, ldc, HW = CASES[case]
    g = torch.Generator(device=dev()).manual_seed(100 * case + dt)
    y = torch.randn((B * HW, ldc), generator=g, device=dev()).to(TD[dt])
    y[:, C:] = 1e4  # padding channels must not contribute
    seed = (0x9E3779B97F4A7C15 * (case + 1) + dt) & ((1 << 62) - 1)
    eps = torch.empty((B, C, HW), dtype=torch.float32, device=dev())
    ops.philox_normal(eps, eps.numel(), seed)
    t = torch.tensor([T_CYCLE[b % 4] for b in range(B)], dtype=torch.float32, device=dev())
    return y, eps, seed, t


def _call(y, noise, t, K, case, dt, scratch=None, per=True):
    B, C, ldc, HW = CASES[case]
    table = torch.zeros((K, C), dtype=torch.float64, device=dev())
    count = torch.zeros((K,), dtype=torch.int64, device=dev())
    per_image = torch.full((B,), float("nan"), dtype=torch.float32, device=dev()) if per else None
    if scratch is None:
        scratch = torch.full((ops.sq_err_levels_scratch_bytes(B, C, HW) // 4,), float("nan"), dtype=torch.float32, device=dev())
    ok = ops.sq_err_levels(y, noise, t, table, count, per_image, B, C, HW, ldc, K, scratch, dt)
    return ok, table, count, per_image, scratch


@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("case", sorted(CASES))
def test_level_table_within_float64_bounds(case, dt):
    """table, count and per_image of both noise forms at K = 1, 10, 16 against float64; a second call doubles the table exactly; the
    seed form equals the tensor form on the materialised stream bit for bit, or answers "unsupported" where the header says so."""
    B, C, ldc, HW = CASES[case]
    y, eps, seed, t = _operands(case, dt)
    assert ops.sq_err_levels_scratch_bytes(B, C, HW) == E.scratch_bytes(B, C, HW)
    worst = 0.0
    for K in (1, 10, 16):
        ref = E.sq_err_levels(y, eps, t, B, C, HW, ldc, K)
        ref2 = E.sq_err_levels(y, eps, t, B, C, HW, ldc, K, calls=2)
        got = {}
        for form, noise in (("tensor", eps), ("seed", seed)):
            ok, table, count, per_image, scratch = _call(y, noise, t, K, case, dt)
            torch.cuda.synchronize()
            if form == "seed" and not E.tiled(C, HW, ldc):
                assert ok is False and not table.any() and not count.any()  # unsupported: nothing was launched
                continue
            assert ok is True
            worst = max(worst, R.assert_within(table, ref["table"], what=f"case {case} {form} K={K} table"))
            worst = max(worst, R.assert_within(per_image, ref["per_image"], what=f"case {case} {form} K={K} per_image"))
            assert torch.equal(count, ref["count"].to(count.device))
            first = table.clone()
            assert ops.sq_err_levels(y, noise, t, table, count, None, B, C, HW, ldc, K, scratch, dt)
            torch.cuda.synchronize()
            assert torch.equal(table, 2 * first) and torch.equal(count, ref2["count"].to(count.device))
            R.assert_within(table, ref2["table"], what=f"case {case} {form} K={K} table after two calls")
            got[form] = (first, per_image)
        if len(got) == 2:
            assert torch.equal(got["seed"][0], got["tensor"][0]) and torch.equal(got["seed"][1], got["tensor"][1])
        if K == 10:
            bins = level_bins(t, K)
            assert bins.tolist() == [[0, 9, 7, 9][b % 4] for b in range(B)]
            if B >= 4:
                assert int(ref["count"][9]) >= 2 and int(ref["count"][5]) == 0  # one bin with several images, one empty
    R.report(f"sq_err_levels case {case} dtype {dt}", worst)


@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("case", [1, 3, 5])
def test_level_table_bound_rejects_planted_defects(case, dt):
    B, C, ldc, HW = CASES[case]
    y, eps, seed, t = _operands(case, dt)
    K = 10
    ref = E.sq_err_levels(y, eps, t, B, C, HW, ldc, K)
    ok, table, count, per_image, _ = _call(y, seed, t, K, case, dt)
    torch.cuda.synchronize()
    assert ok
    b = B - 1
    nslab = E.slab_plan(B, HW)[2]
    bin_b = int(level_bins(t, K)[b])
    slab = E.slab_term(y, eps, B, C, HW, ldc, b, nslab - 1)  # the last (possibly short) slab of the last image dropped
    bad = table.clone()
    bad[bin_b] -= slab
    R.assert_rejects(bad, ref["table"], what=f"case {case}: a slab dropped (table)")
    bad_pi = per_image.double().clone()
    bad_pi[b] -= slab.sum()
    R.assert_rejects(bad_pi, ref["per_image"], what=f"case {case}: a slab dropped (per_image)")
    pad = E.padding_term(y, B, C, HW, ldc, b)  # channel C of the rows read as one more channel
    bad = table.clone()
    bad[bin_b, C - 1] += pad
    R.assert_rejects(bad, ref["table"], what=f"case {case}: a padding channel included (table)")
    bad_pi = per_image.double().clone()
    bad_pi[b] += pad
    R.assert_rejects(bad_pi, ref["per_image"], what=f"case {case}: a padding channel included (per_image)")


@pytest.mark.parametrize("case,dt", [(2, BF16), (3, F32), (5, F16), (4, BF16)])
def test_twenty_launches_give_identical_bits(case, dt):
    B, C, ldc, HW = CASES[case]
    y, eps, seed, t = _operands(case, dt)
    noise = seed if E.tiled(C, HW, ldc) else eps
    outs = []
    for _ in range(20):
        ok, table, count, per_image, _ = _call(y, noise, t, 10, case, dt)
        assert ok
        outs.append((table, per_image))
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]) for o in outs[1:])


@pytest.mark.parametrize("form", ["tensor", "seed"])
def test_short_or_missing_scratch_is_a_bad_argument(form):
    case, dt = 1, BF16
    B, C, ldc, HW = CASES[case]
    y, eps, seed, t = _operands(case, dt)
    need = ops.sq_err_levels_scratch_bytes(B, C, HW)
    short = torch.zeros(need // 4 - 1, dtype=torch.float32, device=dev())
    with pytest.raises(_lib.C2wError, match="bad argument"):
        _call(y, seed if form == "seed" else eps, t, 10, case, dt, scratch=short)
    lib = _lib.load()
    table = torch.zeros((10, C), dtype=torch.float64, device=dev())
    count = torch.zeros((10,), dtype=torch.int64, device=dev())
    rc = lib.c2w_sq_err_levels(y.data_ptr(), eps.data_ptr(), t.data_ptr(), table.data_ptr(), count.data_ptr(), None, B, C, HW, ldc, 10, None, 0, dt,
                               None)
    assert rc == -1  # C2W_ERR_BAD_ARG: never a fall-back to atomics
    torch.cuda.synchronize()
    assert not table.any() and not count.any()


# ------------------------------------------------------------------------------------------------------------------ end to end, tiny net

CFG = dict(embedding_dim=64, hidden_channels=[64, 128], hidden_blocks=[1, 1], attention_levels=[1], kernel_size=3, padding_mode="zeros")


def _net(seed=11):
    torch.manual_seed(seed)
    return ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, **CFG).to(dev())


def _held_out(seed=5, n=8):
    return torch.randn(n, 6, 32, 32, generator=torch.Generator().manual_seed(seed)) * 0.5 + 0.5


def _scale_rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def test_fp32_table_matches_the_cpu_oracle():
    """evaluate on the regenerated noise of its own plan against the oracle's unreduced loss on the same (t, eps): 1e-4 scale-relative,
    the project's fp32 north-star."""
    net, pipe, K = _net(), SDAPipeline(), 10
    x = _held_out()
    res = evaluate(net, pipe, x.to(dev()), batch=8, bins=K, seed=3, precision="fp32", window=3)
    (p,) = validation_plan(8, 8, seed=3)
    eps = torch.empty((8, 6, 32, 32), dtype=torch.float32, device=dev())
    ops.philox_normal(eps, eps.numel(), p.noise_seed)
    ref = ou.OracleScoreUNet({k: v.detach().cpu() for k, v in net.state_dict().items()}, CFG["hidden_blocks"], CFG["attention_levels"])
    with torch.no_grad():
        sq = od.loss(ref, x, p.t.view(-1, 1, 1, 1), eps.cpu()).double()
    want = torch.zeros(K, 6, dtype=torch.float64).index_add_(0, level_bins(p.t, K), sq.sum(dim=(2, 3)))
    got = res.table.cpu()
    print(f"fp32 table vs CPU oracle: scale-relative {_scale_rel(got, want):.3e}")
    assert _scale_rel(got, want) <= 1e-4
    assert res.count.cpu().tolist() == np.bincount(level_bins(p.t, K).numpy(), minlength=K).tolist()
    assert res.mean() == pytest.approx(float(sq.mean()), rel=1e-4)


@pytest.mark.parametrize("dt,name", [(BF16, "bf16"), (F16, "fp16")])
def test_16bit_table_tracks_the_fp32_table(dt, name):
    worst = 0.0
    for seed in (1, 2, 3):
        net, pipe = _net(10 + seed), SDAPipeline()
        x = _held_out(seed).to(dev())
        a = evaluate(net, pipe, x, batch=8, bins=10, seed=seed, precision="fp32", window=3).table
        b = evaluate(net, pipe, x, batch=8, bins=10, seed=seed, precision=name, window=3).table
        worst = max(worst, _scale_rel(b, a))
    print(f"{name} table vs fp32 table, three seeds: worst scale-relative {worst:.3e} (asserted {TABLE_TOL[dt]:.3e})")
    assert worst <= TABLE_TOL[dt]


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_validate_on_the_live_weights_gives_the_training_steps_loss(precision, monkeypatch):
    """Trainer.validate(weights="net") with injected (t, eps) before any step, against the loss Trainer.step returns for the same batch.
    Both are fp32 sums of the same squared errors in different orders: the margin is the sum of the two float64 sum bounds
    (fp64_ref.mse_loss_sum for the step's loss tail, fp64_eval_ref for the table), computed on the rows an inference forward gives.
    16-bit: a step with regenerated noise would fuse the loss into the output conv, whose noise is the stream ROUNDED to half precision
    (DESIGN a9) -- another quantity; the comparison is made with C2W_NO_LOSS_FUSION=1, where the step's loss tail reads the fp32 noise.
    There the training forward and the inference forward are also two different 16-bit evaluations of the network (training keeps
    LayerNorm statistics and rebuilds residuals from normalised rows, inference does neither: the rows differ in last bits), each within
    DESIGN section 5's loss bound of the fp32 value; the margin adds twice that bound.  Observed on MI355X: fp32 3.2e-8 (margin 1.7e-5),
    bf16 6.7e-5 (6.9e-4), fp16 1.2e-6 (8.5e-5)."""
    monkeypatch.setenv("C2W_NO_LOSS_FUSION", "1")
    ops.knobs_reload()
    dt = {"fp32": F32, "bf16": BF16, "fp16": F16}[precision]
    net = _net()
    tr = Trainer(net, lr=1e-3, precision=precision, ema_rates=[0.999])
    monkeypatch.setattr(tr.eng, "fuse_loss", False)
    gen = torch.Generator().manual_seed(3)
    x = (torch.randn(8, 6, 32, 32, generator=gen) * 0.5 + 0.5).to(dev())
    t = torch.rand(8, generator=gen).to(dev())
    eps = torch.randn(8, 6, 32, 32, generator=gen).to(dev())
    val = tr.validate(x, weights="net", batch=8, bins=10, t=t, eps=eps, window=3)
    musig = torch.empty((8, 2), dtype=torch.float32, device=dev())
    ops.mu_sigma(t, musig, 8, tr.pipeline.eta)
    y = tr.eng.forward(x, t, dt, tape=None, noise=(eps, musig), nhwc_out=True)
    ldc, n = tr.eng.layout.cout_pad, 8 * 6 * 1024
    step_ref = R.mse_loss_sum(y, eps, 8, 6, 1024, ldc)
    tab_ref = E.sq_err_levels(y, eps, t, 8, 6, 1024, ldc, 10)
    loss = float(tr.step(x, t=t, eps=eps))
    margin = (step_ref.e.item() + tab_ref["table"].e.sum().item()) / n
    if dt != F32:
        margin += 2 * LOSS_PARITY[dt] * abs(loss)
    print(f"{precision}: validate {val.mean():.9g}, step {loss:.9g}, difference {abs(val.mean() - loss):.3e}, margin {margin:.3e}")
    assert abs(val.mean() * n - tab_ref["table"].v.sum().item()) <= tab_ref["table"].e.sum().item()
    assert abs(val.mean() - loss) <= margin


def _six_steps(validate: bool):
    net = _net()
    tr = Trainer(net, lr=2e-3, precision="bf16", ema_rates=[0.999], deterministic=True)
    gen = torch.Generator().manual_seed(3)
    base = torch.randn(8, 6, 32, 32, generator=gen) * 0.5 + 0.5
    held = _held_out(77, 5).to(dev())
    out = []
    for s in range(6):
        x = (base + 0.05 * torch.randn(8, 6, 32, 32, generator=gen)).to(dev())
        t = torch.rand(8, generator=gen).to(dev())
        eps = torch.randn(8, 6, 32, 32, generator=gen).to(dev())
        out.append(float(tr.step(x, t=t, eps=eps)).hex())
        if validate and s in (2, 4):
            v = tr.validate(held, weights="ema" if s == 2 else "net", batch=4, bins=4, seed=1, window=3)
            assert np.isfinite(v.mean()) and int(v.count.sum()) == 5
    torch.cuda.synchronize()
    for buf in (tr.eng.flat, tr.ema_flats[0], tr.m, tr.v):
        out.append(hashlib.sha256(buf.detach().cpu().numpy().tobytes()).hexdigest())
    out.append((tr.cur_ndata, tr.step_count, tr.rng_cpu.get_state().tolist(), tr.rng_dev.get_state().tolist()))
    return out


def test_validation_leaves_the_training_run_bit_for_bit_unchanged():
    """six deterministic bf16 steps with and without two validations: equal loss hex strings, equal digests of parameters, EMA and
    moments, equal counters and generator states"""
    assert _six_steps(True) == _six_steps(False)


@pytest.mark.parametrize("two_streams", ["0", "1"])
def test_two_validations_of_unchanged_weights_give_identical_bytes(two_streams, monkeypatch):
    monkeypatch.setenv("C2W_WGRAD_STREAM", two_streams)
    net = _net()
    tr = Trainer(net, lr=2e-3, precision="bf16", ema_rates=[0.999])
    gen = torch.Generator().manual_seed(3)
    x = (torch.randn(8, 6, 32, 32, generator=gen) * 0.5 + 0.5).to(dev())
    tr.step(x)
    held = _held_out(77, 7).to(dev())
    a = tr.validate(held, batch=4, bins=8, seed=2, window=3)
    b = tr.validate(held, batch=4, bins=8, seed=2, window=3)
    torch.cuda.synchronize()
    assert a.table.cpu().numpy().tobytes() == b.table.cpu().numpy().tobytes() and torch.equal(a.count, b.count)
    assert int(a.count.sum()) == 7 and a.mean() > 0


# ------------------------------------------------------------------------------------------------------------------ full-size default net

DEFAULT = dict(embedding_dim=512, hidden_blocks=[3] * 5, hidden_channels=[128, 128, 256, 384, 512], kernel_size=3, padding_mode="zeros",
               attention_levels=[4])


def test_full_size_net_on_lazy_windows():
    """C = 65 (13 frames x 5 variables), 128 x 128, B = 2, bf16, lazy WindowBatches of a device-resident feed: the table's total against
    the sum of SDAPipeline.loss's unreduced tensor computed by the fp32 path on the materialised stream (score._forward_loss), within
    DESIGN section 5's bf16 loss bound (3e-4); every cell with items is finite and positive."""
    torch.manual_seed(0)
    net = ScoreUNet(channels=65, spatial=2, activation=torch.nn.SiLU, **DEFAULT).to(dev())
    pipe = SDAPipeline()
    ds = SyntheticWindowDataset(14, 5, 128, 128, window=13, seed=4)
    feed = DeviceWindowFeed(ds, dev(), seed=1)
    cursor = feed.sampler.cursor
    res = evaluate(net, pipe, feed, batch=2, bins=10, seed=6, precision="bf16")
    assert feed.sampler.cursor == cursor and (res.F, res.w, res.H, res.W) == (5, 13, 128, 128)
    (p,) = validation_plan(2, 2, seed=6)
    eps = torch.empty((2, 65, 128, 128), dtype=torch.float32, device=dev())
    ops.philox_normal(eps, eps.numel(), p.noise_seed)
    x = feed.ordered_batch(0, 2).materialize()
    net.precision = "fp32"
    net.__dict__["_loss_request"] = dict(eps=eps, eta=pipe.eta)
    try:
        with torch.no_grad():
            want = net(x, p.t.to(dev())).double().sum().item()
    finally:
        net.__dict__.pop("_loss_request", None)
    got = res.table.sum().item()
    print(f"full-size bf16 table total {got:.9g} vs fp32 loss sum {want:.9g}: relative {abs(got - want) / want:.3e}")
    assert abs(got - want) <= 3e-4 * want
    tab, cnt = res.table.cpu().view(10, 13, 5), res.count.cpu()
    assert int(cnt.sum()) == 2
    cells = tab[cnt > 0]
    assert torch.isfinite(cells).all() and (cells > 0).all() and not tab[cnt == 0].any()
    assert np.isfinite(res.centre_frame()[cnt.numpy() > 0]).all()
