"""The launch-replay harness (tests/launch_replay.py) tested without a GPU: the CPU doubles are installed as the launchers and the
harness goes on top, so "real" and reference are the same function -- every launch of a tiny bf16 training step and of a two-step
sampler must be checked and pass with ratio 0 -- and then the harness must REJECT defects planted into a double's output (a dropped
8x16 tile, a written input, a written padding column, an addition where the op overwrites, a launcher without a reference, a packed
operand nobody packed), naming the launch.  Nothing here touches a device."""
import pytest
import torch

import emu_ops
import launch_replay as LR
from climate2weather_amd import ops as c2w_ops
from climate2weather_amd.pipelines import SDAPipeline
from climate2weather_amd.score import ScoreUNet
from climate2weather_amd.score_fn import BatchedScoreFunction, PoolStrideOperator
from climate2weather_amd.training import Trainer

CPU = torch.device("cpu")


def _net(hidden=(64, 64), blocks=(1, 1), activation=torch.nn.SiLU):
    torch.manual_seed(3)
    return ScoreUNet(channels=6, spatial=2, activation=activation, embedding_dim=64, hidden_channels=list(hidden), hidden_blocks=list(blocks),
                     attention_levels=[1], kernel_size=3, padding_mode="zeros")


def _batch(B=2, seed=1):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, 6, 16, 16, generator=gen) * 0.5 + 0.5, torch.rand(B, generator=gen), torch.randn(B, 6, 16, 16, generator=gen)


def _train(monkeypatch, planted=None, packed=False, steps=1, precision="bf16", activation=torch.nn.SiLU):
    emu_ops.install(monkeypatch, c2w_ops)
    monkeypatch.delenv("C2W_DETERMINISTIC", raising=False)
    if packed:
        monkeypatch.setattr(emu_ops, "PACKED_FROM_PIXELS", 1)
    rep = LR.install(monkeypatch, c2w_ops, mode="default", planted=planted)
    x, t, eps = _batch()
    tr = Trainer(_net(activation=activation), lr=1e-3, precision=precision, ema_rates=[0.9])
    for _ in range(steps):
        tr.step(x, t=t, eps=eps)
    return rep


def _all_zero(rep):
    """the restatement ratios that are not 0 (the float64 bounds are the kernels' error model: recorded for a double, not asserted)"""
    return {(n, k): v for n, d in rep.worst.items() for k, v in d.items() if v != 0.0 and not k.startswith("fp64 ")}


def test_every_launch_of_a_bf16_training_step_is_checked_with_ratio_zero(monkeypatch):
    rep = _train(monkeypatch, steps=2)
    rep.assert_clean()
    assert sum(rep.seen.values()) > 100 and rep.seen == rep.checked
    for name in ("conv", "conv_wgrad", "ln_forward", "attention_forward", "attention_backward", "adamw_ema", "mse_loss_grad", "nchw_to_nhwc"):
        assert rep.seen[name] > 0, name
    assert set(rep.unchecked) <= set(LR.UNCHECKED) | {n for n in rep.unchecked if LR.is_host_query(n)}
    assert not _all_zero(rep), _all_zero(rep)
    assert rep.bounded["conv"] == rep.checked["conv"] and rep.bounded["conv_wgrad"] + rep.bounded["conv_wgrad_grouped"] > 0 and rep.bounded["adamw_ema"] > 0


def test_every_launch_of_a_relu_training_step_is_checked_with_ratio_zero(monkeypatch):
    """the reference UNet's own default activation: the ReLU pair in training (the mask's consistency rule runs on every such launch), and
    no conv launch without its float64 bound"""
    rep = _train(monkeypatch, activation=torch.nn.ReLU)
    rep.assert_clean()
    assert rep.seen == rep.checked and not _all_zero(rep), _all_zero(rep)
    assert rep.flags["conv:relu_pair"] > 0 and rep.bounded_flags["conv:relu_pair"] == rep.flags["conv:relu_pair"]
    assert rep.worst["conv"]["fp64 conv relu mask"] == 0.0
    assert rep.bounded["conv"] == rep.checked["conv"]


def test_every_launch_of_a_deterministic_step_is_checked(monkeypatch):
    import emu_det_ops
    emu_det_ops.install(monkeypatch, c2w_ops)
    rep = LR.install(monkeypatch, c2w_ops, mode="det")
    x, t, eps = _batch()
    Trainer(_net(), lr=1e-3, precision="bf16", ema_rates=[0.9], deterministic=True).step(x, t=t, eps=eps)
    rep.assert_clean()
    assert not _all_zero(rep), _all_zero(rep)
    assert any(k.endswith(":det") or k.endswith(":deterministic") for k in rep.flags), sorted(rep.flags)


def _sampler(monkeypatch, planted=None, gamma=1e-2):
    emu_ops.install(monkeypatch, c2w_ops)
    rep = LR.install(monkeypatch, c2w_ops, mode="default", planted=planted)
    net = _net().eval()
    pipe = SDAPipeline()
    sf = BatchedScoreFunction(net, markov_order=1, batch_size=3, device=CPU, noise_process=pipe)
    g = torch.Generator().manual_seed(5)
    A = PoolStrideOperator(8, 2)
    truth = torch.randn(6, 2, 16, 16, generator=g)
    sf.condition_on(A=A, y=A(truth), std=torch.tensor([0.1, 0.2]).view(1, 2, 1, 1), gamma=gamma, exact_grad=False)
    noise = torch.randn(6, 2, 16, 16, generator=g)
    zs = [torch.randn(6, 2, 16, 16, generator=g) for _ in range(2)]
    pipe.sample(sf, noise, steps=2, corrections=1, tau=0.4, device=CPU, show_progressbar=False, z_draws=zs)
    return rep


@pytest.mark.parametrize("gamma", [1e-2, "per-variable"])
def test_every_launch_of_a_two_step_sampler_is_checked_with_ratio_zero(monkeypatch, gamma):
    rep = _sampler(monkeypatch, gamma=torch.tensor([1e-2, 3e-2]).view(1, 2, 1, 1) if gamma == "per-variable" else gamma)
    rep.assert_clean()
    for name in ("window_gather", "window_scatter", "conv", "conv_center", "gemv_f32", "guidance"):  # (the fused update kernels: device only)
        assert rep.seen[name] > 0, (name, dict(rep.seen))
    assert rep.flags["window_scatter:i0!=0"] > 0  # a window batch that does not start at window 0
    assert (rep.flags["guidance:gamma[F]"] > 0) == (gamma == "per-variable")
    assert not _all_zero(rep), _all_zero(rep)


def test_packed_weight_map_resolves_every_packed_operand(monkeypatch):
    rep = _train(monkeypatch, packed=True, steps=2)
    rep.assert_clean()
    assert rep.flags["conv:wpacked"] > 0 and rep.packed_resolved == rep.flags["conv:wpacked"]
    assert not _all_zero(rep), _all_zero(rep)


# ------------------------------------------------------------------------------------------------------------- the aliasing rule

def _conv_args(res_is_y=False):
    g = dict(B=1, Hin=8, Win=16, Cin=64, Hout=8, Wout=16, Cout=64, ldy=64, wrows=64, mode=emu_ops.CONV_S1)
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(128, 64, generator=gen)
    w = torch.randn(64, 9, 64, generator=gen) / 24
    buf = torch.randn(128 * 64 + 64, generator=gen)
    return g, x, w, buf


def test_an_output_that_is_its_own_residual_shares_one_clone(monkeypatch):
    emu_ops.install(monkeypatch, c2w_ops)
    rep = LR.install(monkeypatch, c2w_ops)
    g, x, w, buf = _conv_args()
    y = buf[: 128 * 64].view(128, 64)
    c2w_ops.conv(x, w, None, y, g, c2w_ops.DTYPE_F32, res=y)
    rep.assert_clean()
    assert rep.checked["conv"] == 1 and not _all_zero(rep)


def test_nan_garbage_behind_an_open_ended_output_is_not_a_difference(monkeypatch):
    """score_fn hands the launchers views of a torch.empty trajectory: what a call leaves alone may hold anything, NaNs included.  They
    have equal bits before and after on both sides and must not fail the comparison -- while a NaN the launcher WRITES still does."""
    emu_ops.install(monkeypatch, c2w_ops)
    rep = LR.install(monkeypatch, c2w_ops)
    F, HW, k, nw, nwin = 2, 16, 1, 2, 6
    eps = torch.full((8 * F * HW,), float("nan"))
    y = torch.randn(nw * HW, 32, generator=torch.Generator().manual_seed(4))
    c2w_ops.window_scatter(y, eps, nw, F, HW, k, 2, nwin, 32, c2w_ops.DTYPE_F32)
    H, W = 8, 16
    out = torch.full((6 * 3 * H * W,), float("nan"))
    x, w = torch.randn(2 * H * W, 64, generator=torch.Generator().manual_seed(5)), torch.randn(9 * 9 * 64, generator=torch.Generator().manual_seed(6)) / 24
    c2w_ops.conv_center(x, w, None, out[3 * H * W:], 2, H, W, 64, 9, 3, 3, 3 * H * W, c2w_ops.DTYPE_F32)
    rep.assert_clean()
    assert rep.checked["window_scatter"] == 1 and rep.checked["conv_center"] == 1 and not torch.isnan(eps[3 * F * HW: 5 * F * HW]).any()

    def nan_out(call):
        call.real["eps"].reshape(-1)[3 * F * HW + 1] = float("nan")
    bad = LR.install(monkeypatch, c2w_ops, planted=nan_out)
    c2w_ops.window_scatter(y, eps, nw, F, HW, k, 2, nwin, 32, c2w_ops.DTYPE_F32)
    assert [f[1] for f in bad.failures] == ["window_scatter"]


def test_a_written_argument_that_partially_overlaps_another_is_an_error(monkeypatch):
    emu_ops.install(monkeypatch, c2w_ops)
    LR.install(monkeypatch, c2w_ops)
    g, x, w, buf = _conv_args()
    y, res = buf[: 128 * 64].view(128, 64), buf[64:].view(128, 64)
    with pytest.raises(LR.AliasError, match=r"launch 0 \(conv\): written argument y partially overlaps argument res"):
        c2w_ops.conv(x, w, None, y, g, c2w_ops.DTYPE_F32, res=res)


# ------------------------------------------------------------------------------------------------------------ planted defects

def _nth(name, n, defect, accept=lambda call: True):
    """a hook that applies ``defect(call)`` to the n-th launch of ``name`` that ``accept`` takes; hit[0] = that launch's index"""
    seen, hit = [], []

    def hook(call):
        if call.name == name and accept(call):
            seen.append(call.index)
            if len(seen) == n + 1:
                hit.append(call.index)
                defect(call)
    return hook, hit


def _y_rows(call):
    g = call.real["g"]
    return LR.rows(call.real["y"], g["B"] * g["Hout"] * g["Wout"], g["ldy"]), g


def _drop_tile(call):
    y, g = _y_rows(call)
    y.view(g["B"], g["Hout"], g["Wout"], g["ldy"])[0, 0:8, 0:16, : g["Cout"]] = LR.rows(call.snap["y"], y.shape[0], g["ldy"]).view(
        g["B"], g["Hout"], g["Wout"], g["ldy"])[0, 0:8, 0:16, : g["Cout"]]  # the tile keeps what the buffer held


def _write_input(call):
    call.real["x"].reshape(-1)[5] += 1.0


def _write_padding(call):
    y, g = _y_rows(call)
    y[3, g["Cout"]] = 1.0


def _add(call):
    y, g = _y_rows(call)
    y[:, : g["Cout"]] += LR.rows(call.snap["y"], y.shape[0], g["ldy"])[:, : g["Cout"]]


def _plain3x3(call):
    a = call.real
    g = a["g"]
    return g["mode"] == emu_ops.CONV_S1 and g["Hout"] == 16 and a["ln"] is None and a["lnf"] is None and a["act"] == 0 and a["mul"] is None \
        and not a["pool2"] and a["loss"] is None


DEFECTS = {
    "a dropped 8x16 tile": (_drop_tile, _plain3x3, "vs restatement"),
    "one element of an input written": (_write_input, _plain3x3, "does not write was written"),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_a_planted_defect_is_rejected_and_the_launch_named(monkeypatch, defect):
    fn, accept, msg = DEFECTS[defect]
    hook, hit = _nth("conv", 1, fn, accept)
    rep = _train(monkeypatch, planted=hook)
    assert hit, "no launch took the defect"
    assert rep.failures and rep.failures[0][0] == hit[0] and rep.failures[0][1] == "conv" and msg in rep.failures[0][2], rep.failures[:2]
    with pytest.raises(AssertionError, match=r"launch %d \(conv\)" % hit[0]):
        rep.assert_clean()


def test_an_addition_where_the_op_overwrites_is_rejected(monkeypatch):
    """a launcher that adds its result onto what the buffer held (ones here)"""
    emu_ops.install(monkeypatch, c2w_ops)
    hook, hit = _nth("conv", 0, _add)
    rep = LR.install(monkeypatch, c2w_ops, planted=hook)
    g, x, w, _ = _conv_args()
    c2w_ops.conv(x, w, None, torch.ones(128, 64), g, c2w_ops.DTYPE_F32)
    assert hit == [0] and [f[:2] for f in rep.failures] == [(0, "conv")] and "y vs restatement" in rep.failures[0][2], rep.failures


def test_a_written_padding_column_is_rejected(monkeypatch):
    """rows of ldy = 72 with 64 real channels: column 64 of one row written"""
    emu_ops.install(monkeypatch, c2w_ops)
    hook, hit = _nth("conv", 0, _write_padding)
    rep = LR.install(monkeypatch, c2w_ops, planted=hook)
    g, x, w, _ = _conv_args()
    g["ldy"] = 72
    c2w_ops.conv(x, w, None, torch.zeros(128, 72), g, c2w_ops.DTYPE_F32)
    assert hit == [0] and [f[:2] for f in rep.failures] == [(0, "conv")] and "outside the 128 x 64 (stride 72)" in rep.failures[0][2], rep.failures
    c2w_ops.conv(x, w, None, torch.zeros(128, 72), g, c2w_ops.DTYPE_F32)  # the same launch without the defect passes
    assert len(rep.failures) == 1 and rep.checked["conv"] == 2


def test_a_launcher_without_a_reference_is_rejected(monkeypatch):
    emu_ops.install(monkeypatch, c2w_ops)
    monkeypatch.setattr(c2w_ops, "rapsd", lambda x, spec, n_fields, H, W: True)  # a kernel launcher the replay has no reference for
    rep = LR.install(monkeypatch, c2w_ops)
    c2w_ops.rapsd(torch.zeros(1, 8, 8), torch.zeros(1, 4), 1, 8, 8)
    assert rep.failures == [(0, "rapsd", "a launcher without a reference")]
    with pytest.raises(AssertionError, match="rapsd"):
        rep.assert_clean()
    assert "rapsd" not in LR.UNCHECKED and not LR.is_host_query("rapsd")


def test_an_unresolved_packed_operand_is_rejected(monkeypatch):
    emu_ops.install(monkeypatch, c2w_ops)
    monkeypatch.setattr(emu_ops, "PACKED_FROM_PIXELS", 1)
    rep = LR.install(monkeypatch, c2w_ops)
    g, x, w, buf = _conv_args()
    y = torch.zeros(128, 64, dtype=torch.bfloat16)
    c2w_ops.conv(x.bfloat16(), -w.bfloat16(), None, y, g, c2w_ops.DTYPE_BF16, wpacked=True)  # nobody packed this operand
    assert len(rep.failures) == 1 and rep.failures[0][:2] == (0, "conv") and "packed weight operand" in rep.failures[0][2]


def test_the_unchecked_list_is_the_written_one():
    assert set(LR.UNCHECKED) == {"knobs_reload", "new_workspace", "publish_scalar", "pack_conv_weights_batched", "check"}
    kernels = [n for n in LR.SIGS if n not in LR.UNCHECKED and not LR.is_host_query(n)]
    metrics = {"rapsd", "ssim", "swd_project", "swd_project_pair", "swd_distance", "kde_eval", "kde_partial", "kde_fold", "pit_counts", "quantiles",
               "crps_terms"}  # the ensemble-metric kernels: one call site each, their own bounded tests; a replayed step never reaches them
    assert sorted(n for n in kernels if n not in LR.WRITES) == sorted(metrics)


def test_dispatch_arithmetic_of_the_gpu_cases(monkeypatch):
    """tests/test_gpu_launch_replay.py relies on these answers of the library's host queries (they need no device): which kernel family
    each level of its net runs on, and that C2W_CONV_T3=16 brings the 16x16-tile kernel with packed weights, the fused loss and the
    chain form to its size"""
    from climate2weather_amd import _lib
    real = {n: getattr(c2w_ops, n) for n in ("conv_dispatch", "conv_splitk_plan", "conv_loss_supported", "conv_lnfwd_chain_supported",
                                             "conv_wpacked_supported", "conv_patch_supported", "conv_center_supported", "knobs_reload")}
    BF16 = c2w_ops.DTYPE_BF16
    g = dict(B=4, Hin=32, Win=32, Cin=128, Hout=32, Wout=32, Cout=128, ldy=128, wrows=128, mode=c2w_ops.CONV_S1)
    small = dict(g, Hin=8, Win=8, Hout=8, Wout=8, Cin=256, Cout=256, ldy=256, wrows=256)
    monkeypatch.delenv("C2W_CONV_T3", raising=False)
    real["knobs_reload"]()
    try:
        assert real["conv_dispatch"](g, BF16) == _lib.KERNEL_PATCH_8X16 and real["conv_dispatch"](small, BF16) == _lib.KERNEL_PATCH_PAIR
        assert real["conv_dispatch"](dict(g, Hout=16, Wout=16, mode=c2w_ops.CONV_S2), BF16) == _lib.KERNEL_GATHER
        assert real["conv_dispatch"](dict(g, Hin=16, Win=16, mode=c2w_ops.CONV_TS2), BF16) == _lib.KERNEL_PATCH_TS2
        assert real["conv_splitk_plan"](g, BF16)[0] > 1 and not real["conv_loss_supported"](dict(g, wrows=65), BF16)
        assert not real["conv_lnfwd_chain_supported"](g, BF16)
        for H, W in ((32, 32), (32, 64), (16, 32), (8, 16)):
            assert real["conv_patch_supported"](dict(g, Hin=H, Win=W, Hout=H, Wout=W), BF16), (H, W)
        assert real["conv_center_supported"](32, 32, 128, 13, BF16)
        monkeypatch.setenv("C2W_CONV_T3", "16")
        real["knobs_reload"]()
        assert real["conv_dispatch"](g, BF16) == _lib.KERNEL_PATCH_16X16 and real["conv_wpacked_supported"](g, BF16)
        assert real["conv_loss_supported"](dict(g, wrows=65), BF16) and real["conv_lnfwd_chain_supported"](g, BF16)
    finally:
        monkeypatch.delenv("C2W_CONV_T3", raising=False)
        real["knobs_reload"]()
