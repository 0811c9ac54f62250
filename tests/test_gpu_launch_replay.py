"""Every launch a real step makes on the GPU, replayed against its references (tests/launch_replay.py): the kernel tests call each kernel
with arguments their authors wrote down; here the arguments are the ones the ENGINE computes -- ldy != Cout with an emitted LayerNorm,
kvalid with packed weights and the fused loss, kept statistics, the chain form, split-K plans, grouped weight gradients with the real
layer counts, conv_center with the sampler's r0 / nr / ostride, window batches at i0 != 0, views into the flat parameter, shadow and
modulation buffers at their real offsets.

The net is the smallest that reaches every route: hidden_channels [128, 128, 256] (the fused LayerNorm epilogues are 128-channel
only), hidden_blocks [2, 1, 1] (two consecutive 128-channel blocks; three in the chain-form case), attention on the last level, 65 channels (the
padded edge convs and kvalid), 32 x 32 windows at B = 4 (levels 32^2, 16^2 and 8^2: paired images, T = 64 attention); a 32 x 64 leg
(8 x 16 at the attention level: T = 128, the blocked route) chosen with the library's *_supported queries, and a 52-channel leg.

Eager routes and one stream only: the harness synchronises around every launch, which a graph capture does not allow and which makes
the two-stream mode moot.  What this proves is kernel against reference at the engine's arguments -- not that the engine passes the
right arguments (tests/test_engine_emulated.py and the oracle parities), and nothing about races between launches.
"""
import time
from collections import Counter

import pytest
import torch

import launch_replay as LR
from climate2weather_amd import _lib, ops
from climate2weather_amd.data import WindowBatch
from climate2weather_amd.evaluation import evaluate
from climate2weather_amd.pipelines import SDAPipeline
from climate2weather_amd.score import ScoreUNet
from climate2weather_amd.score_fn import BatchedScoreFunction, PoolStrideOperator
from climate2weather_amd.training import Trainer
from test_gpu_launch_layer import knob  # noqa: F401  (the fixture: sets a knob, reloads the library's table, undoes both)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, F16 = ops.DTYPE_F32, ops.DTYPE_BF16, ops.DTYPE_F16
DT = {"fp32": F32, "bf16": BF16, "fp16": F16}
CFG = dict(embedding_dim=64, hidden_channels=[128, 128, 256], hidden_blocks=[2, 1, 1], attention_levels=[2], kernel_size=3, padding_mode="zeros")
B = 4
REPORTS = {}  # test id -> Report: the final test looks at the families and routes reached over the whole file
FAMILIES = {v: k for k, v in vars(_lib).items() if k.startswith("KERNEL_")}


def _net(channels=65, seed=3, activation=torch.nn.SiLU, **cfg):
    torch.manual_seed(seed)
    return ScoreUNet(channels=channels, spatial=2, activation=activation, **dict(CFG, **cfg)).to(DEV)


def _data(channels=65, H=32, W=32, seed=1, n=B):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, channels, H, W, generator=g) * 0.5 + 0.5).to(DEV)


def _windows(F=13, w=5, H=32, W=32, seed=2):
    """B overlapping, shuffled windows of a (frames, F, H, W) array: what a training batch is made of"""
    g = torch.Generator().manual_seed(seed)
    data = (torch.randn(8 + w, F, H, W, generator=g) * 0.5 + 0.5).to(DEV)
    return WindowBatch(data, torch.tensor([4, 0, 7, 2], dtype=torch.int64, device=DEV), w)


def _levels_supported(H, W, dt):
    """the queries the second shape was picked with: every level's 3x3 convs on the halo-patch kernels, the pooled input gradient, the
    fused LayerNorm epilogues on the 128-channel levels, the sampler's centre conv"""
    ok = True
    for lvl, C in enumerate((128, 128, 256)):
        h, w = H >> lvl, W >> lvl
        g = dict(B=B, Hin=h, Win=w, Cin=C, Hout=h, Wout=w, Cout=C, ldy=C, wrows=C, mode=ops.CONV_S1)
        ok = ok and ops.conv_patch_supported(g, dt)
        if C == 128 and dt != F32:
            ok = ok and ops.conv_lnfwd_supported(g, dt) and ops.conv_lnbwd_supported(g, dt)
    return ok and ops.conv_center_supported(H, W, 128, 13, dt)


def _replay(monkeypatch, request, body, mode="default", power=True):
    """run ``body`` under the harness; then (d) run it again with one border tap of channel 0 removed from the compared output of one
    engine-made conv launch: the replay must report exactly that launch"""
    t0 = time.perf_counter()
    with monkeypatch.context() as mp:
        rep = LR.install(mp, ops, mode=mode)
        body()
    rep.assert_clean()  # (a): nothing unchecked beyond the written list, every launch inside its references
    if power:
        hook, hit = LR.border_tap_defect()
        with monkeypatch.context() as mp:
            bad = LR.install(mp, ops, mode=mode, planted=hook)
            body()
        assert hit, "no conv launch took the planted defect"
        assert [f[0] for f in bad.failures] == hit, f"planted on launch {hit}, reported {[f[:2] for f in bad.failures]}"
    REPORTS[request.node.name] = rep
    print(f"\n== {request.node.name}: {sum(rep.seen.values())} launches, {time.perf_counter() - t0:.2f} s with the power-check run")
    for line in rep.lines():
        print("   " + line)
    print("   flags: " + ", ".join(f"{k} {v}" for k, v in sorted(rep.flags.items())))
    return rep


def _two_steps(precision, x, channels=65, chain=False, cfg={}, **kw):
    def body():
        tr = Trainer(_net(channels, **cfg), lr=1e-3, precision=precision, ema_rates=[0.999], seed=11, **kw)
        if chain:
            tr.eng.chain_blocks = True
        tr.step(x)
        tr.step(x)  # sees the optimizer's writes, the refreshed shadows and packed copies
        torch.cuda.synchronize()
    return body


def _expect(rep, *flags):
    missing = [f for f in flags if not rep.flags.get(f)]
    assert not missing, f"the launches this case is there for did not appear: {missing}; seen: {sorted(rep.flags)}"


TRAIN = ("conv", "ln_forward", "attention_forward", "attention_backward", "adamw_ema", "timestep_embedding", "mu_sigma")


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_two_training_steps_default_knobs(monkeypatch, request, precision):
    """case 1: window batches (the training feed's form), the EMA on, fp16 under the loss scaler"""
    rep = _replay(monkeypatch, request, _two_steps(precision, _windows()))
    for name in TRAIN:
        assert rep.seen[name] > 0, name
    assert rep.seen["conv_wgrad"] + rep.seen["conv_wgrad_grouped"] > 0
    _expect(rep, "conv:kvalid", "conv:pool2", "conv:y2", "conv:mul", "conv:res", "conv:mode2", "conv:mode3", "conv:mode4", "attention_forward:" + ("valu" if precision == "fp32" else "t64"))
    if precision != "fp32":
        _expect(rep, "conv:lnf", "conv:ln", "conv:ln.rstd", "adamw_ema:shadow", "windows_to_nhwc_noise:img_off")
    if precision == "fp16":
        _expect(rep, "adamw_ema:scaler")
        assert rep.seen["grad_scaler_check"] == 2 and rep.seen["grad_scaler_update"] == 2


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_two_training_steps_on_the_16x16_tile_kernel(monkeypatch, request, knob, precision):  # noqa: F811
    """case 2: C2W_CONV_T3=16 -- packed weights, the fused loss, the lnf / ln epilogues with kept statistics, pooled input gradients"""
    knob("C2W_CONV_T3", "16")
    rep = _replay(monkeypatch, request, _two_steps(precision, _data()))
    _expect(rep, "conv:loss", "conv:wpacked", "conv:lnf", "conv:ln.rstd", "conv:lnf.rstd", "conv:pool2", "conv:kvalid", "conv:family%d" % _lib.KERNEL_PATCH_16X16)
    assert rep.packed_resolved == rep.flags["conv:wpacked"]
    assert rep.seen["nchw_to_nhwc_noise_rows"] > 0


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_two_training_steps_in_the_chain_form(monkeypatch, request, knob, precision):  # noqa: F811
    """case 3: Engine.chain_blocks -- resn, no_y, lnf["mean"]; at this size the chain kernels exist under C2W_CONV_T3=16 only.  A block
    hands over only where the NEXT block's second conv emits a LayerNorm too (forward.py::run_blocks), which on a descent side takes a
    third block behind it: three blocks on the 128-channel top level here."""
    g = dict(B=B, Hin=32, Win=32, Cin=128, Hout=32, Wout=32, Cout=128, ldy=128, wrows=128, mode=ops.CONV_S1)
    if not ops.conv_lnfwd_chain_supported(g, DT[precision]):
        knob("C2W_CONV_T3", "16")
    assert ops.conv_lnfwd_chain_supported(g, DT[precision])
    rep = _replay(monkeypatch, request, _two_steps(precision, _data(), chain=True, cfg=dict(hidden_blocks=[3, 1, 1])))
    _expect(rep, "conv:resn", "conv:no_y", "conv:lnf.mean")


def test_two_deterministic_training_steps(monkeypatch, request):
    """case 4"""
    rep = _replay(monkeypatch, request, _two_steps("bf16", _windows(), deterministic=True), mode="det")
    assert any(k.endswith(":det") or k.endswith(":deterministic") for k in rep.flags), sorted(rep.flags)


@pytest.mark.parametrize("name,value,flag", [("C2W_CONV_S2_PATCH", "2", "conv:family%d" % _lib.KERNEL_PATCH_S2), ("C2W_ATTN_VALU", "1", "attention_forward:valu")])
def test_one_training_step_under_a_knob(monkeypatch, request, knob, name, value, flag):  # noqa: F811
    """case 5: the stride-2 patch forward; the VALU attention route in bf16"""
    knob(name, value)

    def body():
        Trainer(_net(), lr=1e-3, precision="bf16", ema_rates=[0.999], seed=11).step(_data())
        torch.cuda.synchronize()
    _expect(_replay(monkeypatch, request, body), flag)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_two_training_steps_on_a_field_that_is_not_square(monkeypatch, request, precision):
    """the second shape: 32 x 64 -- 8 x 16 at the attention level, T = 128: the blocked attention route"""
    assert _levels_supported(32, 64, DT[precision])
    rep = _replay(monkeypatch, request, _two_steps(precision, _data(H=32, W=64)))
    _expect(rep, "attention_forward:blocks", "attention_backward:blocks", "conv:lnf", "conv:ln")


@pytest.mark.parametrize("precision", ["bf16"])
def test_two_training_steps_at_52_channels(monkeypatch, request, precision):
    """the reference's own width: another K padding of the edge convs"""
    rep = _replay(monkeypatch, request, _two_steps(precision, _windows(F=4, w=13), channels=52))
    _expect(rep, "conv:kvalid")


def _sampler(precision, gamma, exact=False, steps=2, corrections=1, L=11, activation=torch.nn.SiLU):
    F, k = 13, 2
    net = _net(activation=activation).eval().requires_grad_(False)
    net.precision = precision
    pipe = SDAPipeline()
    g = torch.Generator().manual_seed(5)
    A = PoolStrideOperator(8, 2)
    truth = torch.randn(L, F, 32, 32, generator=g)
    noise = torch.randn(L, F, 32, 32, generator=g)
    zs = [torch.randn(L, F, 32, 32, generator=g) for _ in range(steps * corrections)]
    std = (torch.rand(1, F, 1, 1, generator=g) * 0.2 + 0.1)

    def body():
        sf = BatchedScoreFunction(net, markov_order=k, batch_size=3, device=torch.device(DEV), noise_process=pipe)  # 7 windows: 3 + 3 + 1
        assert not sf.use_graphs
        net._get_engine().use_center_conv = True
        if exact:
            sf.exact_streamed = True
        sf.condition_on(A=A, y=A(truth), std=std, gamma=gamma, exact_grad=exact)
        pipe.sample(sf, noise, steps=steps, corrections=corrections, tau=0.4, device=torch.device(DEV), show_progressbar=False, z_draws=zs)
        torch.cuda.synchronize()
    return body


@pytest.mark.parametrize("gamma", ["scalar", "per-variable"])
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_two_sampler_steps_with_a_corrector(monkeypatch, request, precision, gamma):
    """case 6: BatchedScoreFunction (eager) inside SDAPipeline.sample: three window batches, the last one partial"""
    gam = 1e-2 if gamma == "scalar" else (torch.rand(1, 13, 1, 1, generator=torch.Generator().manual_seed(8)) * 0.05 + 1e-3)
    rep = _replay(monkeypatch, request, _sampler(precision, gam))
    for name in ("window_gather", "conv_center", "sampler_predict", "sampler_correct", "sumsq", "guidance", "gemv_f32"):
        assert rep.seen[name] > 0, (name, dict(rep.seen))
    assert rep.flags["window_gather:i0!=0"] + rep.flags["window_scatter:i0!=0"] > 0
    _expect(rep, "conv:splitk")  # the split-K plans of inference
    assert (rep.flags["guidance:gamma[F]"] > 0) == (gamma == "per-variable")


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_two_training_steps_of_a_relu_network(monkeypatch, request, precision):
    """case 9: torch.nn.ReLU, the reference UNet's own default activation (model/nn.py:118): C2W_ACT_RELU_PAIR on every block's first conv,
    its mask as the multiplier of the input-gradient convs; every conv launch with its float64 bound, the mask by its consistency rule"""
    rep = _replay(monkeypatch, request, _two_steps(precision, _windows(), cfg=dict(activation=torch.nn.ReLU)))
    _expect(rep, "conv:relu_pair", "conv:mul", "conv:lnf", "conv:ln.rstd")
    assert rep.bounded_flags["conv:relu_pair"] == rep.flags["conv:relu_pair"] and rep.bounded["conv"] == rep.checked["conv"]


def test_one_sampler_step_of_a_relu_network(monkeypatch, request):
    """case 10: inference takes C2W_ACT_RELU in the accumulator epilogue, through the split-K reduction too, and the gemv's ReLU"""
    rep = _replay(monkeypatch, request, _sampler("bf16", 1e-2, steps=1, corrections=0, activation=torch.nn.ReLU))
    _expect(rep, "conv:relu", "conv:splitk")
    assert rep.bounded_flags["conv:relu"] == rep.flags["conv:relu"] and rep.bounded["conv"] == rep.checked["conv"]


def test_one_sampler_step_with_streamed_exact_guidance(monkeypatch, request):
    """case 7: the window-list kernels and backward(want_dw=False)"""
    rep = _replay(monkeypatch, request, _sampler("bf16", 1e-2, exact=True, steps=1, corrections=0), mode="exact")
    for name in ("guidance_delta", "window_gather_list", "window_cotangent_list", "window_grad_fold_list"):
        assert rep.seen[name] > 0, (name, dict(rep.seen))
    assert rep.seen["conv_wgrad"] + rep.seen["conv_wgrad_grouped"] == 0


def test_validation_on_two_batches(monkeypatch, request):
    """case 8: evaluation.evaluate (sq_err_levels)"""
    net = _net(channels=15).eval()
    x = _data(channels=15, n=8)

    def body():
        evaluate(net, SDAPipeline(), x, batch=4, bins=10, seed=3, precision="bf16", window=3)
        torch.cuda.synchronize()
    rep = _replay(monkeypatch, request, body, mode="eval")
    assert rep.seen["sq_err_levels"] == 2


CASES = 22  # parametrised cases above


def test_every_conv_family_and_attention_route_was_reached():
    """(c): over the whole file, from the reports the cases above collected (a run of a part of the file has nothing to say here)"""
    if len(REPORTS) < CASES:
        return
    fams, routes = set(), set()
    seen, bounded = Counter(), Counter()
    for rep in REPORTS.values():
        fams |= set(rep.families)
        routes |= set(rep.routes)
        seen.update(rep.flags)
        bounded.update(rep.bounded_flags)
    for flag in ("conv:relu", "conv:relu_pair", "conv:resn", "conv:no_y", "conv:lnf.mean", "conv:ln.rstd"):  # no conv launch left unmodelled
        assert seen[flag] > 0 and bounded[flag] == seen[flag], f"{flag}: {seen[flag]} launches seen, {bounded[flag]} with a float64 bound"
    assert fams == set(FAMILIES), f"conv families not reached: {[FAMILIES[f] for f in set(FAMILIES) - fams]}"
    assert routes == {"valu", "t64", "blocks"}, routes
