"""Pins the launch order of the host engine: every ``ops.*`` call of a forward (and its backward), by name, argument shapes / dtypes and
scalar values, against the trace recorded in tests/launch_order_tiny.json.  The launchers are the CPU test doubles (tests/emu_ops.py,
tests/emu_det_ops.py); the few the doubles lack (the regenerated-noise input conversions) get stand-ins here.

The JSON was recorded BEFORE Engine.forward was split into climate2weather_amd/forward.py and is not regenerated when the orchestration is
refactored: a behaviour-preserving change of the engine leaves every trace as it is.  A change that adds, drops, reorders or re-shapes a
launch on purpose re-records it with ``C2W_RECORD_LAUNCH_ORDER=1 python -m pytest tests/test_engine_launch_order.py`` and says so."""
import json
import os

import pytest
import torch

import emu_det_ops
import emu_ops
from climate2weather_amd import ops as c2w_ops
from climate2weather_amd.data import WindowBatch
from climate2weather_amd.engine import Tape
from climate2weather_amd.pipelines import SDAPipeline
from climate2weather_amd.score import ScoreUNet
from climate2weather_amd.score_fn import BatchedScoreFunction
from climate2weather_amd.training import Trainer
from test_engine_emulated import _tiny

TRACES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "launch_order_tiny.json")
DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16", torch.int64: "i64", torch.int32: "i32", torch.bool: "b8"}
NOISE_STANDINS = ["nchw_to_nhwc_noise", "nchw_to_nhwc_noise_rows", "windows_to_nhwc_noise", "philox_normal"]


def _fmt(v):
    if isinstance(v, torch.Tensor):
        return "%s%s" % (DT.get(v.dtype, str(v.dtype)), list(v.shape))
    if isinstance(v, dict):
        return "{" + ",".join("%s=%s" % (k, _fmt(x)) for k, x in v.items()) + "}"
    if isinstance(v, (list, tuple)):
        return "[" + ",".join(_fmt(x) for x in v) + "]"
    if v is None or isinstance(v, (bool, int, str)):
        return str(v)
    if isinstance(v, float):
        return repr(v)
    return type(v).__name__


def _record(monkeypatch, log):
    """Wrap every launcher the test doubles installed on climate2weather_amd.ops with a recorder."""
    names = sorted(set(emu_ops.ALL) | set(emu_det_ops.NEW_NAMES) | set(emu_det_ops.WRAPPED) | set(NOISE_STANDINS) | {"new_workspace"})
    for name in names:
        fn = getattr(c2w_ops, name, None)
        if fn is None or not callable(fn) or name == "install":
            continue

        def rec(*a, _fn=fn, _name=name, **kw):
            log.append(" ".join([_name] + [_fmt(x) for x in a] + ["%s=%s" % (k, _fmt(x)) for k, x in kw.items()]))
            return _fn(*a, **kw)
        monkeypatch.setattr(c2w_ops, name, rec)


# ---- stand-ins for the regenerated-noise input conversions (the doubles have no Philox stream): ``ACCEPT`` names those that take the
# shape; the others answer False, as the library does outside its domain
ACCEPT = set()


def _eps_of(seed, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(int(seed) & 0xFFFF))


def _philox_normal(out, n, seed):
    out.copy_(_eps_of(seed, out.shape))


def _nchw_to_nhwc_noise(x, seed, musig, y, B, C, HW, ldc, dtype):
    if "nchw_to_nhwc_noise" not in ACCEPT:
        return False
    emu_ops.nchw_to_nhwc(x, _eps_of(seed, x.shape), musig, y, B, C, HW, ldc, dtype)
    return True


def _gather(data, img_off, B, C, HW):
    flat = data.reshape(-1)
    return torch.stack([flat[o:o + C * HW] for o in img_off.tolist()]).view(B, C, HW)


def _windows_to_nhwc_noise(data, img_off, seed, musig, y, B, C, HW, ldc, dtype):
    if "windows_to_nhwc_noise" not in ACCEPT:
        return False
    x = _gather(data, img_off, B, C, HW)
    emu_ops.nchw_to_nhwc(x, _eps_of(seed, x.shape), musig, y, B, C, HW, ldc, dtype)
    return True


def _nchw_to_nhwc_noise_rows(x, img_off, seed, musig, y, erows, B, C, HW, ldc, lde, dtype):
    if "nchw_to_nhwc_noise_rows" not in ACCEPT:
        return False
    if img_off is not None:
        x = _gather(x, img_off, B, C, HW)
    eps = _eps_of(seed, (B, C, HW)).half()
    erows.zero_()
    erows.view(B, HW, lde)[:, :, :C] = eps.permute(0, 2, 1)
    emu_ops.nchw_to_nhwc(x.reshape(B, C, HW), eps.float(), musig, y, B, C, HW, ldc, dtype)
    return True


def _install(monkeypatch, log, det=False, accept=(), fused_loss=False):
    (emu_det_ops if det else emu_ops).install(monkeypatch, c2w_ops)
    monkeypatch.delenv("C2W_DETERMINISTIC", raising=False)
    monkeypatch.setattr(emu_ops, "CHAIN", True)
    ACCEPT.clear()
    ACCEPT.update(accept)
    for name in NOISE_STANDINS:
        monkeypatch.setattr(c2w_ops, name, globals()["_" + name])
    if fused_loss:  # the output conv "takes" the loss tail: the stand-in drops the argument (the numbers are not what this test is about)
        real = c2w_ops.conv
        monkeypatch.setattr(c2w_ops, "conv_loss_supported", lambda g, dtype: True)
        monkeypatch.setattr(c2w_ops, "conv", lambda *a, loss=None, **kw: real(*a, **kw))
    _record(monkeypatch, log)


def _inputs(B=2, seed=1):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 6, 16, 16, generator=gen) * 0.5 + 0.5
    return x, torch.rand(B, generator=gen), torch.randn(B, 6, 16, 16, generator=gen)


def _net(hidden_channels=None, hidden_blocks=(1, 1), attention_levels=(1,), forcing_dim=0):
    if hidden_channels is None and tuple(hidden_blocks) == (1, 1) and not forcing_dim:
        return _tiny()
    torch.manual_seed(3)
    return ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, forcing_dim=forcing_dim, embedding_dim=64,
                     hidden_channels=list(hidden_channels or [32, 64]), hidden_blocks=list(hidden_blocks), attention_levels=list(attention_levels),
                     kernel_size=3, padding_mode="zeros")


def _module_step(net, precision, want_dx=False, t=None, forcing=None):
    x, tt, eps = _inputs()
    net.precision = precision
    x = x.requires_grad_(want_dx)
    y = net(x, tt if t is None else t, forcing=forcing) if forcing is not None else net(x, tt if t is None else t)
    ((y - eps) ** 2).mean().backward()


def _trainer_step(monkeypatch, net, precision, chain=None, **kw):
    x, t, eps = _inputs()
    tr = Trainer(net, lr=1e-3, precision=precision, ema_rates=[0.9], **kw)
    if chain is not None:
        tr.eng.chain_blocks = True  # the engine's opt-in; the doubles' CHAIN switch stands for the kernels' existence
        monkeypatch.setattr(emu_ops, "CHAIN", chain)
    tr.step(x, t=t, eps=eps)


def _engine_step(net, dt, x, loss=False):
    """Engine.forward with a noise SEED (what a trainer on the GPU passes), then the backward of what it returned."""
    eng = net._get_engine()
    eng.ensure_grad_buffer()
    B = x.shape[0]
    musig = torch.empty((B, 2), dtype=torch.float32)
    c2w_ops.mu_sigma(_inputs()[1], musig, B, 1e-3)
    tape = Tape()
    lf = dict(sum=torch.zeros(1), gscale=0.5, scaler=None) if loss else None
    y = eng.forward(x, _inputs()[1], dt, tape=tape, noise=(1234, musig), nhwc_out=True, loss=lf)
    eng.backward(tape, torch.ones_like(y))
    return tape.meta.get("loss_fused")


def _window_batch():
    data = torch.randn(5, 2, 16, 16, generator=torch.Generator().manual_seed(4))
    return WindowBatch(data, torch.tensor([0, 2]), 3)


def _pass_inference_fp32(mp):
    with torch.no_grad():
        x, t, _ = _inputs()
        _net().eval()(x, t)


def _pass_inference_bf16_one_t(mp):
    net = _net([64, 64]).eval()
    net.precision = "bf16"
    with torch.no_grad():
        net(_inputs()[0], torch.tensor(0.3))


def _pass_score_function_fold(mp):
    torch.manual_seed(5)
    net = ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, embedding_dim=32, hidden_channels=[64, 64], hidden_blocks=[1, 1],
                    attention_levels=[1], kernel_size=3, padding_mode="zeros").eval()
    sf = BatchedScoreFunction(net, markov_order=1, batch_size=3, device=torch.device("cpu"), noise_process=SDAPipeline())
    sf.score_fn(torch.randn(7, 2, 16, 16, generator=torch.Generator().manual_seed(9)), 0.6)


def _pass_frozen_input_gradient(mp):
    net = _net().eval().requires_grad_(False)
    _module_step(net, "fp32", want_dx=True)


def _pass_seed_fused_loss(mp):
    assert _engine_step(_net([64, 64]), c2w_ops.DTYPE_BF16, _window_batch(), loss=True) is True


def _pass_seed_not_fused_loss(mp):
    assert _engine_step(_net([64, 64]), c2w_ops.DTYPE_BF16, _inputs()[0], loss=True) is False


# name -> (installation keywords, body)
PASSES = {
    "inference_fp32_per_item_t": ({}, _pass_inference_fp32),
    "inference_bf16_one_t": ({}, _pass_inference_bf16_one_t),
    "train_fp32_want_dx": ({}, lambda mp: _module_step(_net(), "fp32", want_dx=True)),
    "train_bf16": ({}, lambda mp: _trainer_step(mp, _net([64, 64]), "bf16")),
    "train_fp16_chain": ({}, lambda mp: _trainer_step(mp, _net([64, 64], (3, 2), ()), "fp16", chain=True)),
    "train_bf16_chain_refused": ({}, lambda mp: _trainer_step(mp, _net([64, 64], (3, 2), ()), "bf16", chain=False)),
    "train_fp32_forcing": ({}, lambda mp: _module_step(_net(forcing_dim=5), "fp32", forcing=torch.linspace(-1, 1, 10).view(2, 5))),
    "train_bf16_deterministic": (dict(det=True), lambda mp: _trainer_step(mp, _net([64, 64]), "bf16", deterministic=True)),
    "train_fp32_deterministic_one_t": (dict(det=True), lambda mp: _module_step(_det(_net()), "fp32", t=torch.tensor(0.3))),
    "frozen_network_input_gradient": ({}, _pass_frozen_input_gradient),
    "score_function_fold": ({}, _pass_score_function_fold),
    # the input conversion's attempts, in order (a noise seed, as on the GPU)
    "seed_every_fused_conversion_refuses": ({}, lambda mp: _engine_step(_net(), c2w_ops.DTYPE_F32, _inputs()[0])),
    "seed_dense_conversion": (dict(accept=["nchw_to_nhwc_noise"]), lambda mp: _engine_step(_net(), c2w_ops.DTYPE_F32, _inputs()[0])),
    "seed_windows_in_place": (dict(accept=["windows_to_nhwc_noise"]), lambda mp: _engine_step(_net(), c2w_ops.DTYPE_F32, _window_batch())),
    "seed_windows_materialised": (dict(accept=["nchw_to_nhwc_noise"]), lambda mp: _engine_step(_net(), c2w_ops.DTYPE_F32, _window_batch())),
    "seed_fused_loss_rows": (dict(accept=["nchw_to_nhwc_noise_rows"], fused_loss=True), _pass_seed_fused_loss),
    "seed_fused_loss_rows_refused": (dict(accept=["nchw_to_nhwc_noise"], fused_loss=True), _pass_seed_not_fused_loss),
}


def _det(net):
    net.deterministic = True
    return net


def _trace(monkeypatch, name):
    kw, body = PASSES[name]
    log = []
    _install(monkeypatch, log, **kw)
    body(monkeypatch)
    return log


@pytest.mark.parametrize("name", list(PASSES))
def test_launch_order_is_the_recorded_one(monkeypatch, name):
    got = _trace(monkeypatch, name)
    if os.environ.get("C2W_RECORD_LAUNCH_ORDER") == "1":
        traces = json.load(open(TRACES)) if os.path.exists(TRACES) else {}
        traces[name] = got
        with open(TRACES, "w") as f:
            f.write("{\n" + ",\n".join(json.dumps(k) + ": [\n" + ",\n".join(json.dumps(c) for c in v) + "\n]" for k, v in traces.items()) + "\n}\n")
        return
    want = json.load(open(TRACES))[name]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, "call %d differs\n  now:      %s\n  recorded: %s" % (i, a, b)
    assert len(got) == len(want), "%d calls now, %d recorded; first extra / missing: %s" % (
        len(got), len(want), (got + want)[min(len(got), len(want))] if len(got) > len(want) else want[len(got)])
