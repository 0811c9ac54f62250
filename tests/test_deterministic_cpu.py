"""CPU checks of the deterministic mode's host side (Engine.deterministic, Trainer(deterministic=True), ScoreUNet.deterministic): the
scratch wiring and the launch sequence with the HIP launchers replaced by tests/emu_det_ops.py (a layer over tests/emu_ops.py), that
the default engine touches nothing new, and the ctypes mirror of C2wConvArgs against the C struct.  The kernels themselves are
checked on the GPU (tests/test_gpu_deterministic.py)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import emu_det_ops
import emu_ops
from climate2weather_amd import _lib
from climate2weather_amd import ops as c2w_ops
from climate2weather_amd.score import ScoreUNet
from climate2weather_amd.training import Trainer

TINY = dict(embedding_dim=64, hidden_channels=[32, 64], hidden_blocks=[1, 1], attention_levels=[1], kernel_size=3,
            padding_mode="zeros")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(golden_dir, name):
    return {k: v for k, v in np.load(os.path.join(golden_dir, name), allow_pickle=False).items()}


def _tiny(forcing_dim=0, **over):
    torch.manual_seed(3)
    return ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, forcing_dim=forcing_dim, **dict(TINY, **over))


def _close(a, b, what):
    # the two modes differ in the summation order of fp32 sums only
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-6 + 1e-5 * b.abs().max().item()), (what, (a - b).abs().max().item())


def _module_grads(net, x, t, eps, forcing):
    net.zero_grad(set_to_none=True)
    y = net(x, t, forcing=forcing) if forcing is not None else net(x, t)
    loss = ((y - eps) ** 2).mean()
    loss.backward()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in net.named_parameters()}


@pytest.mark.parametrize("case", ["per_item_t", "scalar_t", "forcing"])
def test_module_path_gives_the_default_engines_gradients(monkeypatch, golden_dir, case):
    g = _golden(golden_dir, "tiny_net_forcing.npz" if case == "forcing" else "tiny_net.npz")
    x, t, eps = (torch.from_numpy(g[k]) for k in ("x", "t", "eps"))
    forcing = torch.from_numpy(g["forcing"]) if case == "forcing" else None
    if case == "scalar_t":  # one t for the whole batch: the modulation gradient is ONE shared row (ldm == 0)
        t = torch.tensor(0.3)
    fd = 5 if case == "forcing" else 0
    emu_det_ops.install(monkeypatch, c2w_ops)
    ref_loss, ref = _module_grads(_tiny(fd), x, t, eps, forcing)
    assert emu_det_ops.LOG == []  # mode off: nothing went through a scratch
    net = _tiny(fd)
    net.deterministic = True
    loss, got = _module_grads(net, x, t, eps, forcing)
    assert net._get_engine().deterministic is True
    _close(loss, ref_loss, "loss")
    assert set(got) == set(ref)
    for n in ref:
        _close(got[n], ref[n], n)
    sites = {s for s, _ in emu_det_ops.LOG}
    assert "conv_wgrad" in sites and ({"conv_ln", "ln_backward"} & sites), sites
    # every bias gradient of the step was reduced: one reduce per layer record (the blocks' modulation projections are ONE record)
    assert sum(1 for s, _ in emu_det_ops.LOG if s == "conv_wgrad") == len(net._get_engine().layout.convs)
    # a second backward accumulates on top (p.grad += ...), through the same scratch
    y = net(x, t, forcing=forcing) if forcing is not None else net(x, t)
    ((y - eps) ** 2).mean().backward()
    for n, p in net.named_parameters():
        _close(p.grad, 2 * ref[n], n + " (accumulated)")


def test_trainer_two_accumulation_rounds_match_the_default_trainer(monkeypatch, golden_dir):
    g = _golden(golden_dir, "tiny_net.npz")
    x = torch.from_numpy(g["x"])
    rounds = [x[:1].contiguous(), x[1:].contiguous()]
    emu_det_ops.install(monkeypatch, c2w_ops)
    out = {}
    for det in (False, True):
        torch.manual_seed(0)
        del emu_det_ops.LOG[:]
        tr = Trainer(_tiny(), lr=0.0, precision="fp32", ema_rates=[], deterministic=det)
        assert tr.eng.deterministic is det
        loss = tr.step(rounds)
        out[det] = (float(loss), tr.eng.flat_grad.clone(), list(emu_det_ops.LOG))
        if det:  # the scratch buffers are sized during the first step and kept
            ptrs = {k: v.data_ptr() for k, v in tr.eng._det_ws.items()}, {k: v.data_ptr() for k, v in tr.eng._ws.items()}
            torch.manual_seed(0)
            tr.step(rounds)
            assert ptrs == ({k: v.data_ptr() for k, v in tr.eng._det_ws.items()}, {k: v.data_ptr() for k, v in tr.eng._ws.items()})
    assert out[False][2] == []
    sites = [s for s, _ in out[True][2]]
    assert sites.count("mse_loss_grad") == 2  # one loss reduce per round
    assert "conv_wgrad" in sites
    assert out[True][0] == pytest.approx(out[False][0], rel=1e-5)
    _close(out[True][1], out[False][1], "flat gradient of two rounds")


def test_fp16_loss_scale_step_in_deterministic_mode(monkeypatch):
    emu_det_ops.install(monkeypatch, c2w_ops)
    x = torch.randn(2, 6, 16, 16, generator=torch.Generator().manual_seed(1))
    t = torch.tensor([0.3, 0.7])
    eps = torch.randn(2, 6, 16, 16, generator=torch.Generator().manual_seed(2))
    losses, params = [], []
    for det in (False, True):
        net = _tiny(hidden_channels=[64, 64])  # 16-bit modes: channel counts in whole 128-byte K chunks
        tr = Trainer(net, lr=1e-3, precision="fp16", ema_rates=[0.9], init_scale=256.0, growth_interval=2, deterministic=det)
        losses.append(float(tr.step(x, t=t, eps=eps)))
        assert tr.loss_scale() == 256.0 and tr.optimizer_steps_taken() == 1
        params.append(tr.eng.flat.clone())
    assert losses[1] == pytest.approx(losses[0], rel=1e-4)
    assert (params[1] - params[0]).abs().max().item() <= 2e-3  # one AdamW step of lr 1e-3 from the same weights


def test_default_engine_calls_nothing_new(monkeypatch, golden_dir):
    """Mode off: the engine runs on tests/emu_ops.py alone -- whose launchers know none of the new keyword arguments -- with every new
    ops attribute deleted."""
    emu_ops.install(monkeypatch, c2w_ops)
    for name in emu_det_ops.NEW_NAMES + ["_nbytes"]:
        monkeypatch.delattr(c2w_ops, name)
    monkeypatch.delenv("C2W_DETERMINISTIC", raising=False)
    g = _golden(golden_dir, "tiny_net.npz")
    x, t, eps = (torch.from_numpy(g[k]) for k in ("x", "t", "eps"))
    net = _tiny()
    assert net._get_engine().deterministic is False
    _, grads = _module_grads(net, x, t, eps, None)
    assert all(torch.isfinite(v).all() for v in grads.values())
    tr = Trainer(_tiny(), lr=1e-3, precision="fp32", ema_rates=[0.9])
    assert tr.eng.deterministic is False and tr.eng._det_ws == {}
    assert float(tr.step(x, t=t.reshape(-1), eps=eps)) == pytest.approx(float(g["loss"]), rel=1e-5)
    assert tr.eng._det_ws == {} and tr.eng._det_need == {}


def test_environment_sets_the_host_default(monkeypatch):
    emu_ops.install(monkeypatch, c2w_ops)
    monkeypatch.setenv("C2W_DETERMINISTIC", "1")
    assert _tiny()._get_engine().deterministic is True
    net = _tiny()
    net.deterministic = False  # the module's own switch wins over the environment
    assert net._get_engine().deterministic is False
    monkeypatch.setenv("C2W_DETERMINISTIC", "0")
    assert _tiny()._get_engine().deterministic is False
    assert Trainer(_tiny(), precision="fp32", ema_rates=[], deterministic=True).eng.deterministic is True


def _host_compiler():
    for cand in (os.environ.get("CC"), "cc", "gcc", "clang"):
        if cand and shutil.which(cand):
            return [shutil.which(cand), "-x", "c"]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # what the library itself is built with; host-only C++ here
    assert os.path.exists(hipcc), "no host compiler found (cc / gcc / clang / hipcc)"
    return [hipcc, "-x", "c++"]


def test_ctypes_conv_args_mirror_the_c_struct(tmp_path):
    fields = [n for n, _ in _lib.ConvArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "c2w_hip.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(C2wConvArgs));\n'
                   + "".join(f'    printf("{f} %zu\\n", offsetof(C2wConvArgs, {f}));\n' for f in fields)
                   + '    printf("flag %d\\n", (int)C2W_CONV_DETERMINISTIC);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(_host_compiler() + ["-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=30).stdout.splitlines())
    assert int(out.pop("sizeof")) == ctypes.sizeof(_lib.ConvArgs)
    assert int(out.pop("flag")) == _lib.CONV_DETERMINISTIC == 8
    assert {f: int(v) for f, v in out.items()} == {f: getattr(_lib.ConvArgs, f).offset for f in fields}
    assert fields[-2:] == ["det_ws", "det_ws_bytes"]  # the new fields sit at the end: every older field keeps its offset
