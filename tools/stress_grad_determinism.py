#!/usr/bin/env python3
"""Does every backward pass of the full-size network give the same bits in deterministic mode?  The default net at C = 52, B = 2, fp16 and
bf16, Trainer(deterministic=True), fixed operands (batch, t, noise, weights), N backward passes on one stream and with the weight
gradients on a second one: after every pass all 228 gradient tensors and the loss are compared with pass 0 (torch.equal).  On the
first mismatch the two tensors and the pass's launch order are saved under --out and the run stops; in this mode any differing bit is
a bug.  It compares values only.
    python tools/stress_grad_determinism.py [N=200] [--out stress_grad_determinism_out]"""
import argparse
import os
import sys

sys.path.insert(0, os.getcwd())
import torch

from climate2weather_amd import ops
from climate2weather_amd.score import ScoreUNet
from climate2weather_amd.training import Trainer

DEFAULT = dict(embedding_dim=512, hidden_blocks=[3] * 5, hidden_channels=[128, 128, 256, 384, 512], kernel_size=3, padding_mode="zeros",
               attention_levels=[4])
LAUNCHERS = ["conv", "conv_wgrad", "conv_wgrad_grouped", "ln_forward", "ln_backward", "mse_loss_grad", "mse_loss_grad_noise", "attention_forward",
             "attention_backward", "sumpool2", "upsample2", "nchw_to_nhwc", "nchw_to_nhwc_noise", "nchw_to_nhwc_noise_rows", "weight_transpose_batched"]


class LaunchLog:
    """names (and, for convs, geometry) of the ops.* calls of one pass, in order"""

    def __init__(self):
        self.cur, self.real = [], {}

    def install(self):
        for name in LAUNCHERS:
            fn = getattr(ops, name)
            self.real[name] = fn

            def wrapped(*a, _fn=fn, _name=name, **kw):
                g = next((v for v in list(a) + list(kw.values()) if isinstance(v, dict) and "Hout" in v), None)
                self.cur.append(_name if g is None else f"{_name} B={g['B']} {g['Cin']}->{g['Cout']} @{g['Hout']}x{g['Wout']} mode={g['mode']}")
                return _fn(*a, **kw)
            setattr(ops, name, wrapped)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("passes", nargs="?", type=int, default=200)
    ap.add_argument("--out", default="stress_grad_determinism_out")
    a = ap.parse_args()
    log = LaunchLog()
    log.install()
    B, C, H = 2, 52, 128
    bad = 0
    for precision in ("fp16", "bf16"):
        for grad_stream in (False, True):
            torch.manual_seed(0)
            net = ScoreUNet(channels=C, spatial=2, activation=torch.nn.SiLU, **DEFAULT).cuda()
            gen = torch.Generator().manual_seed(128)
            x = (torch.randn(B, C, H, H, generator=gen) * 0.5 + 0.5).cuda()
            t = torch.rand(B, generator=gen).cuda()
            eps = torch.randn(B, C, H, H, generator=gen).cuda()
            tr = Trainer(net, precision=precision, ema_rates=(), deterministic=True)
            tr.eng.use_grad_stream = grad_stream
            views = tr.eng.layout.views
            assert len(views) == 228
            ref = first_order = None
            what = f"{precision}, weight gradients on {'a second stream' if grad_stream else 'the same stream'}"
            for p in range(a.passes):
                tr.eng.flat_grad.zero_()
                log.cur = []
                loss = tr._forward_backward(x, t, eps, sync=False)
                torch.cuda.synchronize()
                cur = {n: tr.eng.flat_grad[off:off + int(torch.tensor(shape).prod())].clone() for n, (off, shape, _) in views.items()}
                cur["<loss>"] = loss.detach().reshape(1).clone()
                if ref is None:
                    ref, first_order = cur, list(log.cur)
                    continue
                diff = [n for n in cur if not torch.equal(cur[n], ref[n])]
                if diff:
                    os.makedirs(a.out, exist_ok=True)
                    n = diff[0]
                    tag = f"{precision}_{'two' if grad_stream else 'one'}_stream_pass{p}"
                    torch.save(dict(name=n, pass0=ref[n].cpu(), this_pass=cur[n].cpu(), differing=diff, launch_order_pass0=first_order,
                                    launch_order_this_pass=list(log.cur)), os.path.join(a.out, tag + ".pt"))
                    nd = int((cur[n] != ref[n]).sum())
                    print(f"{what}: MISMATCH at pass {p}: {len(diff)} of 229 tensors differ from pass 0, first {n} ({nd} of {cur[n].numel()} elements); "
                          f"saved {tag}.pt under {a.out}", flush=True)
                    bad += 1
                    break
            else:
                print(f"{what}: {a.passes} backward passes, all 228 gradient tensors and the loss bit-identical to pass 0 "
                      f"({len(first_order)} launches per pass)", flush=True)
            del tr, net
            torch.cuda.empty_cache()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
