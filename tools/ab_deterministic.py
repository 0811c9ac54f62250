#!/usr/bin/env python3
"""What does the deterministic mode cost?  bench.py's headline step (default net, 65 channels, 128x128, bf16, B = 128, synthetic windows read
in place) timed with the mode off and on ALTERNATELY in one process -- same box, same clock -- on one trainer whose engine switch is
flipped between blocks.  Prints ms/step per block and the medians; the target of this work is <= 0.15 ms/step.
    python tools/ab_deterministic.py      (ROUNDS=4 STEPS=20 B=128 PRECISION=bf16; C2W_WGRAD_STREAM=1 for the two-stream step)"""
import gc
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from climate2weather_amd.data import DeviceWindowFeed, SyntheticWindowDataset
from climate2weather_amd.pipelines import SDAPipeline
from climate2weather_amd.score import ScoreUNet
from climate2weather_amd.training import Trainer

DEFAULT = dict(embedding_dim=512, hidden_blocks=[3] * 5, hidden_channels=[128, 128, 256, 384, 512], kernel_size=3, padding_mode="zeros",
               attention_levels=[4])
ROUNDS, STEPS, B = int(os.environ.get("ROUNDS", "4")), int(os.environ.get("STEPS", "20")), int(os.environ.get("B", "128"))
PRECISION = os.environ.get("PRECISION", "bf16")
ONLY = os.environ.get("ONLY")  # "off" / "on": one mode only (a profiler run of each)

dev = torch.device("cuda:0")
torch.manual_seed(0)
net = ScoreUNet(channels=65, spatial=2, activation=torch.nn.SiLU, **DEFAULT).to(dev)
tr = Trainer(net, SDAPipeline(), lr=1e-4, weight_decay=1e-3, ema_rates=[0.9999], precision=PRECISION, batch_size=B, seed=1000)
ds = SyntheticWindowDataset(n_frames=1024 + 12, n_vars=5, height=128, width=128, window=13, seed=0)
feed = DeviceWindowFeed(ds, dev, rank=0, num_replicas=1, seed=0)


def block(det: bool, steps: int) -> float:
    tr.eng.deterministic = det
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        tr.step(feed.next_batch(B, lazy=True))
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


modes = [m == "on" for m in ([ONLY] if ONLY else ["off", "on"])]
for det in modes:  # warm-up of both modes: scratch buffers, allocator, clocks
    block(det, 3)
gc.collect()
gc.disable()
ms = {False: [], True: []}
for r in range(ROUNDS):
    for det in modes:
        ms[det].append(block(det, STEPS))
        print(f"round {r}: deterministic {'on ' if det else 'off'} {ms[det][-1]:.3f} ms/step", flush=True)
gc.enable()
for det in modes:
    print(f"deterministic {'on ' if det else 'off'}: median {statistics.median(ms[det]):.3f} ms/step, min {min(ms[det]):.3f}, max {max(ms[det]):.3f}  "
          f"({PRECISION}, B = {B}, {'two streams' if tr.eng.use_grad_stream else 'one stream'})")
if len(modes) == 2:
    d = statistics.median(ms[True]) - statistics.median(ms[False])
    print(f"cost of the mode: {d:+.3f} ms/step (difference of the medians; target <= 0.15)")
