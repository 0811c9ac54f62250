#!/usr/bin/env python3
"""Throughput of the temporal-increment kernel (csrc/temporal.hip) against the torch routes, in one process, with device events.

    python tools/bench_temporal.py     (SHAPES="8x256,64x32" LAGS="6,24" VARS=4 ROUNDS=3 ITERS=10; OUT=path also writes the JSON there)

Fields of 128 x 128, with a truth.  For every MEMBERSxTIMES of SHAPES (the defaults are ensembles of the same 537 MB) and every lag
count of LAGS, timed alternately in ROUNDS blocks:
  kernel      temporal_ops.tincr_terms: the terms kernel and its fold kernel; its bytes are the samples and the truth, counted once
              (the kernel reads a plane up to L + 1 times: what the re-reads cost shows in the share below)
  torch_fp32  the same table through torch in fp32: per lag ``rows[:, tau:] - rows[:, :-tau]``, abs / square, the sums over the cells
              in float64
  general     temporal._general: the package's own float64 route, chunked over the times (one call)
  read        torch's sum over the samples and the truth: the read rate of this box on the same bytes, against which the kernel's input
              rate is a share
The calls are back to back on the same tensors, so the caches are as warm as they get.  One JSON line per route, then a summary line per
configuration."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from climate2weather_amd import temporal as TP
from climate2weather_amd import temporal_ops

SHAPES = [tuple(int(v) for v in c.split("x")) for c in os.environ.get("SHAPES", "8x256,64x32").split(",") if c]
LAGS = [int(v) for v in os.environ.get("LAGS", "6,24").split(",") if v]
F = int(os.environ.get("VARS", "4"))
ROUNDS, ITERS = int(os.environ.get("ROUNDS", "3")), int(os.environ.get("ITERS", "10"))
H = W = 128
dev = torch.device("cuda:0")


def terms_fp32(x, y, S, L):
    """x (M, T, F, hw), y (T, F, hw) -> S (M + 1, T, F, L, 3): one sliced pass per lag in fp32, the sums over a plane in float64"""
    rows = torch.cat([y[None], x])
    T = rows.shape[1]
    S.zero_()
    for tau in range(1, min(L, T - 1) + 1):
        dx = rows[:, tau:] - rows[:, :-tau]
        e = dx - dx[:1]
        S[:, :T - tau, :, tau - 1, 0] = dx.abs().sum(dim=-1, dtype=torch.float64)
        S[:, :T - tau, :, tau - 1, 1] = (dx * dx).sum(dim=-1, dtype=torch.float64)
        S[:, :T - tau, :, tau - 1, 2] = (e * e).sum(dim=-1, dtype=torch.float64)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def fields(M, T):
    """series in time: every row a random walk of its own around a shared start, de-normalised"""
    torch.manual_seed(0)
    off = torch.tensor([101325.0, 280.0, 0.0, 3.0], device=dev)[:F] if F <= 4 else torch.zeros(F, device=dev)
    sd = torch.tensor([1200.0, 10.0, 4.0, 4.0], device=dev)[:F] if F <= 4 else torch.ones(F, device=dev)
    start = off[None, :, None, None] + sd[None, :, None, None] * torch.randn(1, F, H, W, device=dev)
    y = (start + 0.05 * sd[None, :, None, None] * torch.cumsum(torch.randn(T, F, H, W, device=dev), dim=0)).contiguous()
    x = torch.empty(M, T, F, H, W, device=dev)
    for m in range(M):
        x[m] = start + 0.05 * sd[None, :, None, None] * torch.cumsum(torch.randn(T, F, H, W, device=dev), dim=0)
    return x, y


def one(M, T, L, x, y):
    hw = H * W
    xf, yf = x.view(M, T, F, hw), y.view(T, F, hw)
    nbytes = temporal_ops.tincr_scratch_bytes(M + 1, T, F, hw, L)
    scratch = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=dev)
    outs = {k: torch.empty(M + 1, T, F, L, 3, dtype=torch.float64, device=dev) for k in ("kernel", "torch_fp32", "general")}

    def kernel():
        assert temporal_ops.tincr_terms(xf, yf, outs["kernel"], scratch, M, T, F, hw, L)

    def read():
        x.sum()
        y.sum()

    routes = {"kernel": kernel, "torch_fp32": lambda: terms_fp32(xf, yf, outs["torch_fp32"], L),
              "general": lambda: TP._general(xf, yf, outs["general"], L), "read": read}
    iters = {"general": 1, "torch_fp32": max(1, ITERS // 5)}
    ms = {k: [] for k in routes}
    for name, fn in routes.items():  # warm-up: code objects, allocator; the warm-up call is the agreement run too
        timed(fn, 1)
    ref = outs["general"]
    scale = ref.abs().clamp_min(1e-300)
    agree = {k: float(((outs[k] - ref).abs() / scale)[..., :2].max()) for k in ("kernel", "torch_fp32")}  # A1, A2: relative rules
    for _ in range(ROUNDS):
        for name, fn in routes.items():
            if name == "general" and ms[name]:
                continue  # one timed call: seconds
            ms[name].append(timed(fn, iters.get(name, ITERS)))
    in_bytes = (M + 1) * T * F * hw * 4
    read_gbs = in_bytes / (statistics.median(ms["read"]) * 1e-3) / 1e9
    tag = f"{M}x{T} L={L}"
    result = dict(config=tag, members=M, times=T, vars=F, lags=L, input_bytes=in_bytes, max_rel_kernel_vs_general=agree["kernel"],
                  max_rel_torch_fp32_vs_general=agree["torch_fp32"], measured_read_GBps=round(read_gbs, 1), routes={})
    for name in routes:
        med = statistics.median(ms[name])
        gbs = in_bytes / (med * 1e-3) / 1e9
        r = dict(config=tag, route=name, ms_median=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                 input_GBps=round(gbs, 1), share_of_measured_read=round(gbs / read_gbs, 3))
        result["routes"][name] = r
        print(json.dumps(r), flush=True)
    k, t32, g = (result["routes"][r]["ms_median"] for r in ("kernel", "torch_fp32", "general"))
    print(f"temporal {tag}: kernel {k:.3f} ms ({result['routes']['kernel']['input_GBps']:.0f} GB/s of input, "
          f"{result['routes']['kernel']['share_of_measured_read']:.3f} of the measured read rate {read_gbs:.0f} GB/s); torch_fp32 {t32:.3f} ms "
          f"({t32 / k:.2f} x), general {g:.3f} ms ({g / k:.2f} x); A1 and A2 against general: kernel {agree['kernel']:.2e}, "
          f"torch_fp32 {agree['torch_fp32']:.2e} relative", flush=True)
    return result


def main():
    results = []
    for M, T in SHAPES:
        x, y = fields(M, T)
        results += [one(M, T, L, x, y) for L in LAGS]
        del x, y
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
