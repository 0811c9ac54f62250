#!/usr/bin/env python3
"""Throughput of the CRPS kernel (csrc/crps.hip) against the torch routes, in one process, with device events.

    python tools/bench_crps.py            (CONFIGS="8x256,64x32" VARS=4 ROUNDS=3 ITERS=20; OUT=path also writes the JSON there)

For every MEMBERSxTIMES of CONFIGS, on MEMBERS x TIMES x VARS fields of 128 x 128 against TIMES x VARS truth fields (the defaults are
two ensembles of the same 537 MB), timed alternately in ROUNDS blocks of ITERS calls each:
  kernel        ops.crps_terms without the per-cell output: crps_terms_kernel and, a plane being four chunks, the shared fold_parts_kernel;
                its bytes are the samples and the truth, each read once
  kernel_cells  the same with the (4, T, F, hw) per-cell output written
  torch_fp32    the same four sums through torch in fp32: torch.sort(dim=0), the gaps times the weights, the pivoted moments, the
                reductions over a plane in float64
  general       crps._general: the package's own float64 route, chunked over the times (one call per round)
  read          torch's sum over the samples: the HBM read rate of this box, against which the kernel's input rate is a share
One JSON line per route, then a summary line per configuration."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from climate2weather_amd import crps as C
from climate2weather_amd import ops

CONFIGS = [tuple(int(v) for v in c.split("x")) for c in os.environ.get("CONFIGS", "8x256,64x32").split(",")]
F = int(os.environ.get("VARS", "4"))
ROUNDS, ITERS = int(os.environ.get("ROUNDS", "3")), int(os.environ.get("ITERS", "20"))
H = W = 128
dev = torch.device("cuda:0")


def torch_fp32(x, y, sums):
    """x (M, T, F, hw), y (T, F, hw) -> sums (T, F, 4): the kernel's algebra as whole-tensor fp32 torch operations"""
    M = x.shape[0]
    s = torch.sort(x, dim=0).values
    k = torch.arange(1, M, dtype=torch.float32, device=x.device)
    a = (s - y[None]).abs().sum(dim=0) / M
    b = ((k * (M - k))[:, None, None, None] * (s[1:] - s[:-1])).sum(dim=0) if M > 1 else torch.zeros_like(y)
    e = s - s[M // 2][None]
    ebar = e.sum(dim=0) / M
    v = ((e - ebar[None]) ** 2).sum(dim=0) / max(M - 1, 1)
    t = (s[M // 2] - y) + ebar
    for i, term in enumerate((a, b, t * t, v)):
        sums[..., i] = term.sum(dim=-1, dtype=torch.float64)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def one(M, T):
    torch.manual_seed(0)
    hw = H * W
    off = torch.tensor([101325.0, 280.0, 0.0, 3.0], device=dev)[:F] if F <= 4 else torch.zeros(F, device=dev)
    sd = torch.tensor([1200.0, 10.0, 4.0, 4.0], device=dev)[:F] if F <= 4 else torch.ones(F, device=dev)
    centre = off[None, :, None] + sd[None, :, None] * torch.randn(T, F, hw, device=dev)
    y = (centre + 0.01 * sd[None, :, None] * torch.randn(T, F, hw, device=dev)).contiguous()
    x = (centre[None] + 0.01 * sd[None, None, :, None] * torch.randn(M, T, F, hw, device=dev)).contiguous()
    del centre
    nbytes = ops.crps_scratch_bytes(T, F, hw)
    scratch = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=dev)
    sums, sums_c, sums32, sums64 = (torch.empty(T, F, 4, dtype=torch.float64, device=dev) for _ in range(4))
    cells = torch.empty(4, T, F, hw, dtype=torch.float32, device=dev)

    def kernel():
        assert ops.crps_terms(x, y, sums, None, scratch, M, T, F, hw)

    def kernel_cells():
        assert ops.crps_terms(x, y, sums_c, cells, scratch, M, T, F, hw)

    routes = {"kernel": kernel, "kernel_cells": kernel_cells, "torch_fp32": lambda: torch_fp32(x, y, sums32),
              "general": lambda: C._general(x, y, sums64, None), "read": lambda: x.sum()}
    slow = ("general",)
    ms = {k: [] for k in routes}
    for name, fn in routes.items():  # warm-up: code objects, allocator; the warm-up call is the agreement run too
        timed(fn, 1 if name in slow else 2)
    agree32 = float(((sums - sums32).abs() / sums64.abs()).max())
    agree64 = float(((sums - sums64).abs() / sums64.abs()).max())
    torch32_vs64 = float(((sums32 - sums64).abs() / sums64.abs()).max())
    same = bool(torch.equal(sums.nan_to_num(nan=-1.0), sums_c.nan_to_num(nan=-1.0)))  # M = 1: the sums of V are NaN on both sides
    for _ in range(ROUNDS):
        for name, fn in routes.items():
            if name in slow and ms[name]:
                continue  # one timed call: seconds
            ms[name].append(timed(fn, 1 if name in slow else ITERS))
    in_bytes = (M + 1) * T * F * hw * 4
    read_gbs = x.numel() * 4 / (statistics.median(ms["read"]) * 1e-3) / 1e9
    result = {"members": M, "times": T, "vars": F, "hw": hw, "input_bytes": in_bytes, "rounds": ROUNDS, "iters": ITERS,
              "max_rel_kernel_vs_torch_fp32": agree32, "max_rel_kernel_vs_general": agree64, "max_rel_torch_fp32_vs_general": torch32_vs64,
              "sums_equal_with_and_without_cells": same, "measured_read_GBps": round(read_gbs, 1), "routes": {}}
    for name in routes:
        med = statistics.median(ms[name])
        r = dict(members=M, times=T, route=name, ms_median=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4))
        gbs = (x.numel() * 4 if name == "read" else in_bytes) / (med * 1e-3) / 1e9
        r.update(input_GBps=round(gbs, 1), share_of_measured_read=round(gbs / read_gbs, 3))
        if name in ("kernel", "kernel_cells"):
            r.update(cells_per_s=float(f"{T * F * hw / (med * 1e-3):.4g}"))
        result["routes"][name] = r
        print(json.dumps(r), flush=True)
    k, kc, t32, g = (result["routes"][r]["ms_median"] for r in ("kernel", "kernel_cells", "torch_fp32", "general"))
    print(f"M {M} T {T}: kernel {k:.3f} ms ({result['routes']['kernel']['input_GBps']:.0f} GB/s of input, "
          f"{result['routes']['kernel']['share_of_measured_read']:.2f} of the measured read rate {read_gbs:.0f} GB/s), with cells {kc:.3f} ms; "
          f"torch_fp32 {t32:.3f} ms ({t32 / k:.2f} x), general {g:.3f} ms ({g / k:.2f} x); sums: kernel vs torch_fp32 {agree32:.2e}, vs general "
          f"{agree64:.2e}, torch_fp32 vs general {torch32_vs64:.2e} relative; equal with and without cells {same}", flush=True)
    return result


def main():
    results = [one(M, T) for M, T in CONFIGS]
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
