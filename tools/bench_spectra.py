#!/usr/bin/env python3
"""Throughput of the spectrum kernel (csrc/spectrum.hip) against the vendor-FFT route, in one process, with device events.

    python tools/bench_spectra.py            (FIELDS=16384 ROUNDS=5 ITERS=10; OUT=path also writes the JSON there)

Timed, alternately, ROUNDS blocks of ITERS calls each, on FIELDS = 8 x 512 x 4 fields of 128 x 128 (1 GiB, four times the Infinity Cache):
  kernel        ops.rapsd, one launch
  fft_general   spectra._rapsd_general: the package's own general route (full fft2 in chunks, float64 dense binning)
  fft_lean      what a careful user writes: rfft2 in chunks, power, one fp32 dense product with the half-plane bin table
  read          torch's sum over the same tensor: the HBM read rate of this box, against which the kernel's input rate is a share
and the kernel alone on the same number of 8 x 8 fields.  Input bytes = FIELDS * N * N * 4; a route's GB/s is input bytes over its time,
whatever else it moves.  One JSON line per route, then a summary."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from climate2weather_amd import ops, spectra

FIELDS, ROUNDS, ITERS = int(os.environ.get("FIELDS", "16384")), int(os.environ.get("ROUNDS", "5")), int(os.environ.get("ITERS", "10"))
dev = torch.device("cuda:0")


def half_plane_table(N):
    """(N * (N/2 + 1), N/2) fp32: rfft2 cell -> bin mean weights (kv = 0 once, kv >= 1 twice; Nyquist row and column in no bin)"""
    bins = spectra.cell_bins(N, N)[:, :N // 2 + 1].copy()
    bins[N // 2, :] = -1
    bins[:, N // 2] = -1
    w = np.where(np.arange(N // 2 + 1) == 0, 1.0, 2.0)[None, :] * np.ones((N, 1))
    t = np.zeros((N * (N // 2 + 1), N // 2))
    keep = bins.reshape(-1) >= 0
    t[np.nonzero(keep)[0], bins.reshape(-1)[keep]] = w.reshape(-1)[keep]
    return torch.from_numpy((t / t.sum(0, keepdims=True)).astype(np.float32)).to(dev)


def fft_lean(x, out, table, chunk=2048):
    N = x.shape[-1]
    for i in range(0, x.shape[0], chunk):
        c = x[i:i + chunk]
        z = torch.fft.rfft2(c - c.mean(dim=(-2, -1), keepdim=True))
        p = (z.real ** 2 + z.imag ** 2).reshape(c.shape[0], -1) * (1.0 / (N * N))
        torch.matmul(p, table, out=out[i:i + chunk])


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    torch.manual_seed(0)
    N = 128
    x = torch.randn(FIELDS, N, N, device=dev) + 0.5
    spec = torch.empty(FIELDS, N // 2, device=dev)
    table = half_plane_table(N)
    x8 = torch.randn(FIELDS, 8, 8, device=dev) + 0.5
    spec8 = torch.empty(FIELDS, 4, device=dev)
    routes = {
        "kernel": lambda: ops.rapsd(x, spec, FIELDS, N, N),
        "fft_general": lambda: spectra._rapsd_general(x, spec),
        "fft_lean": lambda: fft_lean(x, spec, table),
        "read": lambda: x.sum(),
        "kernel_8x8": lambda: ops.rapsd(x8, spec8, FIELDS, 8, 8),
    }
    # the routes agree before they are timed
    ops.rapsd(x, spec, FIELDS, N, N)
    a = spec[:256].clone()
    fft_lean(x[:256], spec[:256], table)
    agree = float(((spec[:256, 1:].double() / a[:, 1:].double()).log().abs()).max())  # bin 0 is the mean, which fft_lean takes off
    for name, fn in routes.items():  # warm-up: code objects, FFT plans, allocator
        timed(fn, 2)
    ms = {k: [] for k in routes}
    for _ in range(ROUNDS):
        for name, fn in routes.items():
            ms[name].append(timed(fn, ITERS if name != "fft_general" else max(1, ITERS // 5)))
    result = {"fields": FIELDS, "rounds": ROUNDS, "iters": ITERS, "max_log_ratio_kernel_vs_fft_lean": agree, "routes": {}}
    read_gbs = x.numel() * 4 / (statistics.median(ms["read"]) * 1e-3) / 1e9
    for name in routes:
        n = 8 if name == "kernel_8x8" else N
        med = statistics.median(ms[name])
        gbs = FIELDS * n * n * 4 / (med * 1e-3) / 1e9
        r = dict(route=name, N=n, ms_median=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                 fields_per_s=round(FIELDS / (med * 1e-3)), input_GBps=round(gbs, 1), share_of_measured_read=round(gbs / read_gbs, 3))
        result["routes"][name] = r
        print(json.dumps(r), flush=True)
    k, l = result["routes"]["kernel"]["ms_median"], result["routes"]["fft_lean"]["ms_median"]
    print(f"kernel {k:.3f} ms vs fft_lean {l:.3f} ms: {l / k:.2f} x; measured read rate {read_gbs:.0f} GB/s; kernel vs fft_lean max |log ratio| {agree:.2e}")
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
