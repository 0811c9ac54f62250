#!/usr/bin/env python3
"""Throughput of the sliced-Wasserstein kernels (csrc/swd.hip) against the torch routes, in one process, with device events.

    python tools/bench_swd.py            (MEMBERS=8 TIMES=512 VARS=4 P=100 ROUNDS=5 ITERS=10; OUT=path also writes the JSON there)

Timed, alternately, ROUNDS blocks of ITERS calls each, on MEMBERS x TIMES x VARS = 16384 fields of 128 x 128 (1 GiB of samples, four
times the Infinity Cache) against TIMES x VARS truth fields, P = 100 unit directions:
  project       ops.swd_project over the samples, one launch: the fp32-input MFMA GEMM with the normalisation on the loaded value
  distance      ops.swd_distance over the MEMBERS x VARS x P column pairs, one launch
  kernels       what wasserstein.sliced_wasserstein enqueues: the projection of samples and truth in one launch, the distance
  torch_fp32    the same score through torch: x^ in fp32, torch.matmul, torch.sort, differences in float64
  general       wasserstein._general: the package's own float64 route
  read          torch's sum over the samples: the HBM read rate of this box, against which the projection's input rate is a share
and both kernels alone on the same number of 8 x 8 fields.  The projection's flop are the useful ones, 2 fields d P (the padding of P
to 128 is not counted), against the 157.3 TFLOP/s FP32-matrix figure of the MI355X; its input bytes are the samples, each field once.
One JSON line per route, then a summary."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from climate2weather_amd import ops
from climate2weather_amd import wasserstein as W

M, T, F = int(os.environ.get("MEMBERS", "8")), int(os.environ.get("TIMES", "512")), int(os.environ.get("VARS", "4"))
P = int(os.environ.get("P", "100"))
ROUNDS, ITERS = int(os.environ.get("ROUNDS", "5")), int(os.environ.get("ITERS", "10"))
FP32_MATRIX_TFLOPS = 157.3
dev = torch.device("cuda:0")


def torch_fp32(x, y, theta, shift, scale, out):
    """x (M, T, F, d), y (T, F, d): member by member, so that x^ costs one member's worth of memory"""
    s, c = shift[None, :, None], scale[None, :, None]
    b = torch.sort(torch.matmul((y - s) * c, theta.t()), dim=0).values.double()  # (T, F, P)
    for m in range(x.shape[0]):
        a = torch.sort(torch.matmul((x[m] - s) * c, theta.t()), dim=0).values.double()
        out[m] = ((a - b) ** 2).mean(dim=0)


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
    d, n = 128 * 128, M * T * F
    off = torch.tensor([101325.0, 280.0, 0.0, 3.0], device=dev)[:F] if F <= 4 else torch.zeros(F, device=dev)
    y = off[None, :, None] + 10.0 * torch.randn(T, F, d, device=dev)
    x = (y[None] + 3.0 * torch.randn(M, T, F, d, device=dev)).contiguous()
    shift, scale = W.truth_moments(y.view(T, F, 128, 128))
    theta = W.projections(d, P, 0, dev)
    px, py = torch.empty(M, F, P, T, device=dev), torch.empty(F, P, T, device=dev)
    out, out2 = torch.empty(M, F, P, dtype=torch.float64, device=dev), torch.empty(M, F, P, dtype=torch.float64, device=dev)
    d8 = 64
    y8 = torch.randn(T, F, d8, device=dev)
    x8 = (y8[None] + 0.3 * torch.randn(M, T, F, d8, device=dev)).contiguous()
    theta8 = W.projections(d8, P, 0, dev)
    zero, one = torch.zeros(F, device=dev), torch.ones(F, device=dev)
    px8 = torch.empty(M, F, P, T, device=dev)

    def kernels():
        assert ops.swd_project_pair(x, y, theta, shift, scale, px, py, M, T, F, d, P)
        assert ops.swd_distance(px, py, out, M, F, P, T)

    routes = {
        "project": lambda: ops.swd_project(x, theta, shift, scale, px, M, T, F, d, P),
        "distance": lambda: ops.swd_distance(px, py, out, M, F, P, T),
        "kernels": kernels,
        "torch_fp32": lambda: torch_fp32(x, y, theta, shift, scale, out2),
        "general": lambda: W._general(x, y, theta, shift, scale, out2),
        "read": lambda: x.sum(),
        "project_8x8": lambda: ops.swd_project(x8, theta8, zero, one, px8, M, T, F, d8, P),
        "distance_8x8": lambda: ops.swd_distance(px8, px8[0], out, M, F, P, T),
    }
    slow = ("torch_fp32", "general")
    # the routes agree before they are timed
    kernels()
    torch_fp32(x, y, theta, shift, scale, out2)
    swd_k, swd_t = torch.sqrt(out.mean(-1)), torch.sqrt(out2.mean(-1))
    agree = float(((swd_k - swd_t).abs() / swd_t).max())
    for name, fn in routes.items():  # warm-up: code objects, GEMM algorithms, allocator
        timed(fn, 1 if name in slow else 2)
    ms = {k: [] for k in routes}
    for _ in range(ROUNDS):
        for name, fn in routes.items():
            ms[name].append(timed(fn, 1 if name == "general" else max(1, ITERS // 5) if name in slow else ITERS))
    result = {"members": M, "times": T, "vars": F, "P": P, "rounds": ROUNDS, "iters": ITERS, "max_rel_kernels_vs_torch_fp32": agree, "routes": {}}
    read_gbs = x.numel() * 4 / (statistics.median(ms["read"]) * 1e-3) / 1e9
    for name in routes:
        dd = d8 if name.endswith("8x8") else d
        med = statistics.median(ms[name])
        r = dict(route=name, d=dd, ms_median=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4))
        if name not in ("distance", "distance_8x8"):
            nbytes = n * dd * 4 if name in ("read", "project", "project_8x8") else (n + T * F) * dd * 4
            gbs = nbytes / (med * 1e-3) / 1e9
            r.update(input_GBps=round(gbs, 1), share_of_measured_read=round(gbs / read_gbs, 3))
        if name in ("project", "project_8x8"):
            tf = 2.0 * n * dd * P / (med * 1e-3) / 1e12
            r.update(useful_TFLOPs=round(tf, 2), share_of_fp32_matrix_spec=round(tf / FP32_MATRIX_TFLOPS, 3))
        result["routes"][name] = r
        print(json.dumps(r), flush=True)
    k, t32, g = (result["routes"][r]["ms_median"] for r in ("kernels", "torch_fp32", "general"))
    print(f"kernels {k:.3f} ms vs torch_fp32 {t32:.3f} ms ({t32 / k:.2f} x) and general {g:.3f} ms ({g / k:.2f} x); measured read rate "
          f"{read_gbs:.0f} GB/s; kernels vs torch_fp32 max relative difference of the score {agree:.2e}")
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
