#!/usr/bin/env python3
"""Throughput of the wind-power kernel (csrc/wind.hip) against the torch routes, in one process, with device events.

    python tools/bench_wind.py            (CONFIGS="8x256x128,64x32x128,2x8x32" VARS=4 ROUNDS=3 ITERS=20; OUT=path also writes the JSON)

For every MEMBERSxTIMESxSIDE of CONFIGS, on MEMBERS x TIMES x VARS fields of SIDE x SIDE with the wind components in variables 2 and 3
and a 61-knot curve (0.5 m/s steps), timed alternately in ROUNDS blocks of ITERS calls each, back to back:
  kernel          wind_ops.wind_power without the per-cell output: wind_power_kernel and, where a plane has several chunks,
                  the shared fold_parts_kernel; its bytes are the u and the v planes, each read once (2 / VARS of the tensor)
  kernel_derived  the same with the (planes, 2, hw) per-cell speed and power written
  torch_fp32      the same two sums through torch in fp32: sqrt, bucketize, gather, the reductions over a plane in float64
  general         windpower._general: the package's own float64 route, chunked (one call per round)
  read            torch's sum over a dense copy of the two wind planes: the read rate this box reaches on the same bytes
and once, after a warm-up on a small shape, the whole wind_report of the first configuration (members, one more field set as the
truth, 300 grid points) next to the time of its KDE calls alone.  One JSON line per route, then a summary line per configuration."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from climate2weather_amd import marginals, wind_ops
from climate2weather_amd import windpower as W

CONFIGS = [tuple(int(v) for v in c.split("x")) for c in os.environ.get("CONFIGS", "8x256x128,64x32x128,2x8x32").split(",")]
F = int(os.environ.get("VARS", "4"))
ROUNDS, ITERS = int(os.environ.get("ROUNDS", "3")), int(os.environ.get("ITERS", "20"))
U, V = 2, 3
dev = torch.device("cuda:0")


def curve61():
    """0.5 m/s steps from a cut-in at 2 m/s, a cubic ramp to 12 m/s, a plateau: no turbine's numbers"""
    xs = 2.0 + 0.5 * np.arange(61)
    return W.PowerCurve(xs, 2.0e6 * np.clip((xs - 2.0) / 10.0, 0.0, 1.0) ** 3)


def torch_fp32(x, xs, ps, slope, c, sums):
    """x (P, F, hw) -> sums (P, 2): the definition as whole-tensor fp32 torch operations"""
    s = torch.sqrt(x[:, U] * x[:, U] + x[:, V] * x[:, V]) * c
    j = (torch.bucketize(s, xs, right=True) - 1).clamp_(0, xs.numel() - 2)
    val = ps[j] + (s - xs[j]) * slope[j]
    val = torch.where(s == xs[-1], ps[-1], val)
    p = torch.where((s < xs[0]) | (s > xs[-1]), torch.zeros_like(val), val)
    sums[:, 0], sums[:, 1] = s.sum(dim=-1, dtype=torch.float64), p.sum(dim=-1, dtype=torch.float64)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def fields(M, T, side):
    torch.manual_seed(0)
    x = torch.randn(M * T, F, side * side, device=dev)
    x[:, U] *= 6.0
    x[:, V] *= 6.0
    return x.contiguous()


def one(M, T, side, curve):
    hw, planes = side * side, M * T
    x = fields(M, T, side)
    c = W.hub_factor()
    table = curve.device_table(dev)
    xs64, ps64, _ = curve._on(dev)
    xs, ps = xs64.float(), ps64.float()
    slope = ((ps64[1:] - ps64[:-1]) / (xs64[1:] - xs64[:-1])).float()
    nbytes = wind_ops.wind_scratch_bytes(planes, hw)
    scratch = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=dev)
    sums, sums_d, sums32, sums64 = (torch.empty(planes, 2, dtype=torch.float64, device=dev) for _ in range(4))
    derived = torch.empty(planes, 2, hw, dtype=torch.float32, device=dev)
    uv = x[:, U:V + 1].contiguous() if V == U + 1 else torch.stack([x[:, U], x[:, V]], dim=1).contiguous()

    def kernel():
        assert wind_ops.wind_power(x, F, U, V, table, curve.K, c, sums, None, scratch, planes, hw)

    def kernel_derived():
        assert wind_ops.wind_power(x, F, U, V, table, curve.K, c, sums_d, derived, scratch, planes, hw)

    routes = {"kernel": kernel, "kernel_derived": kernel_derived, "torch_fp32": lambda: torch_fp32(x, xs, ps, slope, np.float32(c).item(), sums32),
              "general": lambda: W._general(x, curve, U, V, c, None, sums64), "read": lambda: uv.sum()}
    slow = ("general",)
    ms = {k: [] for k in routes}
    for name, fn in routes.items():  # warm-up: code objects, allocator; the warm-up call is the agreement run too
        timed(fn, 1 if name in slow else 2)
    agree32 = float(((sums - sums32).abs() / sums64.abs()).max())
    agree64 = float(((sums - sums64).abs() / sums64.abs()).max())
    torch32_vs64 = float(((sums32 - sums64).abs() / sums64.abs()).max())
    same = bool(torch.equal(sums, sums_d))
    for _ in range(ROUNDS):
        for name, fn in routes.items():
            if name in slow and ms[name]:
                continue  # one timed call
            ms[name].append(timed(fn, 1 if name in slow else ITERS))
    in_bytes = 2 * planes * hw * 4
    read_gbs = in_bytes / (statistics.median(ms["read"]) * 1e-3) / 1e9
    result = {"members": M, "times": T, "vars": F, "hw": hw, "input_bytes": in_bytes, "rounds": ROUNDS, "iters": ITERS,
              "max_rel_kernel_vs_torch_fp32": agree32, "max_rel_kernel_vs_general": agree64, "max_rel_torch_fp32_vs_general": torch32_vs64,
              "sums_equal_with_and_without_derived": same, "measured_read_GBps": round(read_gbs, 1), "routes": {}}
    for name in routes:
        med = statistics.median(ms[name])
        r = dict(members=M, times=T, side=side, route=name, ms_median=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4))
        gbs = in_bytes / (med * 1e-3) / 1e9
        r.update(input_GBps=round(gbs, 1), share_of_measured_read=round(gbs / read_gbs, 3))
        if name == "kernel_derived":
            r.update(moved_GBps=round(2 * gbs, 1))  # as many bytes written as read
        result["routes"][name] = r
        print(json.dumps(r), flush=True)
    k, kd, t32, g = (result["routes"][r]["ms_median"] for r in ("kernel", "kernel_derived", "torch_fp32", "general"))
    print(f"M {M} T {T} {side}x{side}: kernel {k:.4f} ms ({result['routes']['kernel']['input_GBps']:.0f} GB/s of the two planes read, "
          f"{result['routes']['kernel']['share_of_measured_read']:.2f} of the measured read rate {read_gbs:.0f} GB/s), with derived {kd:.4f} ms "
          f"({result['routes']['kernel_derived']['moved_GBps']:.0f} GB/s read + written); torch_fp32 {t32:.3f} ms ({t32 / k:.1f} x), general {g:.3f} ms "
          f"({g / k:.1f} x); sums: kernel vs torch_fp32 {agree32:.2e}, vs general {agree64:.2e}, torch_fp32 vs general {torch32_vs64:.2e} relative; "
          f"equal with and without derived {same}", flush=True)
    return result


def report(M, T, side, curve):
    """the whole wind_report once (host clock around a synchronise: it is many launches), and its two gaussian_kde calls' share"""
    import time
    small = fields(2, 2, 32).view(2, 2, F, 32, 32)
    W.wind_report(small, small[0], curve)  # warm-up: code objects of every kernel the report uses
    x = fields(M + 1, T, side).view(M + 1, T, F, side, side)
    samples, truth = x[:M], x[M]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rep = W.wind_report(samples, truth, curve)
    torch.cuda.synchronize()
    whole = (time.perf_counter() - t0) * 1e3
    d_s = torch.stack([rep["sample_windspeed_100"], rep["sample_windpower"]], dim=2)
    d_t = torch.stack([rep["gt_windspeed_100"], rep["gt_windpower"]], dim=1)
    grid = torch.stack([rep["windspeed_range"], rep["windpower_range"]])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    marginals.gaussian_kde(d_s, grid, truth=d_t)
    torch.cuda.synchronize()
    kde = (time.perf_counter() - t0) * 1e3
    r = dict(route="wind_report", members=M, times=T, side=side, grid_points=300, ms_whole=round(whole, 3), ms_kde=round(kde, 3), kde_share=round(kde / whole, 3))
    print(json.dumps(r), flush=True)
    return r


def main():
    curve = curve61()
    results = [one(M, T, side, curve) for M, T, side in CONFIGS]
    results.append(report(*CONFIGS[0], curve))
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
