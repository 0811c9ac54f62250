#!/usr/bin/env python3
"""Throughput of the SSIM kernel (csrc/ssim.hip) against the avg_pool2d routes, in one process, with device events.

    python tools/bench_ssim.py            (PAIRS=16384 MEMBERS=8 ROUNDS=5 ITERS=10; OUT=path also writes the JSON there)

Timed, alternately, ROUNDS blocks of ITERS calls each, on PAIRS = 8 members x 2048 (frame, variable) slots of 128 x 128, window 15
(1 GiB of samples, four times the Infinity Cache, against 128 MiB of truth):
  kernel        ops.ssim, one launch
  pool_general  ssim._ssim_general: the package's own general route (float64 avg_pool2d in chunks)
  pool_lean     what a careful user writes: fp32, both fields pivoted by the truth's mean, the five moments through ONE avg_pool2d call
                per chunk, the mean over the windows in float64
  read          torch's sum over the samples: the HBM read rate of this box, against which the kernel's input rate is a share
and the kernel alone on the same number of 16 x 16 pairs.  Input bytes = (PAIRS + PAIRS / MEMBERS) * H * W * 4, each field counted once;
a route's GB/s is input bytes over its time, whatever else it moves.  One JSON line per route, then a summary."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from climate2weather_amd import ops
from climate2weather_amd import ssim as ssim_mod

PAIRS, MEMBERS = int(os.environ.get("PAIRS", "16384")), int(os.environ.get("MEMBERS", "8"))
ROUNDS, ITERS = int(os.environ.get("ROUNDS", "5")), int(os.environ.get("ITERS", "10"))
WIN = 15
dev = torch.device("cuda:0")


def pool_lean(x, y, rng, out, win, chunk=512):
    n, nt = x.shape[0], y.shape[0]
    cn = win * win / (win * win - 1.0)
    for i in range(0, n, chunk):
        idx = torch.arange(i, min(n, i + chunk), device=x.device) % nt
        b = y.index_select(0, idx)
        p = b.mean(dim=(-2, -1), keepdim=True)
        a, b = x[i:i + chunk] - p, b - p
        u = torch.nn.functional.avg_pool2d(torch.stack((a, b, a * a, b * b, a * b), dim=1), win, stride=1)
        ua, ub = u[:, 0], u[:, 1]
        va, vb, vab = cn * (u[:, 2] - ua * ua), cn * (u[:, 3] - ub * ub), cn * (u[:, 4] - ua * ub)
        R = rng.index_select(0, idx)[:, None, None]
        C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
        ux, uy, d = ua + p, ub + p, ua - ub
        S = (1.0 - d * d / (ux * ux + uy * uy + C1)) * ((2.0 * vab + C2) / (va + vb + C2))
        out[i:i + chunk] = S.mean(dim=(-2, -1), dtype=torch.float64)


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
    N, nt = 128, PAIRS // MEMBERS
    y = 280.0 + 10.0 * torch.randn(nt, N, N, device=dev)
    x = y.repeat(MEMBERS, 1, 1) + 3.0 * torch.randn(PAIRS, N, N, device=dev)
    rng = torch.full((nt,), 90.0, device=dev)
    out, out2 = torch.empty(PAIRS, dtype=torch.float64, device=dev), torch.empty(PAIRS, dtype=torch.float64, device=dev)
    y16 = 280.0 + 10.0 * torch.randn(nt, 16, 16, device=dev)
    x16 = y16.repeat(MEMBERS, 1, 1) + 3.0 * torch.randn(PAIRS, 16, 16, device=dev)
    routes = {
        "kernel": lambda: ops.ssim(x, y, rng, out, PAIRS, nt, N, N, WIN),
        "pool_general": lambda: ssim_mod._ssim_general(x, y, rng, out2, WIN),
        "pool_lean": lambda: pool_lean(x, y, rng, out2, WIN),
        "read": lambda: x.sum(),
        "kernel_16x16": lambda: ops.ssim(x16, y16, rng, out, PAIRS, nt, 16, 16, WIN),
    }
    # the routes agree before they are timed
    assert ops.ssim(x, y, rng, out, PAIRS, nt, N, N, WIN)
    ssim_mod._ssim_general(x[:256], y, rng, out2[:256], WIN)
    agree = float((out[:256] - out2[:256]).abs().max())
    for name, fn in routes.items():  # warm-up: code objects, pooling algorithms, allocator
        timed(fn, 2)
    ms = {k: [] for k in routes}
    for _ in range(ROUNDS):
        for name, fn in routes.items():
            ms[name].append(timed(fn, ITERS if name not in ("pool_general", "pool_lean") else max(1, ITERS // 5)))
    result = {"pairs": PAIRS, "members": MEMBERS, "win": WIN, "rounds": ROUNDS, "iters": ITERS, "max_abs_kernel_vs_pool_general": agree, "routes": {}}
    read_gbs = x.numel() * 4 / (statistics.median(ms["read"]) * 1e-3) / 1e9
    for name in routes:
        n = 16 if name == "kernel_16x16" else N
        med = statistics.median(ms[name])
        nbytes = x.numel() * 4 if name == "read" else (PAIRS + nt) * n * n * 4
        gbs = nbytes / (med * 1e-3) / 1e9
        r = dict(route=name, N=n, ms_median=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                 pairs_per_s=round(PAIRS / (med * 1e-3)), input_GBps=round(gbs, 1), share_of_measured_read=round(gbs / read_gbs, 3))
        result["routes"][name] = r
        print(json.dumps(r), flush=True)
    k, l, g = (result["routes"][r]["ms_median"] for r in ("kernel", "pool_lean", "pool_general"))
    print(f"kernel {k:.3f} ms vs pool_lean {l:.3f} ms ({l / k:.2f} x) and pool_general {g:.3f} ms ({g / k:.2f} x); measured read rate "
          f"{read_gbs:.0f} GB/s; kernel vs pool_general max |difference| {agree:.2e}")
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
