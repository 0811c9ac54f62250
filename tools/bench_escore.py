#!/usr/bin/env python3
"""Throughput of the energy-score and variogram-score kernels (csrc/escore.hip) against the torch routes, in one process, with device
events.

    python tools/bench_escore.py     (PAIRS="8x256,64x32" VARIO="8x256x4,8x256x8,16x128x4,16x128x8" VARS=4 ORDER=0.5 ROUNDS=3 ITERS=10;
                                      OUT=path also writes the JSON there)

Fields of 128 x 128.  For every MEMBERSxTIMES of PAIRS and every MEMBERSxTIMESxRADIUS of VARIO (the defaults are ensembles of the same
537 MB), timed alternately in ROUNDS blocks:
  kernel      escore_ops.escore_pairs / vario_terms: the pairs or terms kernel and its fold kernel; its bytes are the samples and the
              truth, each read once from HBM
  torch_fp32  the same product through torch in fp32: for the pairs a difference loop over the rows (row i against all later rows,
              squared, summed over the cells in float64); for the variogram one sliced pass per offset
  general     multivariate._general_pairs / _general_vario: the package's own float64 route, chunked over the times (one call)
  read        torch's sum over the samples: the HBM read rate of this box, against which the kernel's input rate is a share
One JSON line per route, then a summary line per configuration."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from climate2weather_amd import escore_ops
from climate2weather_amd import multivariate as MV

PAIRS = [tuple(int(v) for v in c.split("x")) for c in os.environ.get("PAIRS", "8x256,64x32").split(",") if c]
VARIO = [tuple(int(v) for v in c.split("x")) for c in os.environ.get("VARIO", "8x256x4,8x256x8,16x128x4,16x128x8").split(",") if c]
F = int(os.environ.get("VARS", "4"))
ORDER = float(os.environ.get("ORDER", "0.5"))
ROUNDS, ITERS = int(os.environ.get("ROUNDS", "3")), int(os.environ.get("ITERS", "10"))
H = W = 128
dev = torch.device("cuda:0")


def pairs_fp32(x, y, d2):
    """x (M, T, F, hw), y (T, F, hw) -> d2 (T, F, P): direct fp32 differences, a loop over the rows"""
    rows = torch.cat([y[None], x])
    p, M = 0, x.shape[0]
    for i in range(M):
        d = rows[i + 1:] - rows[i]
        d2[..., p:p + M - i] = (d * d).sum(dim=-1, dtype=torch.float64).permute(1, 2, 0)
        p += M - i


def vario_fp32(x, y, V, R, p):
    """x (M, T, F, H, W), y (T, F, H, W) -> V (T, F, O, 3): one sliced pass per offset in fp32, the sums over a plane in float64"""
    M = x.shape[0]
    pw = (lambda d: d.abs().sqrt()) if p == 0.5 else (lambda d: d.abs()) if p == 1.0 else (lambda d: d * d)
    for o, (di, dj) in enumerate(MV.offsets(R)):
        c = (slice(0, H - di), slice(max(0, -dj), W - max(0, dj)))
        n = (slice(di, H), slice(max(0, dj), W + min(0, dj)))
        gy = pw(y[..., c[0], c[1]] - y[..., n[0], n[1]])
        gx = pw(x[..., c[0], c[1]] - x[..., n[0], n[1]]).sum(dim=0) / M
        V[:, :, o, 0] = ((gy - gx) ** 2).sum(dim=(-2, -1), dtype=torch.float64)
        V[:, :, o, 1] = gy.sum(dim=(-2, -1), dtype=torch.float64)
        V[:, :, o, 2] = gx.sum(dim=(-2, -1), dtype=torch.float64)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def fields(M, T):
    torch.manual_seed(0)
    off = torch.tensor([101325.0, 280.0, 0.0, 3.0], device=dev)[:F] if F <= 4 else torch.zeros(F, device=dev)
    sd = torch.tensor([1200.0, 10.0, 4.0, 4.0], device=dev)[:F] if F <= 4 else torch.ones(F, device=dev)
    centre = off[None, :, None, None] + sd[None, :, None, None] * torch.randn(T, F, H, W, device=dev)
    y = (centre + 0.01 * sd[None, :, None, None] * torch.randn(T, F, H, W, device=dev)).contiguous()
    x = (centre[None] + 0.01 * sd[None, None, :, None, None] * torch.randn(M, T, F, H, W, device=dev)).contiguous()
    return x, y


def run(what, tag, x, y, routes, outs, iters):
    """routes: name -> callable; outs: name -> the tensor the route fills (kernel, torch_fp32, general)"""
    M, T = x.shape[0], x.shape[1]
    ms = {k: [] for k in routes}
    for name, fn in routes.items():  # warm-up: code objects, allocator; the warm-up call is the agreement run too
        timed(fn, 1)
    ref = outs["general"]
    scale = ref.abs().clamp_min(1e-300)
    agree = {k: float(((outs[k] - ref).abs() / scale).max()) for k in ("kernel", "torch_fp32")}
    for _ in range(ROUNDS):
        for name, fn in routes.items():
            if name == "general" and ms[name]:
                continue  # one timed call: seconds
            ms[name].append(timed(fn, iters.get(name, ITERS)))
    in_bytes = (M + 1) * T * F * H * W * 4
    read_gbs = x.numel() * 4 / (statistics.median(ms["read"]) * 1e-3) / 1e9
    result = dict(what=what, config=tag, members=M, times=T, vars=F, input_bytes=in_bytes, max_rel_kernel_vs_general=agree["kernel"],
                  max_rel_torch_fp32_vs_general=agree["torch_fp32"], measured_read_GBps=round(read_gbs, 1), routes={})
    for name in routes:
        med = statistics.median(ms[name])
        gbs = (x.numel() * 4 if name == "read" else in_bytes) / (med * 1e-3) / 1e9
        r = dict(what=what, config=tag, route=name, ms_median=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                 input_GBps=round(gbs, 1), share_of_measured_read=round(gbs / read_gbs, 3))
        result["routes"][name] = r
        print(json.dumps(r), flush=True)
    k, t32, g = (result["routes"][r]["ms_median"] for r in ("kernel", "torch_fp32", "general"))
    print(f"{what} {tag}: kernel {k:.3f} ms ({result['routes']['kernel']['input_GBps']:.0f} GB/s of input, "
          f"{result['routes']['kernel']['share_of_measured_read']:.3f} of the measured read rate {read_gbs:.0f} GB/s); torch_fp32 {t32:.3f} ms "
          f"({t32 / k:.2f} x), general {g:.3f} ms ({g / k:.2f} x); against general: kernel {agree['kernel']:.2e}, torch_fp32 {agree['torch_fp32']:.2e} "
          f"relative", flush=True)
    return result


def one_pairs(M, T):
    x, y = fields(M, T)
    hw, P = H * W, M * (M + 1) // 2
    xf, yf = x.view(M, T, F, hw), y.view(T, F, hw)
    nbytes = escore_ops.escore_scratch_bytes(T * F, hw, M)
    scratch = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=dev)
    outs = {k: torch.empty(T, F, P, dtype=torch.float64, device=dev) for k in ("kernel", "torch_fp32", "general")}

    def kernel():
        assert escore_ops.escore_pairs(xf, yf, outs["kernel"], scratch, M, T * F, hw)

    routes = {"kernel": kernel, "torch_fp32": lambda: pairs_fp32(xf, yf, outs["torch_fp32"]),
              "general": lambda: MV._general_pairs(xf, yf, outs["general"]), "read": lambda: x.sum()}
    return run("pairs", f"{M}x{T}", x, y, routes, outs, {"general": 1, "torch_fp32": max(1, ITERS // 5)})


def one_vario(M, T, R):
    x, y = fields(M, T)
    O = len(MV.offsets(R))
    nbytes = escore_ops.vario_scratch_bytes(T * F, H, W, R)
    scratch = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=dev)
    outs = {k: torch.empty(T, F, O, 3, dtype=torch.float64, device=dev) for k in ("kernel", "torch_fp32", "general")}

    def kernel():
        assert escore_ops.vario_terms(x, y, outs["kernel"], scratch, M, T * F, H, W, R, MV.KERNEL_ORDERS[ORDER])

    routes = {"kernel": kernel, "torch_fp32": lambda: vario_fp32(x, y, outs["torch_fp32"], R, ORDER),
              "general": lambda: MV._general_vario(x, y, outs["general"], R, ORDER), "read": lambda: x.sum()}
    return run(f"vario p={ORDER}", f"{M}x{T} R={R}", x, y, routes, outs, {"general": 1, "torch_fp32": 1, "kernel": max(1, ITERS // 2)})


def main():
    results = [one_pairs(M, T) for M, T in PAIRS] + [one_vario(M, T, R) for M, T, R in VARIO]
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
