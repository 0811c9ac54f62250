#!/usr/bin/env python3
"""Throughput of the block-moment kernel (csrc/blockmoments.hip) against the torch routes, in one process, with device events.

    python tools/bench_scalesplit.py     (SHAPES="8x256,64x32" VARS=4 SIZES="4,16,32" ROUNDS=3 ITERS=10; OUT=path also writes the JSON there)

Fields of 128 x 128 with the truth.  For every MEMBERSxTIMES of SHAPES and every block size of SIZES, the time of ONE call, timed
alternately in ROUNDS blocks:
  kernel            scale_ops.block_moments into tables allocated once
  kernel_no_truth   the same members without a truth: M rows instead of M + 1, no truth planes read, NS = 2
  pool32            the fp32 torch route a user would write: avg_pool2d of x, of x x and of x y (not the bits, and off by more than
                    the field's standard deviation on a pressure-like field: tests/test_scalesplit_cpu.py)
  general           scalesplit._general: the package's own float64 route, the same bits (ONE call a round: it is slow)
  read              torch's sum over the samples and the truth: the read rate of this box on the same bytes
and, per shape, ``profile``: scalesplit.scale_profile at its default scales (2 takes the general route).  The calls are back to back on
the same tensors, so the caches are as warm as they get; a cold call is not measured.  One JSON line per route."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from climate2weather_amd import scale_ops
from climate2weather_amd import scalesplit as SS

SHAPES = [tuple(int(v) for v in c.split("x")) for c in os.environ.get("SHAPES", "8x256,64x32").split(",") if c]
F = int(os.environ.get("VARS", "4"))
SIZES = [int(v) for v in os.environ.get("SIZES", "4,16,32").split(",") if v]
ROUNDS, ITERS = int(os.environ.get("ROUNDS", "3")), int(os.environ.get("ITERS", "10"))
H = W = 128
dev = torch.device("cuda:0")


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def record(tag, name, ms, in_bytes, out_bytes, read_gbs):
    med = statistics.median(ms)
    gbs = in_bytes / (med * 1e-3) / 1e9
    r = dict(config=tag, route=name, ms_median=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), input_MB=round(in_bytes / 1e6, 1),
             output_MB=round(out_bytes / 1e6, 1), input_GBps=round(gbs, 1), share_of_measured_read=round(gbs / read_gbs, 3))
    print(json.dumps(r), flush=True)
    return r


def pool32(x, y, s):
    pool = torch.nn.functional.avg_pool2d
    M, T = x.shape[:2]
    return pool(x.view(M * T, F, H, W), s), pool((x * x).view(M * T, F, H, W), s), pool((x * y[None]).view(M * T, F, H, W), s)


def tables(D, T, NS, s):
    h, w = H // s, W // s
    return (torch.empty(D, T, F, h, w, dtype=torch.int32, device=dev), torch.empty(D, T, F, h, w, device=dev),
            torch.empty(D, T, F, NS, h, w, dtype=torch.float64, device=dev))


def one(M, T):
    torch.manual_seed(0)
    x, y = torch.randn(M, T, F, H, W, device=dev), torch.randn(T, F, H, W, device=dev)
    nb = lambda a, b: 4 * (a.numel() + (0 if b is None else b.numel()))
    routes, agree = {}, {}
    for s in SIZES:
        st, sn, sg = tables(M + 1, T, 3, s), tables(M, T, 2, s), tables(M + 1, T, 3, s)
        out = lambda t: sum(a.numel() * a.element_size() for a in t)

        def kernel(a, b, t, s=s):
            return scale_ops.block_moments(a, b, *t, M, T, F, H, W, s) or sys.exit("the kernel declined")

        routes[f"kernel_s{s}"] = (lambda st=st, kernel=kernel: kernel(x, y, st), nb(x, y), out(st), ITERS)
        routes[f"kernel_no_truth_s{s}"] = (lambda sn=sn, kernel=kernel: kernel(x, None, sn), nb(x, None), out(sn), ITERS)
        routes[f"pool32_s{s}"] = (lambda s=s: pool32(x, y, s), nb(x, y), 0, ITERS)
        routes[f"general_s{s}"] = (lambda sg=sg, s=s: SS._general(x, y, *sg, s), nb(x, y), out(sg), 1)
        agree[s] = (st, sg)
    routes["profile"] = (lambda: SS.scale_profile(x, y), nb(x, y), 0, 1)
    routes["read"] = (lambda: (x.sum(), y.sum()), nb(x, y), 0, ITERS)
    for fn, _, _, _ in routes.values():   # warm-up: code objects, allocator; the warm-up call is the agreement run too
        timed(fn, 1)
    same = {f"kernel_equal_general_bits_s{s}": all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a.view(torch.int32),
                                                               b.view(torch.int64) if b.dtype == torch.float64 else b.view(torch.int32))
                                                   for a, b in zip(st, sg)) for s, (st, sg) in agree.items()}
    ms = {k: [] for k in routes}
    for _ in range(ROUNDS):
        for name, (fn, _, _, iters) in routes.items():
            ms[name].append(timed(fn, iters))
    tag = f"{M}x{T}x{F}x{H}x{W}"
    read = nb(x, y) / (statistics.median(ms["read"]) * 1e-3) / 1e9
    out = [record(tag, name, ms[name], b, o, read) for name, (_, b, o, _) in routes.items()]
    print(json.dumps(dict(config=tag, agreement=same)), flush=True)
    return dict(config=tag, routes=out, agreement=same)


def main():
    results = [one(M, T) for M, T in SHAPES]
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
