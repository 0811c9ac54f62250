#!/usr/bin/env python3
"""Throughput of the two event-verification kernels (csrc/events.hip) against the torch routes, in one process, with device events.

    python tools/bench_events.py     (SHAPES="8x256,64x32" VARS=4 ROUNDS=3 ITERS=10; OUT=path also writes the JSON there)

Fields of 128 x 128, K = 2 thresholds per variable, radii (0, 1, 2, 4, 8).  For every MEMBERSxTIMES of SHAPES (the defaults are
ensembles of the same 537 MB), timed alternately in ROUNDS blocks:
  counts            event_ops.event_counts on a random field (thresholds at the truth's 95th and 99th percentile)
  counts_no_event   the same with thresholds no value reaches: every cell is bin (0, 0), the bin the kernel never sends to LDS
  counts_torch      the same table through torch in fp32: ``(x >= thr).sum(0)`` and one-hot sums over the cells, chunked over the times
  fss               event_ops.fss_sums at K = 2; fss_k1 the same at K = 1 (the thresholds run over the grid: what a second one costs)
  fss_torch         the same sums through torch in fp32: ``avg_pool2d`` with zero padding per radius
  fss_general       events._general_fss: the package's own int64 route (cumulative tables, clipped corner differences; one call)
  read              torch's sum over the samples and the truth: the read rate of this box on the same bytes
The calls are back to back on the same tensors, so the caches are as warm as they get.  One JSON line per route, then a summary line per
configuration."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from climate2weather_amd import event_ops
from climate2weather_amd import events as EV

SHAPES = [tuple(int(v) for v in c.split("x")) for c in os.environ.get("SHAPES", "8x256,64x32").split(",") if c]
F = int(os.environ.get("VARS", "4"))
ROUNDS, ITERS = int(os.environ.get("ROUNDS", "3")), int(os.environ.get("ITERS", "10"))
H = W = 128
K, RADII = 2, (0, 1, 2, 4, 8)
dev = torch.device("cuda:0")


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def counts_torch(x, y, thr, counts):
    """x (M, T, F, hw), y (T, F, hw), thr (F, K) -> counts (T, F, K, 2, M + 1): member counts by a sum over the members, bins by one-hot sums"""
    M, T = int(x.shape[0]), int(x.shape[1])
    th = thr[:, :, None]
    step = max(1, (1 << 25) // (F * K * x.shape[-1] * 2 * (M + 1) // 8))
    for t0 in range(0, T, step):
        j = (x[:, t0:t0 + step, :, None, :] >= th).sum(dim=0)
        o = (y[t0:t0 + step, :, None, :] >= th).long()
        counts[t0:t0 + step] = torch.nn.functional.one_hot(o * (M + 1) + j, 2 * (M + 1)).sum(dim=-2).view(-1, F, K, 2, M + 1)


def fss_torch(x, y, thr, sums):
    """the FSS sums in fp32: indicator rows, a zero-padded box sum per radius by avg_pool2d, products summed in float64"""
    M, T = int(x.shape[0]), int(x.shape[1])
    th = thr[:, :, None]
    step = max(1, (1 << 24) // ((M + 2) * F * K * H * W // 8))
    for t0 in range(0, T, step):
        e = (x[:, t0:t0 + step, :, None, :] >= th).float()
        rows = torch.cat([(y[t0:t0 + step, :, None, :] >= th).float()[None], e, e.sum(dim=0, keepdim=True)])  # (M + 2, t, F, K, hw)
        shape = rows.shape[:-1]
        for s, r in enumerate(RADII):
            n = torch.nn.functional.avg_pool2d(rows.view(-1, 1, H, W), 2 * r + 1, stride=1, padding=r, count_include_pad=True) * float((2 * r + 1) ** 2)
            n = n.view(shape + (H * W,))
            sums[t0:t0 + step, :, :, s, :, 0] = (n * n).sum(dim=-1, dtype=torch.float64).permute(1, 2, 3, 0).long()
            sums[t0:t0 + step, :, :, s, :, 1] = (n * n[:1]).sum(dim=-1, dtype=torch.float64).permute(1, 2, 3, 0).long()


def one(M, T):
    torch.manual_seed(0)
    hw = H * W
    y = torch.randn(T, F, H, W, device=dev)
    x = 0.6 * y[None] + 0.8 * torch.randn(M, T, F, H, W, device=dev)
    xf, yf = x.view(M, T, F, hw), y.view(T, F, hw)
    thr = EV.thresholds_from_quantiles(y, (0.95, 0.99)).contiguous()
    never = torch.full((F, K), 1e30, device=dev)
    above = torch.ones(F, K, dtype=torch.int32, device=dev)
    c = {k: torch.empty(T, F, K, 2, M + 1, dtype=torch.int64, device=dev) for k in ("counts", "counts_no_event", "counts_torch")}
    inv = torch.empty(T, F, dtype=torch.int64, device=dev)
    s = {k: torch.empty(T, F, K, len(RADII), M + 2, 2, dtype=torch.int64, device=dev) for k in ("fss", "fss_torch", "fss_general")}
    s1 = torch.empty(T, F, 1, len(RADII), M + 2, 2, dtype=torch.int64, device=dev)
    thr1, above1 = thr[:, :1].contiguous(), above[:, :1].contiguous()

    def k_counts():
        assert event_ops.event_counts(xf, yf, thr, above, c["counts"], inv, M, T, F, hw, K)

    def k_none():
        assert event_ops.event_counts(xf, yf, never, above, c["counts_no_event"], inv, M, T, F, hw, K)

    def k_fss():
        assert event_ops.fss_sums(xf, yf, thr, above, s["fss"], RADII, M, T, F, H, W, K)

    def k_fss1():
        assert event_ops.fss_sums(xf, yf, thr1, above1, s1, RADII, M, T, F, H, W, 1)

    def read():
        x.sum()
        y.sum()

    routes = {"counts": k_counts, "counts_no_event": k_none, "counts_torch": lambda: counts_torch(xf, yf, thr, c["counts_torch"]),
              "fss": k_fss, "fss_k1": k_fss1, "fss_torch": lambda: fss_torch(xf, yf, thr, s["fss_torch"]),
              "fss_general": lambda: EV._general_fss(xf, yf, thr, above, s["fss_general"], list(RADII), H, W), "read": read}
    iters = {"fss_general": 1, "fss_torch": 1, "counts_torch": max(1, ITERS // 5)}
    ms = {k: [] for k in routes}
    for name, fn in routes.items():  # warm-up: code objects, allocator; the warm-up call is the agreement run too
        timed(fn, 1)
    agree = dict(counts_equal_torch=bool(torch.equal(c["counts"], c["counts_torch"])),
                 no_event_all_in_bin_0=bool((c["counts_no_event"][..., 0, 0] == hw).all()),
                 fss_equal_general=bool(torch.equal(s["fss"], s["fss_general"])), fss_k1_equal=bool(torch.equal(s1[:, :, 0], s["fss"][:, :, 0])),
                 fss_torch_fp32_max_rel=float(((s["fss_torch"] - s["fss_general"]).abs().double() / s["fss_general"].abs().clamp_min(1).double()).max()))
    for _ in range(ROUNDS):
        for name, fn in routes.items():
            if name in ("fss_general", "fss_torch") and ms[name]:
                continue  # one timed call
            ms[name].append(timed(fn, iters.get(name, ITERS)))
    in_bytes = (M + 1) * T * F * hw * 4
    read_gbs = in_bytes / (statistics.median(ms["read"]) * 1e-3) / 1e9
    tag = f"{M}x{T}"
    result = dict(config=tag, members=M, times=T, vars=F, thresholds=K, radii=list(RADII), input_bytes=in_bytes,
                  measured_read_GBps=round(read_gbs, 1), agreement=agree, routes={})
    for name in routes:
        med = statistics.median(ms[name])
        gbs = in_bytes / (med * 1e-3) / 1e9
        r = dict(config=tag, route=name, ms_median=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                 input_GBps=round(gbs, 1), share_of_measured_read=round(gbs / read_gbs, 3))
        result["routes"][name] = r
        print(json.dumps(r), flush=True)
    m = {k: v["ms_median"] for k, v in result["routes"].items()}
    print(f"events {tag}: counts {m['counts']:.3f} ms ({result['routes']['counts']['share_of_measured_read']:.3f} of the measured read rate "
          f"{read_gbs:.0f} GB/s), no event {m['counts_no_event']:.3f} ms, torch {m['counts_torch']:.3f} ms ({m['counts_torch'] / m['counts']:.1f} x); "
          f"fss {m['fss']:.3f} ms (K = 1: {m['fss_k1']:.3f} ms), torch fp32 {m['fss_torch']:.3f} ms ({m['fss_torch'] / m['fss']:.1f} x), "
          f"general {m['fss_general']:.3f} ms ({m['fss_general'] / m['fss']:.1f} x); {json.dumps(agree)}", flush=True)
    return result


def main():
    results = [one(M, T) for M, T in SHAPES]
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
