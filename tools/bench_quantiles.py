#!/usr/bin/env python3
"""Throughput of the quantile kernels (csrc/quantile.hip) against a torch.sort per data set, in one process, with device events.

    python tools/bench_quantiles.py      (MEMBERS=8 TIMES=1457 VARS=4 PRE_TIMES=21900 ROUNDS=5 ITERS=3; OUT=path also writes the JSON)

Workloads, all on fields of 128 x 128 at the reference's nine levels:
  ensemble      MEMBERS x TIMES x VARS fields against TIMES x VARS truth fields: D = MEMBERS VARS + VARS data sets of TIMES x 16384
                values, standard normal -- and the same shape filled with ONE constant and with a pressure-like field (101325 + 900 z),
                the hot-bin worst cases: every value of a wave lands on one LDS counter in every pass (constant) or in pass 0 (pressure)
  preprocessing one "member" of PRE_TIMES x VARS fields, no truth: D = VARS data sets (the reference's compute_quantiles; its 87600
                hours are 23 GB, PRE_TIMES is what is timed here)
Per workload, ROUNDS blocks of ITERS calls of ops.quantiles (the memset, three counting launches, three locating launches); the sort
route -- torch.sort of every data set in fp32 and a gather of the same ranks -- is timed once per workload and its order statistics
must equal the kernels' bit for bit.  "read" is torch's sum over the samples: the HBM read rate of this box.  The counting kernel reads
the data three times, so the yardstick of a call is 3 x bytes / read rate.  One JSON line per route, then a summary."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from climate2weather_amd import ops
from climate2weather_amd.quantiles import REFERENCE_LEVELS

M, T, F = int(os.environ.get("MEMBERS", "8")), int(os.environ.get("TIMES", "1457")), int(os.environ.get("VARS", "4"))
PRE_T = int(os.environ.get("PRE_TIMES", "21900"))
ROUNDS, ITERS = int(os.environ.get("ROUNDS", "5")), int(os.environ.get("ITERS", "3"))
H = W = 128
Q = len(REFERENCE_LEVELS)
dev = torch.device("cuda:0")


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def fill(t, kind):
    if kind == "constant":
        t.fill_(3.5)
    else:
        t.normal_()
        if kind == "pressure":
            t.mul_(900.0).add_(101325.0)


def sort_route(x, y, stats):
    """the order statistics of every data set from a full fp32 torch.sort (no NaNs in the benchmark's fields)"""
    n_rep, T_, F_, hw = x.shape
    n = T_ * hw
    pos = (n - 1) * torch.tensor(REFERENCE_LEVELS, dtype=torch.float64, device=x.device)
    lo = torch.floor(pos).long()
    hi = torch.clamp(lo + 1, max=n - 1)
    for ds in range(stats.shape[0]):
        v = (x[ds // F_, :, ds % F_] if ds < n_rep * F_ else y[:, ds - n_rep * F_]).reshape(-1)
        s = torch.sort(v).values
        stats[ds, :, 0], stats[ds, :, 1] = s[lo], s[hi]


class Workload:
    def __init__(self, name, n_rep, times, with_truth):
        self.name, self.n_rep, self.T = name, n_rep, times
        self.x = torch.empty(n_rep, times, F, H * W, device=dev)
        self.y = torch.empty(times, F, H * W, device=dev) if with_truth else None
        self.D = n_rep * F + (F if with_truth else 0)
        self.bytes = (self.x.numel() + (self.y.numel() if with_truth else 0)) * 4
        self.scratch = torch.empty(ops.quantile_scratch_bytes(self.D, Q) // 8, dtype=torch.int64, device=dev)
        self.out = torch.empty(self.D, Q, dtype=torch.float64, device=dev)
        self.stats = torch.empty(self.D, Q, 2, device=dev)
        self.nv = torch.empty(self.D, dtype=torch.int64, device=dev)

    def call(self):
        assert ops.quantiles(self.x, self.y, REFERENCE_LEVELS, True, self.scratch, self.out, self.stats, self.nv, self.n_rep, self.T, F, H * W)

    def measure(self, kind, with_sort):
        fill(self.x, kind)
        if self.y is not None:
            fill(self.y, kind)
        timed(self.call, 2)  # warm-up: code objects, the LDS opt-in
        ms = [timed(self.call, ITERS) for _ in range(ROUNDS)]
        read = [timed(lambda: self.x.sum(), ITERS) for _ in range(ROUNDS)]
        med = statistics.median(ms)
        read_gbs = self.x.numel() * 4 / (statistics.median(read) * 1e-3) / 1e9
        r = dict(route=f"{self.name}/{kind}", data_sets=self.D, values_per_set=self.T * H * W, input_GB=round(self.bytes / 1e9, 3),
                 ms_median=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), input_GBps=round(self.bytes / (med * 1e-3) / 1e9, 1),
                 read_GBps=round(read_gbs, 1), ratio_to_three_reads=round(med * 1e-3 / (3 * self.bytes / (read_gbs * 1e9)), 3))
        if with_sort:
            want = torch.empty_like(self.stats)
            sort_ms = timed(lambda: sort_route(self.x, self.y, want), 1)  # its warm-up is its agreement run
            sort_ms = min(sort_ms, timed(lambda: sort_route(self.x, self.y, want), 1))
            r.update(sort_route_ms=round(sort_ms, 3), speedup_over_sort=round(sort_ms / med, 2),
                     stats_equal_sort=bool(torch.equal(self.stats.view(torch.int32), want.view(torch.int32))),
                     n_valid_ok=bool((self.nv == self.T * H * W).all()))
        print(json.dumps(r), flush=True)
        return r


def main():
    torch.manual_seed(0)
    results = []
    ens = Workload("ensemble", M, T, True)
    for kind in ("normal", "constant", "pressure", "normal"):  # the normal field twice: the spread between two visits of one case
        results.append(ens.measure(kind, with_sort=kind != "constant" and not any(r["route"] == f"ensemble/{kind}" for r in results)))
    del ens
    torch.cuda.empty_cache()
    pre = Workload("preprocessing", 1, PRE_T, False)
    results.append(pre.measure("normal", with_sort=True))
    normal = [r for r in results if r["route"] == "ensemble/normal"]
    const = next(r for r in results if r["route"] == "ensemble/constant")
    press = next(r for r in results if r["route"] == "ensemble/pressure")
    lo, hi = min(r["ms_min"] for r in normal), max(r["ms_max"] for r in normal)
    print(f"ensemble: normal {normal[0]['ms_median']:.3f} / {normal[1]['ms_median']:.3f} ms (all repeats {lo:.3f} .. {hi:.3f}), constant "
          f"{const['ms_median']:.3f} ms, pressure {press['ms_median']:.3f} ms; constant beyond the normal field's spread: {const['ms_median'] > hi}; "
          f"preprocessing {results[-1]['ms_median']:.3f} ms at {results[-1]['input_GBps']:.0f} GB/s of input")
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(dict(members=M, times=T, vars=F, pre_times=PRE_T, levels=list(REFERENCE_LEVELS), rounds=ROUNDS, iters=ITERS,
                           compute_units=torch.cuda.get_device_properties(0).multi_processor_count, routes=results), f, indent=1)


if __name__ == "__main__":
    main()
