#!/usr/bin/env python3
"""Throughput of the co-moment kernel (csrc/comoments.hip) against the torch routes, in one process, with device events.

    python tools/bench_dependence.py     (SHAPES="8x256,64x32" VARS=4 HOURS="8,24,256" ROUNDS=3 ITERS=10; OUT=path also writes the JSON there)

Fields of 128 x 128 with the truth.  For every MEMBERSxTIMES of SHAPES, the time of ONE update, timed alternately in ROUNDS blocks:
  update            dependence_ops.comoments_update on a normal field, all T hours in one call
  update_nan        the same on a field of NaNs: every hour is invalid and counted
  update_no_truth   the same members without a truth: M rows instead of M + 1, no truth planes read, NS = F + F (F + 1) / 2
  update_T<h>       one call of the first h hours (h of HOURS below T): the state, 8 NS + 8 F + 4 bytes a series, is loaded and stored
                    once a call whatever h is, so short calls pay for it
  two_pass          an fp32 torch route: centre every series by its mean, then einsum the co-moments and the cross-moments with the
                    truth (no validity, no pivots, fp32 sums -- less than the kernel computes, and not its bits)
  general           dependence._general: the package's own hour-by-hour float64 route (ONE call a round: it is slow)
  read              torch's sum over the samples and the truth: the read rate of this box on the same bytes
Every update continues from the state the call before left: the work per call does not change.  The calls are back to back on the
same tensors, so the caches are as warm as they get; a cold call is not measured.  One JSON line per route."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from climate2weather_amd import dependence_ops
from climate2weather_amd import dependence as DP

SHAPES = [tuple(int(v) for v in c.split("x")) for c in os.environ.get("SHAPES", "8x256,64x32").split(",") if c]
F = int(os.environ.get("VARS", "4"))
HOURS = [int(v) for v in os.environ.get("HOURS", "8,24,256").split(",") if v]
ROUNDS, ITERS = int(os.environ.get("ROUNDS", "3")), int(os.environ.get("ITERS", "10"))
dev = torch.device("cuda:0")


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def record(tag, name, ms, in_bytes, state_bytes, read_gbs):
    med = statistics.median(ms)
    gbs = in_bytes / (med * 1e-3) / 1e9
    r = dict(config=tag, route=name, ms_median=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), input_MB=round(in_bytes / 1e6, 1),
             state_MB_each_way=round(state_bytes / 1e6, 1), input_GBps=round(gbs, 1), share_of_measured_read=round(gbs / read_gbs, 3),
             all_bytes_GBps=round((in_bytes + 2 * state_bytes) / (med * 1e-3) / 1e9, 1))
    print(json.dumps(r), flush=True)
    return r


def two_pass(x, y):
    rows = torch.cat([y[None], x])                                   # (D, T, F, hw)
    c = rows - rows.mean(dim=1, keepdim=True)
    return torch.einsum("dtfc,dtgc->dfgc", c, c), torch.einsum("dtfc,tfc->dfc", c, c[0])


def state(D, with_truth, hw):
    NS = DP.entries(F, with_truth)
    return (torch.zeros(D, hw, dtype=torch.int32, device=dev), torch.zeros(D, F, hw, device=dev), torch.zeros(D, F, hw, device=dev) if with_truth else None,
            torch.zeros(D, NS, hw, dtype=torch.float64, device=dev), torch.zeros(D, dtype=torch.int64, device=dev))


def state_bytes(D, with_truth, hw):
    return D * hw * (8 * DP.entries(F, with_truth) + (8 if with_truth else 4) * F + 4)


def one(M, T):
    torch.manual_seed(0)
    hw, D = 128 * 128, M + 1
    x, y = torch.randn(M, T, F, hw, device=dev), torch.randn(T, F, hw, device=dev)
    xn, yn = torch.full_like(x, float("nan")), torch.full_like(y, float("nan"))
    hours = [h for h in HOURS if h < T]
    short = {h: (x[:, :h].contiguous(), y[:h].contiguous()) for h in hours}
    st = {k: state(D, True, hw) for k in ["update", "update_nan", "general"] + [f"update_T{h}" for h in hours]}
    st["update_no_truth"] = state(M, False, hw)

    def kernel(a, b, s):
        return dependence_ops.comoments_update(a, b, *s, M, int(a.shape[1]), F, hw) or sys.exit("the kernel declined")

    nb = lambda a, b: 4 * (a.numel() + (0 if b is None else b.numel()))
    routes = {
        "update": (lambda: kernel(x, y, st["update"]), nb(x, y), state_bytes(D, True, hw), ITERS),
        "update_nan": (lambda: kernel(xn, yn, st["update_nan"]), nb(x, y), state_bytes(D, True, hw), ITERS),
        "update_no_truth": (lambda: kernel(x, None, st["update_no_truth"]), nb(x, None), state_bytes(M, False, hw), ITERS),
    }
    for h in hours:
        routes[f"update_T{h}"] = (lambda h=h: kernel(*short[h], st[f"update_T{h}"]), nb(*short[h]), state_bytes(D, True, hw), ITERS)
    routes["two_pass"] = (lambda: two_pass(x, y), nb(x, y), 0, ITERS)
    routes["general"] = (lambda: DP._general(x, y, *st["general"]), nb(x, y), state_bytes(D, True, hw), 1)
    routes["read"] = (lambda: (x.sum(), y.sum()), nb(x, y), 0, ITERS)
    for fn, _, _, _ in routes.values():   # warm-up: code objects, allocator; from fresh state the warm-up call is the agreement run too
        timed(fn, 1)
    same = all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
               for a, b in zip(st["update"], st["general"]))
    cov = (st["update"][3][:, F:F + F * (F + 1) // 2] - 0.0)[:, 0] - st["update"][3][:, 0] ** 2 / T          # central sum of variable 0
    agree = dict(update_equal_general_bits=bool(same), nan_field_counts_every_hour=int(st["update_nan"][4].sum()) == D * T * hw,
                 two_pass_max_rel_diff_var0=float(((two_pass(x, y)[0][:, 0, 0].double() - cov).abs() / cov.abs()).max()))
    ms = {k: [] for k in routes}
    for _ in range(ROUNDS):
        for name, (fn, _, _, iters) in routes.items():
            ms[name].append(timed(fn, iters))
    tag = f"{M}x{T}x{F}x128x128"
    read = nb(x, y) / (statistics.median(ms["read"]) * 1e-3) / 1e9
    out = [record(tag, name, ms[name], b, s, read) for name, (_, b, s, _) in routes.items()]
    print(json.dumps(dict(config=tag, agreement=agree)), flush=True)
    return dict(config=tag, routes=out, agreement=agree)


def main():
    results = [one(M, T) for M, T in SHAPES]
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
