#!/usr/bin/env python3
"""Throughput of the extremes kernels (csrc/extremes.hip) against the torch routes, in one process, with device events.

    python tools/bench_extremes.py     (SHAPES="8x256,64x32" VARS=4 BLOCK=24 ROUNDS=3 ITERS=10; OUT=path also writes the JSON there)

Fields of 128 x 128 with the truth, block = BLOCK hours (a shape with fewer hours than BLOCK takes block = 8), maxima.  For every
MEMBERSxTIMES of SHAPES, the time of ONE update and of ONE lmoments call on the table it fills, timed alternately in ROUNDS blocks:
  update            extreme_ops.block_extremes_update on a normal field
  update_nan        the same on a field of NaNs: every hour is skipped and counted
  torch_fmax        the fp32 torch route: the whole blocks as view(D, B, block, F, hw) folded with torch.fmax hour by hour (maxima of
                    values, not of keys: no -0.0 < +0.0, no NaN count -- less than the kernel computes)
  general           extremes._general: the package's own route on integer keys (one call)
  read              torch's sum over the samples and the truth: the read rate of this box on the same bytes
  lmoments          extreme_ops.lmoments on the (D F, n, hw) table of the update
  lmoments_sort     extremes._general_lmoments: torch.sort and float64 torch on the same table
  read_table        torch's sum over the table
Every update continues from the keys the call before left: the work per call does not change.  The calls are back to back on the same
tensors, so the caches are as warm as they get; a cold call is not measured.  One JSON line per route."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from climate2weather_amd import extreme_ops
from climate2weather_amd import extremes as EX

SHAPES = [tuple(int(v) for v in c.split("x")) for c in os.environ.get("SHAPES", "8x256,64x32").split(",") if c]
F = int(os.environ.get("VARS", "4"))
BLOCK = int(os.environ.get("BLOCK", "24"))
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


def record(tag, name, ms, in_bytes, read_gbs):
    med = statistics.median(ms)
    gbs = in_bytes / (med * 1e-3) / 1e9
    r = dict(config=tag, route=name, ms_median=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), input_GBps=round(gbs, 1),
             share_of_measured_read=round(gbs / read_gbs, 3))
    print(json.dumps(r), flush=True)
    return r


def fmax_blocks(x, y, block):
    rows = torch.cat([y[None], x])
    D, T, F_, hw = rows.shape
    v = rows[:, :T // block * block].view(D, T // block, block, F_, hw)
    m = v[:, :, 0]
    for i in range(1, block):
        m = torch.fmax(m, v[:, :, i])
    return m


def one(M, T):
    torch.manual_seed(0)
    hw, D = 128 * 128, M + 1
    block = BLOCK if T >= BLOCK else 8
    B = max(1, T // block)
    x, y = torch.randn(M, T, F, hw, device=dev), torch.randn(T, F, hw, device=dev)
    xn, yn = torch.full_like(x, float("nan")), torch.full_like(y, float("nan"))
    dirn = torch.ones(F, dtype=torch.int32, device=dev)
    state = lambda: (torch.zeros(D, F, hw, dtype=torch.int32, device=dev), torch.full((D, F, B, hw), float("nan"), device=dev),
                     torch.zeros(D, F, dtype=torch.int64, device=dev))
    st = {k: state() for k in ("update", "update_nan", "general")}
    kernel = lambda a, b, s: extreme_ops.block_extremes_update(a, b, dirn, *s, M, T, F, hw, block, B, 0) or sys.exit("the kernel declined")
    table = st["update"][1].view(D * F, B, hw)
    lm, nv = torch.empty(D * F, 4, hw, dtype=torch.float64, device=dev), torch.empty(D * F, hw, dtype=torch.int32, device=dev)
    lm2, nv2 = torch.empty_like(lm), torch.empty_like(nv)
    routes = {
        "update": (lambda: kernel(x, y, st["update"]), "in"),
        "update_nan": (lambda: kernel(xn, yn, st["update_nan"]), "in"),
        "torch_fmax": (lambda: fmax_blocks(x, y, block), "in"),
        "general": (lambda: EX._general(x, y, dirn, *st["general"], block, 0), "in"),
        "read": (lambda: (x.sum(), y.sum()), "in"),
        "lmoments": (lambda: extreme_ops.lmoments(table, lm, nv, D * F, B, hw) or sys.exit("the kernel declined"), "table"),
        "lmoments_sort": (lambda: EX._general_lmoments(table, lm2, nv2), "table"),
        "read_table": (lambda: table.sum(), "table"),
    }
    for fn, _ in routes.values():   # warm-up: code objects, allocator; from fresh state the warm-up call is the agreement run too
        timed(fn, 1)
    agree = dict(update_equal_general=bool(torch.equal(st["update"][1].view(torch.int32), st["general"][1].view(torch.int32))),
                 update_equal_fmax=bool(torch.equal(st["update"][1], fmax_blocks(x, y, block).permute(0, 2, 1, 3))),
                 nan_field_all_nan=bool(torch.isnan(st["update_nan"][1]).all()) and int(st["update_nan"][2].sum()) == D * F * T * hw,
                 lmoments_max_abs_diff_to_sort_route=float((lm - lm2).abs().max()), n_blocks=B, block=block)
    ms = {k: [] for k in routes}
    for _ in range(ROUNDS):
        for name, (fn, _) in routes.items():
            ms[name].append(timed(fn, ITERS))
    tag = f"{M}x{T}x{F}x128x128"
    nbytes = dict([("in", 4 * (x.numel() + y.numel())), ("table", 4 * table.numel())])
    read = {k: nbytes[k] / (statistics.median(ms[r]) * 1e-3) / 1e9 for k, r in (("in", "read"), ("table", "read_table"))}
    out = [record(tag, name, ms[name], nbytes[kind], read[kind]) for name, (_, kind) in routes.items()]
    print(json.dumps(dict(config=tag, agreement=agree, input_MB=round(nbytes["in"] / 1e6, 1), table_MB=round(nbytes["table"] / 1e6, 2))), flush=True)
    return dict(config=tag, routes=out, agreement=agree)


def main():
    results = [one(M, T) for M, T in SHAPES]
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
