#!/usr/bin/env python3
"""Throughput of the quantile-mapping kernels (csrc/qmap.hip) against the torch routes, in one process, with device events.

    python tools/bench_qmap.py     (GRIDS="128,8" HOURS=8760 VARS=4 LEVELS=101 ROUNDS=3 ITERS=5; OUT=path also writes the JSON there)

Per grid size of GRIDS: VARS variables of grid x grid cells over HOURS hours, twelve calendar months as groups, LEVELS levels.  Timed
alternately in ROUNDS blocks, calls back to back on the same tensors, the warm-up call discarded:
  fit      kernel      biascorrect.cell_quantiles on the device: gather + sort kernels, walked over the cell blocks
           torch_fp32  per month torch.sort along time in fp32, two gathers and the interpolation in float64
           general     biascorrect._general_nodes: the package's own float64 route (one call)
  apply    kernel      qmap_ops.qmap_apply
           torch_fp32  per month a transposed copy, a batched torch.searchsorted on fp32 tables, gathers, the formula in fp32
           general     biascorrect._general_apply: float64 (one call)
           add         torch.add(x, 1, out=out): the rate this box reaches on the same bytes read and written
The warm-up call is the agreement run too: the kernel's nodes and mapped values against the general route, as numbers.  One JSON line
per route, then a summary line per problem."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from climate2weather_amd import biascorrect as BC
from climate2weather_amd import qmap_ops

GRIDS = [int(v) for v in os.environ.get("GRIDS", "128,8").split(",") if v]
T = int(os.environ.get("HOURS", "8760"))
F = int(os.environ.get("VARS", "4"))
K = int(os.environ.get("LEVELS", "101"))
ROUNDS, ITERS = int(os.environ.get("ROUNDS", "3")), int(os.environ.get("ITERS", "5"))
dev = torch.device("cuda:0")


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def fields(n, seed):
    """(T, F, n, n): pressure, temperature and two wind-like variables, de-normalised, an annual cycle under the noise"""
    g = torch.Generator(device=dev).manual_seed(seed)
    off = torch.tensor([101325.0, 280.0, 0.0, 3.0] * ((F + 3) // 4), device=dev)[:F].view(1, F, 1, 1)
    sd = torch.tensor([1200.0, 10.0, 4.0, 4.0] * ((F + 3) // 4), device=dev)[:F].view(1, F, 1, 1)
    season = torch.cos(torch.arange(T, device=dev) * (2.0 * 3.141592653589793 / 8760.0)).view(T, 1, 1, 1)
    return (off + sd * (torch.randn(T, F, n, n, device=dev, generator=g) + 0.8 * season)).contiguous()


def nodes_fp32(x, lists, levels, q):
    """x (T, F, hw) -> q (G, F, hw, K): torch.sort along time per group in fp32, the interpolation of the two order statistics in float64"""
    for g, idx in enumerate(lists):
        s = torch.sort(x[idx], dim=0).values                       # (n, F, hw) fp32
        pos = (len(idx) - 1) * levels                               # (K,)
        lo = torch.floor(pos)
        t = (pos - lo).view(-1, 1, 1)
        lo = lo.long()
        hi = (lo + 1).clamp(max=len(idx) - 1)
        a, b = s[lo].double(), s[hi].double()                       # (K, F, hw)
        q[g] = torch.where(t >= 0.5, b - (b - a) * (1.0 - t), a + (b - a) * t).permute(1, 2, 0)


def apply_fp32(x, out, lists, xq, yq):
    """x, out (T, F, hw), xq, yq (G, F, hw, K) fp32: per group a transposed copy, a batched searchsorted, the formula in fp32"""
    Kn = xq.shape[-1]
    for g, idx in enumerate(lists):
        v = x[idx].permute(1, 2, 0).contiguous()                    # (F, hw, n)
        lo = torch.searchsorted(xq[g], v, right=True)
        j = (lo - 1).clamp(0, Kn - 2)
        xj, xj1, yj, yj1 = (torch.gather(t, -1, i) for t, i in ((xq[g], j), (xq[g], j + 1), (yq[g], j), (yq[g], j + 1)))
        inside = torch.minimum(yj + (v - xj) * ((yj1 - yj) / (xj1 - xj)), yj1)
        y = torch.where(lo == 0, v + (yq[g, ..., :1] - xq[g, ..., :1]), torch.where(lo == Kn, v + (yq[g, ..., -1:] - xq[g, ..., -1:]), inside))
        out[idx] = y.permute(2, 0, 1)


def same_numbers(a, b):
    return bool(torch.all((a == b) | (torch.isnan(a) & torch.isnan(b))))


def one(n):
    hw = n * n
    ids = BC.calendar_groups("2001-01-01-00", T)
    gl = BC._GroupLists(ids, 12, T, dev)
    lists = [torch.tensor(i, dtype=torch.int64, device=dev) for i in gl.index]
    levels = torch.tensor(BC._levels(K), dtype=torch.float64, device=dev)
    model, ref = fields(n, 0), fields(n, 1) * 1.1 + 0.5
    xm = model.view(1, T, F, hw)
    q = {k: torch.empty(1, 12, F, hw, K, dtype=torch.float64, device=dev) for k in ("kernel", "torch_fp32", "general")}
    nv = torch.empty(1, 12, F, hw, dtype=torch.int64, device=dev)
    mapping = BC.QuantileMapping.fit(model, ref, levels=K, model_groups=ids, reference_groups=ids, n_groups=12)
    xq, yq = mapping.xq.view(12, F, hw, K), mapping.yq.view(12, F, hw, K)
    xq32, yq32 = xq.float(), yq.float()
    out = {k: torch.empty(1, T, F, hw, device=dev) for k in ("kernel", "torch_fp32", "general", "add")}

    def fit_kernel():
        assert BC._launch_nodes(xm, gl, levels, True, q["kernel"], nv)

    def apply_kernel():
        assert qmap_ops.qmap_apply(xm, out["kernel"], xq, yq, gl.tidx, gl.goff, 1, T, F, hw, T, 12, K, gl.max_len)

    routes = {
        "fit/kernel": fit_kernel,
        "fit/torch_fp32": lambda: nodes_fp32(xm[0], lists, levels, q["torch_fp32"][0]),
        "fit/general": lambda: BC._general_nodes(xm, gl, levels, True, q["general"], nv),
        "apply/kernel": apply_kernel,
        "apply/torch_fp32": lambda: apply_fp32(xm[0], out["torch_fp32"][0], lists, xq32, yq32),
        "apply/general": lambda: BC._general_apply(xm, out["general"], xq, yq, gl),
        "apply/add": lambda: torch.add(xm, 1.0, out=out["add"]),
    }
    ms = {k: [] for k in routes}
    for fn in routes.values():  # warm-up: code objects, allocator; the warm-up call is the agreement run too
        timed(fn, 1)
    agree = dict(nodes_kernel_equals_general=same_numbers(q["kernel"], q["general"]),
                 apply_kernel_equals_general=same_numbers(out["kernel"], out["general"]),
                 nodes_fp32_max_rel=float(((q["torch_fp32"] - q["general"]).abs() / q["general"].abs().clamp_min(1e-30)).max()),
                 apply_fp32_max_rel=float(((out["torch_fp32"] - out["general"]).abs() / out["general"].abs().clamp_min(1e-30)).max()))
    for _ in range(ROUNDS):
        for name, fn in routes.items():
            if name.endswith("general") and ms[name]:
                continue  # one timed call each
            ms[name].append(timed(fn, 1 if name.endswith("general") else ITERS))
    in_bytes = T * F * hw * 4
    tag = f"{F}x{n}x{n}x{T}h G=12 K={K}"
    result = dict(config=tag, grid=n, hours=T, vars=F, levels=K, input_bytes=in_bytes, **agree, routes={})
    for name in routes:
        med = statistics.median(ms[name])
        moved = in_bytes * (2 if name.startswith("apply") else 1)
        r = dict(config=tag, route=name, ms_median=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                 GBps=round(moved / (med * 1e-3) / 1e9, 1))
        result["routes"][name] = r
        print(json.dumps(r), flush=True)
    m = {k: v["ms_median"] for k, v in result["routes"].items()}
    print(f"qmap {tag}: fit kernel {m['fit/kernel']:.3f} ms, torch_fp32 {m['fit/torch_fp32']:.3f} ms ({m['fit/torch_fp32'] / m['fit/kernel']:.2f} x), "
          f"general {m['fit/general']:.3f} ms ({m['fit/general'] / m['fit/kernel']:.2f} x); apply kernel {m['apply/kernel']:.3f} ms "
          f"({result['routes']['apply/kernel']['GBps']:.0f} GB/s, {m['apply/add'] / m['apply/kernel']:.3f} of torch.add's rate), torch_fp32 "
          f"{m['apply/torch_fp32']:.3f} ms ({m['apply/torch_fp32'] / m['apply/kernel']:.2f} x), general {m['apply/general']:.3f} ms "
          f"({m['apply/general'] / m['apply/kernel']:.2f} x); {agree}", flush=True)
    return result


def main():
    results = [one(n) for n in GRIDS]
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
