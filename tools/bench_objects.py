#!/usr/bin/env python3
"""Throughput of the event-object kernel (csrc/objects.hip) against the general torch route, in one process, with device events.

    python tools/bench_objects.py     (SHAPES="8x256,64x32" VARS=4 ROUNDS=3 ITERS=5 FIELDS=...; OUT=path also writes the JSON there)

Fields of 128 x 128 with the truth, K = 2 thresholds per variable, connectivity 8, max_objects 64.  For every MEMBERSxTIMES of SHAPES
(the defaults are ensembles of the same 537 MB plus the truth) and every field, the time of ONE call of object_ops.object_tables,
timed alternately in ROUNDS blocks of ITERS calls:
  smooth        a spatially smooth field (a box filter over white noise), thresholds at the truth's 70th and 95th percentile: a few
                compact objects a plane, the case a user has
  no_event      thresholds no value reaches: the loads and the passes over the bit mask, no link, no LDS add
  all_event     every cell: one object of 16384 cells, every row's run is linked to the one above and adds to ONE area word
  checkerboard  8192 one-cell runs a plane, every one linked to two runs of the row above at connectivity 8: the most links
  random59      white noise at event density 0.59: runs of every length, objects of every size that merge late
next to
  general       objects._general on the same tensors ON THE DEVICE: the package's own torch route (one timed call; it reads a flag back
                per round of its labelling), and the tables of the two routes compared with torch.equal
  read          torch's sum over the samples and the truth: the read rate of this box on the same bytes
The calls are back to back on the same tensors, so the caches are as warm as they get; a cold call is not measured.  One JSON line per
route, then a summary line per configuration and field."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from climate2weather_amd import object_ops
from climate2weather_amd import objects as OB

SHAPES = [tuple(int(v) for v in c.split("x")) for c in os.environ.get("SHAPES", "8x256,64x32").split(",") if c]
FIELDS = [f for f in os.environ.get("FIELDS", "smooth,no_event,all_event,checkerboard,random59").split(",") if f]
F = int(os.environ.get("VARS", "4"))
ROUNDS, ITERS = int(os.environ.get("ROUNDS", "3")), int(os.environ.get("ITERS", "5"))
K, CONNECTIVITY, MAX_OBJECTS, H, W = 2, 8, 64, 128, 128
dev = torch.device("cuda:0")


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def field(name, M, T):
    """(values (M + 1, T, F, H, W) fp32, thr (F, K) fp32): row 0 the truth"""
    shape = (M + 1, T, F, H, W)
    if name in ("smooth", "no_event"):
        v = torch.randn((M + 1) * T, F, H, W, device=dev)
        for _ in range(3):
            v = torch.nn.functional.avg_pool2d(v, 5, stride=1, padding=2, count_include_pad=False)
        v = (v / v.std()).view(shape)
        thr = torch.quantile(v[0].transpose(0, 1).reshape(F, -1)[:, ::64], torch.tensor([0.70, 0.95], device=dev), dim=1).T.contiguous()
        return v, thr if name == "smooth" else torch.full((F, K), 1e30, device=dev)
    if name == "all_event":
        v = torch.ones(shape, device=dev)
    elif name == "checkerboard":
        i, j = torch.arange(H, device=dev).view(H, 1), torch.arange(W, device=dev).view(1, W)
        v = (((i + j) % 2) * 2.0 - 1.0).expand(shape).contiguous()
    elif name == "random59":
        v = (torch.rand(shape, device=dev) < 0.59).float() * 2.0 - 1.0
    else:
        raise KeyError(name)
    return v, torch.tensor([[0.0, 0.5]], device=dev).expand(F, K).contiguous()


class Tables:
    def __init__(self, D, T):
        self.plane = torch.empty(D, T, F, K, 6, dtype=torch.int64, device=dev)
        self.area_hist = torch.zeros(D, F, K, OB.n_bins(H, W), dtype=torch.int64, device=dev)
        self.objects = torch.empty(D, T, F, K, MAX_OBJECTS, 8, dtype=torch.int32, device=dev)
        self.invalid = torch.empty(D, T, F, dtype=torch.int64, device=dev)

    def all(self):
        return self.plane, self.area_hist, self.objects, self.invalid


def one(M, T, name):
    torch.manual_seed(0)
    D, hw = M + 1, H * W
    v, thr = field(name, M, T)
    x, y = v[1:].contiguous().view(M, T, F, hw), v[0].contiguous().view(T, F, hw)
    del v
    above = torch.ones(F, K, dtype=torch.int32, device=dev)
    tk, tg = Tables(D, T), Tables(D, T)

    def kernel():
        assert object_ops.object_tables(x, y, thr, above, *tk.all(), M, T, F, H, W, K, CONNECTIVITY, MAX_OBJECTS)

    general = lambda: OB._general(x, y, thr, above, *tg.all(), H, W, CONNECTIVITY, MAX_OBJECTS)
    routes = {"kernel": kernel, "general": general, "read": lambda: (x.sum(), y.sum())}
    for fn in routes.values():  # warm-up: code objects, allocator; from zeroed histograms the warm-up call is the agreement run too
        timed(fn, 1)
    equal = all(bool(torch.equal(p, q)) for p, q in zip(tk.all(), tg.all()))
    per_plane = tk.plane[..., 0].double().mean().item()
    ms = {k: [] for k in routes}
    for _ in range(ROUNDS):
        for key, fn in routes.items():
            if key == "general" and ms[key]:
                continue  # one timed call
            ms[key].append(timed(fn, 1 if key == "general" else ITERS))
    in_bytes = D * T * F * hw * 4
    med = {k: statistics.median(m) for k, m in ms.items()}
    read_gbs = in_bytes / (med["read"] * 1e-3) / 1e9
    tag = f"{M}x{T}"
    result = dict(config=tag, field=name, members=M, times=T, vars=F, thresholds=K, connectivity=CONNECTIVITY, max_objects=MAX_OBJECTS,
                  planes=D * T * F * K, input_bytes=in_bytes, measured_read_GBps=round(read_gbs, 1), kernel_equal_general=equal,
                  objects_per_plane=round(per_plane, 2), routes={})
    for key in routes:
        gbs = in_bytes / (med[key] * 1e-3) / 1e9
        result["routes"][key] = dict(ms_median=round(med[key], 4), ms_min=round(min(ms[key]), 4), ms_max=round(max(ms[key]), 4),
                                     input_GBps=round(gbs, 1), share_of_measured_read=round(gbs / read_gbs, 3))
        print(json.dumps(dict(config=tag, field=name, route=key, **result["routes"][key])), flush=True)
    print(f"objects {tag} {name}: kernel {med['kernel']:.3f} ms ({result['routes']['kernel']['share_of_measured_read']:.3f} of the measured read rate "
          f"{read_gbs:.0f} GB/s, {med['kernel'] * 1e3 / result['planes']:.3f} us a plane), general {med['general']:.1f} ms "
          f"({med['general'] / med['kernel']:.1f} x), {per_plane:.1f} objects a plane; equal {equal}", flush=True)
    return result


def main():
    results = [one(M, T, name) for M, T in SHAPES for name in FIELDS]
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(results, f, indent=1)
    slower = [(r["config"], r["field"]) for r in results if r["routes"]["kernel"]["ms_median"] > r["routes"]["general"]["ms_median"]]
    unequal = [(r["config"], r["field"]) for r in results if not r["kernel_equal_general"]]
    print(json.dumps(dict(kernel_slower_than_general=slower, tables_differ=unequal)), flush=True)


if __name__ == "__main__":
    main()
