#!/usr/bin/env python3
"""Throughput of the event-spell kernel (csrc/spells.hip) against the torch routes, in one process, with device events.

    python tools/bench_spells.py     (SHAPES="8x256,64x32" VARS=4 ROUNDS=3 ITERS=10; OUT=path also writes the JSON there)

Fields of 128 x 128 with the truth, K = 2 thresholds per variable, max_duration 48, period 6.  For every MEMBERSxTIMES of SHAPES (the
defaults are ensembles of the same 537 MB plus the truth), the time of ONE update, timed alternately in ROUNDS blocks:
  smooth            spell_ops.spell_update on an AR(1) field (rho = 0.95), thresholds at the truth's 70th and 95th percentile: long spells
  smooth_k1, _k4    the same at K = 1 (the first threshold) and K = 4 (the 50th, 70th, 90th and 95th percentile): what a threshold costs
  no_event          the same field with thresholds no value reaches: no LDS traffic at all
  alternating       a field whose event flips every hour: one LDS add per threshold per two cell-hours, the worst case
  torch             the same integers of the smooth field through torch on the device, int32 temporaries: the running-maximum formulation,
                    chunked over the cells
  general           spells._general on the smooth field: the package's own int64 route (one call)
  read              torch's sum over the samples and the truth: the read rate of this box on the same bytes
and two inputs on which the kernel cannot fill the chip (time is not split over workgroups):
  one_row           one member of one variable, no truth, 128 x 128 over 2048 hours: 16 workgroups
  coarse            8 members and the truth, 4 variables on an 8 x 8 grid over 8760 hours: 36 workgroups of 16 threads
each next to torch's sum over its bytes.  Every call continues from the state the call before left: the counters grow, the work per
call does not.  The calls are back to back on the same tensors, so the caches are as warm as they get; a cold call is not measured.
One JSON line per route, then a summary line per configuration."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from climate2weather_amd import spell_ops
from climate2weather_amd import spells as SP

SHAPES = [tuple(int(v) for v in c.split("x")) for c in os.environ.get("SHAPES", "8x256,64x32").split(",") if c]
F = int(os.environ.get("VARS", "4"))
ROUNDS, ITERS = int(os.environ.get("ROUNDS", "3")), int(os.environ.get("ITERS", "10"))
K, LMAX, PERIOD = 2, 48, 6
dev = torch.device("cuda:0")


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def ar1(M, T, F_, H, W, rho=0.95):
    """(M + 1, T, F, H, W) fp32: unit-variance AR(1) along time, built plane by plane on the device"""
    v = torch.empty(M + 1, T, F_, H, W, device=dev)
    v[:, 0] = torch.randn(M + 1, F_, H, W, device=dev)
    for t in range(1, T):
        v[:, t] = rho * v[:, t - 1] + (1.0 - rho * rho) ** 0.5 * torch.randn(M + 1, F_, H, W, device=dev)
    return v


class Tables:
    """a zeroed state and zeroed accumulators"""

    def __init__(self, D, F_, hw, k=K):
        self.state = torch.zeros(4, D, F_, k, hw, dtype=torch.int32, device=dev)
        self.hist = torch.zeros(D, F_, k, LMAX, dtype=torch.int64, device=dev)
        self.onsets = torch.zeros(D, F_, k, PERIOD, dtype=torch.int64, device=dev)
        self.invalid = torch.zeros(D, F_, dtype=torch.int64, device=dev)

    def all(self):
        return self.state, self.hist, self.onsets, self.invalid


def update_torch(x, y, thr, tb, t0):
    """the kernel's integers through torch with int32 temporaries: x (M, T, F, hw), y (T, F, hw) or None, thresholds above"""
    M, T, F_, hw = x.shape
    D = M + (0 if y is None else 1)
    tt = torch.arange(T, dtype=torch.int32, device=dev).view(T, 1, 1, 1, 1)
    minus, zero = torch.full_like(tt, -1), torch.zeros((), dtype=torch.int32, device=dev)
    phase = ((t0 + torch.arange(T, device=dev)) % PERIOD).view(T, 1, 1, 1, 1)
    row = torch.arange(D * F_ * K, device=dev).view(1, D, F_, K, 1)
    step = max(4, (1 << 25) // (T * D * F_ * K) // 4 * 4)
    for c0 in range(0, hw, step):
        xs = x[..., c0:c0 + step]
        rows = xs if y is None else torch.cat([y[None, ..., c0:c0 + step], xs])           # (D, T, F, cells)
        e = (rows[:, :, :, None, :] >= thr[:, :, None]).permute(1, 0, 2, 3, 4)             # (T, D, F, K, cells)
        st = tb.state[..., c0:c0 + step]
        open_in = st[0].clone()
        lastzero = torch.where(e, minus, tt).cummax(dim=0).values
        length = tt - lastzero + torch.where(lastzero < 0, open_in, zero)
        was_open = open_in > 0
        ended = torch.cat([e & ~torch.cat([e[1:], torch.ones_like(e[:1])]), (~e[0] & was_open)[None]])
        starts = e & ~torch.cat([was_open[None], e[:-1]])
        L = torch.where(ended, torch.cat([length, open_in[None]]), zero)
        bins = (row * LMAX + L.clamp(1, LMAX) - 1)[ended]
        tb.hist.view(-1).add_(torch.bincount(bins, minlength=tb.hist.numel()))
        tb.onsets.view(-1).add_(torch.bincount((row * PERIOD + phase).expand(starts.shape)[starts], minlength=tb.onsets.numel()))
        st[2] += ended.sum(dim=0, dtype=torch.int32)
        st[1] = torch.maximum(st[1], L.amax(dim=0))
        st[3] += e.sum(dim=0, dtype=torch.int32)
        st[0] = torch.where(e[-1], length[-1], zero)


def kernel_call(x, y, thr, above, tb, M, T, F_, hw, t0):
    k = int(thr.shape[1])
    assert spell_ops.spell_update(x, y, thr, above, tb.state, tb.hist, tb.onsets, tb.invalid, M, T, F_, hw, k, LMAX, PERIOD, t0)


def record(tag, name, ms, in_bytes, read_gbs):
    med = statistics.median(ms)
    gbs = in_bytes / (med * 1e-3) / 1e9
    r = dict(config=tag, route=name, ms_median=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), input_GBps=round(gbs, 1),
             share_of_measured_read=round(gbs / read_gbs, 3))
    print(json.dumps(r), flush=True)
    return r


def one(M, T):
    torch.manual_seed(0)
    H = W = 128
    hw, D = H * W, M + 1
    v = ar1(M, T, F, H, W)
    x, y = v[1:].contiguous().view(M, T, F, hw), v[0].contiguous().view(T, F, hw)
    del v
    parity = (torch.arange(T, device=dev) % 2).float().view(1, T, 1, 1) * 2.0 - 1.0
    xa, ya = parity.expand(M, T, F, hw).contiguous(), parity[0].expand(T, F, hw).contiguous()
    thr = torch.quantile(y.transpose(0, 1).reshape(F, -1)[:, ::64], torch.tensor([0.70, 0.95], device=dev), dim=1).T.contiguous()
    never, flip = torch.full((F, K), 1e30, device=dev), torch.zeros(F, K, device=dev)
    above = torch.ones(F, K, dtype=torch.int32, device=dev)
    tb = {k: Tables(D, F, hw) for k in ("smooth", "no_event", "alternating", "torch", "general")}
    tb["smooth_k1"], tb["smooth_k4"] = Tables(D, F, hw, 1), Tables(D, F, hw, 4)
    thr1 = thr[:, :1].contiguous()
    thr4 = torch.quantile(y.transpose(0, 1).reshape(F, -1)[:, ::64], torch.tensor([0.5, 0.70, 0.9, 0.95], device=dev), dim=1).T.contiguous()
    above1, above4 = above[:, :1].contiguous(), torch.ones(F, 4, dtype=torch.int32, device=dev)
    routes = {
        "smooth": lambda: kernel_call(x, y, thr, above, tb["smooth"], M, T, F, hw, 0),
        "smooth_k1": lambda: kernel_call(x, y, thr1, above1, tb["smooth_k1"], M, T, F, hw, 0),
        "smooth_k4": lambda: kernel_call(x, y, thr4, above4, tb["smooth_k4"], M, T, F, hw, 0),
        "no_event": lambda: kernel_call(x, y, never, above, tb["no_event"], M, T, F, hw, 0),
        "alternating": lambda: kernel_call(xa, ya, flip, above, tb["alternating"], M, T, F, hw, 0),
        "torch": lambda: update_torch(x, y, thr, tb["torch"], 0),
        "general": lambda: SP._general(x, y, thr, above, *tb["general"].all(), LMAX, PERIOD, 0),
        "read": lambda: (x.sum(), y.sum()),
    }
    ms = {k: [] for k in routes}
    for name, fn in routes.items():  # warm-up: code objects, allocator; from zeroed tables the warm-up call is the agreement run too
        timed(fn, 1)
    same = lambda a, b: all(bool(torch.equal(p, q)) for p, q in zip(tb[a].all()[:3], tb[b].all()[:3]))
    spells = tb["alternating"].hist.sum().item() + (tb["alternating"].state[0] > 0).sum().item()
    agree = dict(smooth_equal_general=same("smooth", "general"), smooth_equal_torch=same("smooth", "torch"),
                 no_event_all_zero=bool(tb["no_event"].hist.sum().item() == 0 and tb["no_event"].state.abs().sum().item() == 0),
                 alternating_spells=bool(spells == D * F * K * hw * (T // 2)),
                 mean_spell_hours_smooth=round(tb["smooth"].state[3].sum().item() / max(1, tb["smooth"].hist.sum().item()), 2))
    single = {"general": 1, "torch": 1}
    for _ in range(ROUNDS):
        for name, fn in routes.items():
            if name in single and ms[name]:
                continue  # one timed call
            ms[name].append(timed(fn, single.get(name, ITERS)))
    in_bytes = D * T * F * hw * 4
    read_gbs = in_bytes / (statistics.median(ms["read"]) * 1e-3) / 1e9
    tag = f"{M}x{T}"
    result = dict(config=tag, members=M, times=T, vars=F, thresholds=K, max_duration=LMAX, period=PERIOD, input_bytes=in_bytes,
                  measured_read_GBps=round(read_gbs, 1), agreement=agree, routes={k: record(tag, k, ms[k], in_bytes, read_gbs) for k in routes})
    m = {k: r["ms_median"] for k, r in result["routes"].items()}
    print(f"spells {tag}: smooth {m['smooth']:.3f} ms ({result['routes']['smooth']['share_of_measured_read']:.3f} of the measured read rate "
          f"{read_gbs:.0f} GB/s; K = 1: {m['smooth_k1']:.3f} ms, K = 4: {m['smooth_k4']:.3f} ms), no event {m['no_event']:.3f} ms, alternating {m['alternating']:.3f} ms, torch int32 {m['torch']:.3f} ms "
          f"({m['torch'] / m['smooth']:.1f} x), general {m['general']:.3f} ms ({m['general'] / m['smooth']:.1f} x); {json.dumps(agree)}", flush=True)
    return result


def small(tag, M, T, F_, H, W, with_truth):
    """an input on which the kernel cannot fill the chip: the kernel, the torch route and the read rate"""
    torch.manual_seed(1)
    hw, D = H * W, M + (1 if with_truth else 0)
    v = ar1(M, T, F_, H, W)
    x = v[1:].contiguous().view(M, T, F_, hw)
    y = v[0].contiguous().view(T, F_, hw) if with_truth else None
    thr = torch.tensor([[0.5, 1.6]], device=dev).expand(F_, K).contiguous()
    above = torch.ones(F_, K, dtype=torch.int32, device=dev)
    tk, tt_ = Tables(D, F_, hw), Tables(D, F_, hw)
    routes = {"kernel": lambda: kernel_call(x, y, thr, above, tk, M, T, F_, hw, 0), "torch": lambda: update_torch(x, y, thr, tt_, 0),
              "read": (lambda: (x.sum(), y.sum())) if with_truth else (lambda: x.sum())}
    for fn in routes.values():
        timed(fn, 1)
    equal = all(bool(torch.equal(p, q)) for p, q in zip(tk.all()[:3], tt_.all()[:3]))
    ms = {k: [] for k in routes}
    for _ in range(ROUNDS):
        for name, fn in routes.items():
            ms[name].append(timed(fn, 2 if name == "torch" else ITERS))
    in_bytes = D * T * F_ * hw * 4
    read_gbs = in_bytes / (statistics.median(ms["read"]) * 1e-3) / 1e9
    result = dict(config=tag, members=M, times=T, vars=F_, grid=[H, W], workgroups=D * F_ * ((hw + 1023) // 1024), input_bytes=in_bytes,
                  measured_read_GBps=round(read_gbs, 1), kernel_equal_torch=equal, routes={k: record(tag, k, ms[k], in_bytes, read_gbs) for k in routes})
    m = {k: r["ms_median"] for k, r in result["routes"].items()}
    print(f"spells {tag}: kernel {m['kernel']:.3f} ms in {result['workgroups']} workgroups ({result['routes']['kernel']['input_GBps']:.0f} GB/s), "
          f"torch int32 {m['torch']:.3f} ms ({m['torch'] / m['kernel']:.1f} x), read {m['read']:.3f} ms; equal {equal}", flush=True)
    return result


def main():
    results = [one(M, T) for M, T in SHAPES]
    results.append(small("one_row", 1, 2048, 1, 128, 128, False))
    results.append(small("coarse", 8, 8760, 4, 8, 8, True))
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
