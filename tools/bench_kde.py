#!/usr/bin/env python3
"""Throughput of the marginals kernels (csrc/kde.hip) against the torch routes, in one process, with device events.

    python tools/bench_kde.py            (MEMBERS=8 TIMES=256 VARS=4 N=1000 ROUNDS=3 ITERS=3; OUT=path also writes the JSON there)

Timed, alternately, ROUNDS blocks of ITERS calls each, on MEMBERS x TIMES x VARS fields of 128 x 128 against TIMES x VARS truth fields:
D = MEMBERS VARS + VARS data sets of n = TIMES x 16384 values each, N grid points:
  partial       ops.kde_partial: kde_partial_kernel, one launch over all D data sets -- D n N Gaussian evaluations
  fold          ops.kde_fold: kde_fold_kernel
  kernels       what marginals.gaussian_kde enqueues after the bandwidths: both launches
  pit           ops.pit_counts: the memset and pit_count_kernel; its bytes are the samples and the truth, each read once
  torch_fp32    the same densities through torch in fp32: the pivoted x - c and offsets, torch.exp, sums folded in float64
  general       marginals._general: the package's own float64 route (one call per round)
  pit_torch     marginals._pit_general: the comparison, the sum over members and a scatter_add
  read          torch's sum over the samples: the HBM read rate of this box, against which the rank histogram's rate is a share
The modelled ceiling of the density kernel is issue-bound: per 64 pairs a SIMD issues three plain vector instructions and one
v_exp_f32, 4 + 4 + 4 + 8 = 20 cycles for one wave alone, so CUs x 4 SIMDs x 64 lanes / 20 cycles x 2.4 GHz = 7.9e12 pairs/s on 256 CUs.
One JSON line per route, then a summary."""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from climate2weather_amd import marginals as Mg
from climate2weather_amd import ops

M, T, F = int(os.environ.get("MEMBERS", "8")), int(os.environ.get("TIMES", "256")), int(os.environ.get("VARS", "4"))
N = int(os.environ.get("N", "1000"))
ROUNDS, ITERS = int(os.environ.get("ROUNDS", "3")), int(os.environ.get("ITERS", "3"))
H = W = 128
CYCLES_PER_64_PAIRS, CLOCK_HZ = 20.0, 2.4e9
MEASURED_READ_TBPS = (3.7, 3.9)  # profiles/ssim_measurements.md, profiles/spectra_measurements.md
dev = torch.device("cuda:0")


def torch_fp32(x, y, offsets, pivot, h, dens, block=1 << 15):
    """x (M, T, F, hw), y (T, F, hw): per data set, `block` values at a time against all N points, everything fp32 until a block's sum"""
    n_rep, T_, F_, hw = x.shape
    n = T_ * hw
    for ds in range(dens.shape[0]):
        f = ds % F_ if ds < n_rep * F_ else ds - n_rep * F_
        v = (x[ds // F_, :, f] if ds < n_rep * F_ else y[:, f]).reshape(-1)
        inv = (1.0 / h[ds]).float()
        s = torch.zeros(dens.shape[1], dtype=torch.float64, device=x.device)
        for i in range(0, n, block):
            u = (offsets[f][None, :] - (v[i:i + block] - pivot[f])[:, None]) * inv
            s += torch.exp(-0.5 * u * u).sum(dim=0).double()
        dens[ds] = s / (n * h[ds] * math.sqrt(2.0 * math.pi))


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
    hw, n, D = H * W, T * H * W, M * F + F
    off = torch.tensor([101325.0, 280.0, 0.0, 3.0], device=dev)[:F] if F <= 4 else torch.zeros(F, device=dev)
    sd = torch.tensor([1200.0, 10.0, 4.0, 4.0], device=dev)[:F] if F <= 4 else torch.ones(F, device=dev)
    y = off[None, :, None] + sd[None, :, None] * torch.randn(T, F, hw, device=dev)
    x = (off[None, None, :, None] + 1.1 * sd[None, None, :, None] * torch.randn(M, T, F, hw, device=dev)).contiguous()
    grid = Mg.report_grid(x.view(M, T, F, H, W), y.view(T, F, H, W), N)
    h = torch.cat([Mg.bandwidth(x.view(M, T, F, H, W)).reshape(-1), Mg.bandwidth(y.view(T, F, H, W))]).contiguous()
    pivot = (0.5 * (grid[:, 0] + grid[:, -1])).float()
    offsets = (grid - pivot.double()[:, None]).float().contiguous()
    scratch = torch.empty(ops.kde_scratch_bytes(D, n, N) // 8, dtype=torch.float64, device=dev)
    dens, dens32, dens64 = (torch.empty(D, N, dtype=torch.float64, device=dev) for _ in range(3))
    counts, counts_t = (torch.empty(F, M + 1, dtype=torch.int64, device=dev) for _ in range(2))

    def kernels():
        assert ops.kde_eval(x, y, offsets, pivot, h, scratch, dens, M, T, F, hw, N)

    routes = {
        "partial": lambda: ops.kde_partial(x, y, offsets, pivot, h, scratch, M, T, F, hw, N),
        "fold": lambda: ops.kde_fold(scratch, h, dens, D, n, N),
        "kernels": kernels,
        "pit": lambda: ops.pit_counts(x, y, counts, M, T, F, hw),
        "torch_fp32": lambda: torch_fp32(x, y, offsets, pivot, h, dens32),
        "general": lambda: Mg._general(x, y, grid, h, dens64),
        "pit_torch": lambda: Mg._pit_general(x, y, counts_t),
        "read": lambda: x.sum(),
    }
    slow = ("torch_fp32", "general")
    ms = {k: [] for k in routes}
    for name, fn in routes.items():  # warm-up: code objects, allocator; the slow routes' warm-up call is their agreement run too
        timed(fn, 1 if name in slow else 2)
    peak = dens64.max(dim=1, keepdim=True).values
    agree32 = float(((dens - dens32).abs() / peak).max())
    agree64 = float(((dens - dens64).abs() / peak).max())
    pit_equal = bool(torch.equal(counts, counts_t))
    for _ in range(ROUNDS):
        for name, fn in routes.items():
            if name in slow and ms[name]:
                continue  # one timed call each: seconds
            ms[name].append(timed(fn, 1 if name in slow else ITERS))
    pairs = float(D) * n * N
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    model = cus * 4 * 64 / CYCLES_PER_64_PAIRS * CLOCK_HZ
    pit_bytes = (M + 1) * T * F * hw * 4
    read_gbs = x.numel() * 4 / (statistics.median(ms["read"]) * 1e-3) / 1e9
    result = {"members": M, "times": T, "vars": F, "N": N, "data_sets": D, "values_per_set": n, "rounds": ROUNDS, "iters": ITERS,
              "max_abs_over_peak_kernels_vs_torch_fp32": agree32, "max_abs_over_peak_kernels_vs_general": agree64,
              "pit_kernel_equals_torch": pit_equal, "compute_units": cus, "modelled_pairs_per_s": model, "routes": {}}
    for name in routes:
        med = statistics.median(ms[name])
        r = dict(route=name, ms_median=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4))
        if name in ("partial", "kernels", "torch_fp32", "general"):
            rate = pairs / (med * 1e-3)
            r.update(gaussian_evaluations_per_s=float(f"{rate:.4g}"), share_of_modelled_issue_bound=round(rate / model, 3))
        if name in ("pit", "pit_torch", "read"):
            gbs = (pit_bytes if name != "read" else x.numel() * 4) / (med * 1e-3) / 1e9
            r.update(input_GBps=round(gbs, 1), share_of_measured_read=round(gbs / read_gbs, 3),
                     share_of_3p7_to_3p9_TBps=[round(gbs / (1e3 * b), 3) for b in MEASURED_READ_TBPS])
        result["routes"][name] = r
        print(json.dumps(r), flush=True)
    k, t32, g = (result["routes"][r]["ms_median"] for r in ("kernels", "torch_fp32", "general"))
    p, pt = result["routes"]["pit"]["ms_median"], result["routes"]["pit_torch"]["ms_median"]
    print(f"kernels {k:.3f} ms vs torch_fp32 {t32:.3f} ms ({t32 / k:.2f} x) and general {g:.3f} ms ({g / k:.2f} x); pit {p:.3f} ms vs torch "
          f"{pt:.3f} ms ({pt / p:.2f} x), equal counts {pit_equal}; measured read rate {read_gbs:.0f} GB/s; densities: kernels vs torch_fp32 "
          f"{agree32:.2e}, vs general {agree64:.2e} of the peak")
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
