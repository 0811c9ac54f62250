"""Ensemble marginals and calibration on the device: the Gaussian kernel density estimate of every member's and the truth's values per
variable, and the probability-integral-transform (rank) histogram of the truth within the ensemble -- the two halves of the reference's
calibration figure, ``exp/figures.py::kde_and_pmf`` (lines 23-241).

The reference calls ``scipy.stats.gaussian_kde`` on all values of a variable -- 1457 hours of 128 x 128 cells are 2.4e7 values -- and
evaluates it at 1000 points, for the truth and for each member (:52-80): 2.4e10 Gaussians per data set, which is why it caches the result
in ``kde_1000.npz``.  ``run_ensemble`` leaves ``(M, L, F, H, W)`` on the device, and here it stays there: one HIP kernel (csrc/kde.hip)
evaluates the same exact direct sum for every (member, variable) and (truth, variable) in one launch, a second one adds its partial sums
in a fixed order, a third one counts the ranks in one read of every field.

**The definitions**, in this project's words (include/c2w_hip.h: c2w_kde_eval, c2w_pit_counts).  The KDE formula is verified against the
installed ``scipy.stats.gaussian_kde`` (tests/test_kde_cpu.py prints the agreement); the rank count is the reference's own line of numpy.

* KDE of values ``x_1 .. x_n`` at a point ``g``: ``f(g) = (1 / (n h sqrt(2 pi))) * sum_i exp(-(g - x_i)^2 / (2 h^2))`` with
  ``h = factor * std(x, ddof=1)``; ``factor = n^(-1/5)`` (``"scott"``, scipy's default), ``(3 n / 4)^(-1/5)`` for ``"silverman"``, and a
  number is taken as the factor itself.  One data set is one (member, variable) or (truth, variable) over all times and cells; every
  data set has its own ``h``.  The report's grid per variable is ``linspace(min(truth.min, samples.min), max(truth.max, samples.max), N)``
  in float64 (:52-60).
* PIT: for every (time, variable, cell) ``r = #{m : sample_m <= truth}`` with IEEE ``<=`` -- ties count, a NaN on either side compares
  false, as in numpy -- and ``counts[f][r]``, ``r = 0 .. M``, int64.  The reference's PIT value is ``r / M`` (:86) and its histogram with
  ``density=True`` over the ``M + 1`` bins of :185-190 is ``counts * M / counts.sum()``.

**The trap.**  A pressure field lies at 101 325 +- 1200 and with ``n`` in the millions ``h`` is a few tens: rounding a float64 grid point
to fp32 moves it by up to 0.004, 1e-4 of ``h``, several 1e-4 relative in a tail term.  The kernel is handed an fp32 pivot near the middle
of the grid and the grid as offsets from it, computed in float64 and rounded once, and forms ``x - pivot`` in fp32 on the loaded value
before anything else touches it.

Nothing here synchronises.  A NaN or inf value makes the density of its own data set NaN (the whole row) and touches no other; a
degenerate data set (``n < 2``, zero spread) gives what the formula gives, a NaN row, where scipy raises -- raising would need a sync.

Out of scope: weights, multivariate KDE, truncated or binned KDE, the plotting, more than 1024 grid points on the kernel (the general
route takes them), and collectives -- members are rank-local.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import ops
from .ensemble_host import VariableReport, check_ensemble, chunk_step, datasets, dense32, scratch, variable_names
from .ensemble_host import on_device as _on_device


def _factor(n: int, bw_method) -> float:
    if bw_method is None or bw_method == "scott":
        return float(n) ** -0.2 if n > 0 else float("nan")
    if bw_method == "silverman":
        return (0.75 * n) ** -0.2 if n > 0 else float("nan")
    if isinstance(bw_method, (int, float)) and not isinstance(bw_method, bool):
        return float(bw_method)
    raise ValueError(f"bw_method {bw_method!r}: 'scott', 'silverman' or a number")


def bandwidth(values: torch.Tensor, bw_method="scott") -> torch.Tensor:
    """``values (..., T, F, H, W)`` -> ``h (..., F)`` float64 on the same device: per data set ``factor * std(ddof=1)`` over everything
    but the leading dimensions and F, the mean and the sum of squares in float64, two passes in chunks of bounded size, no host sync.
    ``n < 2`` gives NaN, zero spread gives 0."""
    if values.dim() < 4:
        raise ValueError(f"values {tuple(values.shape)} must be (..., T, F, H, W)")
    lead = tuple(values.shape[:-4])
    T, F, H, W = (int(s) for s in values.shape[-4:])
    n = T * H * W
    factor = _factor(n, bw_method)
    x = values.reshape((-1, T, F, H * W))
    R = int(x.shape[0])
    mean = x.sum(dim=(1, 3), dtype=torch.float64) / n
    ss = torch.zeros((R, F), dtype=torch.float64, device=values.device)
    step = chunk_step(R * F * H * W)
    for i in range(0, T, step):
        ss += ((x[:, i:i + step].double() - mean[:, None, :, None]) ** 2).sum(dim=(1, 3))
    return (factor * torch.sqrt(ss / (n - 1))).view(lead + (F,))


def _general(x: Optional[torch.Tensor], y: Optional[torch.Tensor], grid: torch.Tensor, h: torch.Tensor, dens: torch.Tensor) -> None:
    """The definition for any shape, any N and any device, float64 end to end: x (n_rep, T, F, hw), y (T, F, hw) or None, grid (F, N),
    h (D,), dens (D, N)."""
    n_rep, T, F, hw = x.shape
    N = int(grid.shape[1])
    n = T * hw
    step = chunk_step(N)
    for ds in range(int(dens.shape[0])):
        f = ds % F if ds < n_rep * F else ds - n_rep * F
        v = (x[ds // F, :, f] if ds < n_rep * F else y[:, f]).reshape(-1)
        s = torch.zeros(N, dtype=torch.float64, device=dens.device)
        for i in range(0, n, step):
            u = (grid[f][None, :] - v[i:i + step].double()[:, None]) / h[ds]
            s += torch.exp(-0.5 * u * u).sum(dim=0)
        dens[ds] = s / (n * h[ds] * math.sqrt(2.0 * math.pi))


def _launch(x, y, grid, h, dens, n_rep, T, F, hw, N) -> bool:
    if not ops.kde_supported(hw, N):
        return False
    pivot = (0.5 * (grid[:, 0] + grid[:, -1])).to(torch.float32)
    offsets = (grid - pivot.double()[:, None]).to(torch.float32).contiguous()
    ws = scratch(ops.kde_scratch_bytes(int(dens.shape[0]), T * hw, N), x.device, optional=False)
    return ops.kde_eval(x, y, offsets, pivot, h, ws, dens, n_rep, T, F, hw, N)


def gaussian_kde(values: torch.Tensor, grid: torch.Tensor, *, bw_method="scott", truth: Optional[torch.Tensor] = None):
    """The Gaussian kernel density estimate of every data set of ``values (..., T, F, H, W)`` -- one per leading index and variable, over
    all times and cells -- at the points ``grid (F, N)`` float64, one row per variable: float64 of shape ``values.shape[:-4] + (F, N)`` on
    the same device (module docstring: the definition).  With ``truth (T, F, H, W)`` its F data sets ride in the same launch and the
    result is the pair ``(densities of values, densities of truth (F, N))``.  Any float dtype and any strides: a strided or 16-bit
    input costs one dense fp32 copy.

    On the GPU, ``H W`` a multiple of 4 and ``N <= 1024`` take the kernels; everything else and CPU tensors take the same definition in
    float64.  A data set with a NaN or inf value, fewer than two values or zero spread is NaN throughout."""
    if values.dim() < 4 or grid.dim() != 2 or int(grid.shape[0]) != int(values.shape[-3]) or int(grid.shape[1]) < 1:
        raise ValueError(f"values {tuple(values.shape)} must be (..., T, F, H, W) and grid {tuple(grid.shape)} (F, N) with N >= 1")
    x, y, lead = datasets(values, truth)
    T, F, H, W = (int(s) for s in values.shape[-4:])
    n_rep, hw, N = int(x.shape[0]), H * W, int(grid.shape[1])
    if T * hw < 1 or F < 1:
        raise ValueError("an empty data set has no density")
    grid = grid.to(device=x.device, dtype=torch.float64).contiguous()
    h = bandwidth(x.view(n_rep, T, F, H, W), bw_method).reshape(-1)
    if y is not None:
        h = torch.cat([h, bandwidth(y.view(T, F, H, W), bw_method)])
    h = h.contiguous()
    dens = torch.empty((int(h.shape[0]), N), dtype=torch.float64, device=x.device)
    if dens.shape[0] > 0 and not (_on_device(x) and _launch(x, y, grid, h, dens, n_rep, T, F, hw, N)):
        _general(x, y, grid, h, dens)
    out = dens[:n_rep * F].view(lead + (F, N))
    return out if truth is None else (out, dens[n_rep * F:])


def _pit_general(x: torch.Tensor, y: torch.Tensor, counts: torch.Tensor) -> None:
    """the reference's line for any shape and any device: x (M, T, F, hw), y (T, F, hw), counts (F, M + 1)"""
    M, T, F, hw = x.shape
    counts.zero_()
    bin0 = (torch.arange(F, device=x.device) * (M + 1))[None, :, None]
    step = chunk_step(M * F * hw)
    for i in range(0, T, step):
        r = (x[:, i:i + step] <= y[None, i:i + step]).sum(dim=0)  # (t, F, hw) int64
        counts.view(-1).scatter_add_(0, (r + bin0).reshape(-1), torch.ones(r.numel(), dtype=torch.int64, device=x.device))


def pit_counts(samples: torch.Tensor, truth: torch.Tensor) -> torch.Tensor:
    """``samples (M, T, F, H, W)`` against ``truth (T, F, H, W)`` -> ``counts (F, M + 1)`` int64 on the same device: per variable the
    number of (time, cell) at which exactly ``r`` members are ``<=`` the truth (module docstring).  ``counts.sum(-1) == T H W``.  On the
    GPU ``H W`` a multiple of 4 and ``M <= 64`` take the kernel."""
    check_ensemble(samples, truth, members="M >= 1")
    M, T, F, H, W = (int(s) for s in samples.shape)
    x, y = dense32(samples).view(M, T, F, H * W), dense32(truth).view(T, F, H * W)
    counts = torch.empty((F, M + 1), dtype=torch.int64, device=x.device)
    if T * F * H * W == 0:
        return counts.zero_()
    if not (_on_device(x) and ops.pit_counts(x, y, counts, M, T, F, H * W)):
        _pit_general(x, y, counts)
    return counts


def _pit_density(counts: torch.Tensor, M: int) -> torch.Tensor:
    return counts.double() * M / counts.sum(dim=-1, keepdim=True).double()


class MarginalsReport(VariableReport):
    """Per variable, what the reference's ``kde_and_pmf`` saves and draws, as device tensors: ``x (N,)`` the grid, ``gt (N,)`` the truth's
    density and ``samples (M, N)`` the members' (the three arrays of ``kde_1000.npz``, exp/figures.py:81-83); ``counts (M + 1,)`` int64
    the rank histogram and ``density (M + 1,)`` its ``density=True`` form (:180-192).  ``all_variables``: ``counts`` and ``density`` over
    all variables together (:226-241)."""

    def __init__(self, names: Sequence[str], variables: List[dict], all_variables: dict):
        super().__init__(names, variables)
        self.all_variables = all_variables

    def as_dict(self, prefix: str = "marginals") -> dict:
        """flat ``{name: float}`` for a logger (one device-to-host copy): per variable and for all variables together ``pit_mean``, the
        mean PIT value (1/2 for a calibrated ensemble) and ``pit_outside``, the share of cells whose truth lies below or above every
        member (``2 / (M + 1)`` for a calibrated one); per variable ``kde_l1``, the mean over the members of the integral of
        ``|f_member - f_truth|`` over the grid (trapezoid rule)."""
        rows = []
        for v in self.variables + [self.all_variables]:
            c = v["counts"].double()
            M = c.shape[0] - 1
            r = torch.arange(M + 1, dtype=torch.float64, device=c.device)
            row = [(c * r).sum() / (M * c.sum()), (c[0] + c[M]) / c.sum()]
            if "gt" in v:
                row.append(torch.trapezoid((v["samples"] - v["gt"][None]).abs(), v["x"][None], dim=-1).mean())
            else:
                row.append(torch.zeros((), dtype=torch.float64, device=c.device))
            rows.append(torch.stack(row))
        table = torch.stack(rows).cpu().numpy()
        out = {}
        for i, name in enumerate(self.names + ["all_variables"]):
            out[f"{prefix}/{name}/pit_mean"] = float(table[i, 0])
            out[f"{prefix}/{name}/pit_outside"] = float(table[i, 1])
            if name != "all_variables":
                out[f"{prefix}/{name}/kde_l1"] = float(table[i, 2])
        return out


def report_grid(samples: torch.Tensor, truth: torch.Tensor, n_points: int) -> torch.Tensor:
    """``(F, N)`` float64: per variable ``numpy.linspace(min(truth.min, samples.min), max(truth.max, samples.max), N)`` (exp/figures.py:
    52-60) with numpy's own arithmetic, ``arange(N) * step + start`` and the last point set to the stop."""
    lo = torch.minimum(samples.amin(dim=(0, 1, 3, 4)), truth.amin(dim=(0, 2, 3))).double()
    hi = torch.maximum(samples.amax(dim=(0, 1, 3, 4)), truth.amax(dim=(0, 2, 3))).double()
    if n_points == 1:
        return lo[:, None].clone()
    step = (hi - lo) / (n_points - 1)
    grid = torch.arange(n_points, dtype=torch.float64, device=truth.device)[None, :] * step[:, None] + lo[:, None]
    grid[:, -1] = hi
    return grid


def marginals_report(samples: torch.Tensor, truth: torch.Tensor, *, n_points: int = 1000, names: Optional[Sequence[str]] = None) -> MarginalsReport:
    """The calibration figure's numbers for an ensemble ``samples (M, L, F, H, W)`` against ``truth (L, F, H, W)`` as the reference
    computes them: the densities of the truth and of every member at ``n_points`` points between the joint minimum and maximum of each
    variable, and the rank histogram per variable and over all variables.  The fields are expected DE-NORMALISED, as the reference's
    are.  ``names``: one per variable, default ``var0 ...``."""
    check_ensemble(samples, truth, time="L", members="M >= 1")
    M, F = int(samples.shape[0]), int(truth.shape[1])
    names = variable_names(names, F)
    n_points = int(n_points)
    if n_points < 1:
        raise ValueError("n_points >= 1")
    s, g = dense32(samples), dense32(truth)
    grid = report_grid(s, g, n_points)
    dens_s, dens_g = gaussian_kde(s, grid, truth=g)  # (M, F, N), (F, N)
    counts = pit_counts(s, g)                        # (F, M + 1)
    density = _pit_density(counts, M)
    total = counts.sum(dim=0)
    variables = [dict(x=grid[f], gt=dens_g[f], samples=dens_s[:, f], counts=counts[f], density=density[f]) for f in range(F)]
    return MarginalsReport(names, variables, dict(counts=total, density=_pit_density(total, M)))
