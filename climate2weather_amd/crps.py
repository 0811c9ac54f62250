"""Ensemble CRPS and spread-skill on the device: the continuous ranked probability score of the M members of every cell against that
cell's truth, the proper score a probabilistic downscaler is judged by first, and the pair that goes with it -- the RMSE of the ensemble
mean and the ensemble spread.  The rank histogram of ``marginals.py`` says whether an ensemble is calibrated; these say how good it is.

``run_ensemble`` leaves ``(M, L, F, H, W)`` on the device, and here it stays there: one HIP kernel (csrc/crps.hip) sorts the members of
every cell in registers and reads every value once, where the torch route sorts along the member axis of the whole tensor and keeps
several temporaries of its size.

**The definitions**, in this project's words (include/c2w_hip.h: c2w_crps_terms).  One cell ``(t, f, c)`` has the members
``x_1 .. x_M`` and the truth ``y``; four non-negative terms per cell:

* ``A = (1/M) sum_m |x_m - y|``
* ``B = sum_{m<m'} |x_m - x_m'|``; with the members sorted, ``sum_{k=1}^{M-1} k (M-k) (x_(k+1) - x_(k))``
* ``E = (mean_m x_m - y)^2``
* ``V = sum_m (x_m - mean x)^2 / (M - 1)``; NaN for ``M = 1``

and from their means over the cells of a ``(t, f)`` plane, or over any larger set:

* ``crps = mean A - mean B / M^2``, the empirical-CDF form ``integral (F_M(z) - 1[z >= y])^2 dz``.  ``properscoring`` and ``xskillscore``
  are not at hand, so the form is verified, not recalled: tests/test_crps_cpu.py evaluates the integral exactly in float64.
* ``crps_fair = mean A - mean B / (M (M-1))``; NaN for ``M = 1``
* ``rmse = sqrt(mean E)``, ``spread = sqrt(mean V)``
* ``ratio = sqrt((M+1)/M) * spread / rmse``; 1 for a statistically consistent ensemble.  The factor is a stated choice (README,
  statement 8) and ``consistency_factor`` below is the one place that holds it.

A member or a truth that is NaN or infinite makes the four terms of its cell, and with them the four sums of its ``(t, f)`` entry, NaN;
no other entry is touched.

**The trap.**  A pressure field lies at 101 325 +- 1200 and its members differ by 0.05 - 3: the mean and the variance of the raw fp32
values put ``V`` off by orders of magnitude and ``E`` far beyond its bound.  The kernel forms only differences of nearby numbers and sums
of non-negative terms: ``B`` from the gaps of the sorted members, ``V`` and ``E`` from offsets against the middle order statistic.  Per
cell the error is at most ``(M + 16) 2^-24`` of the term (of ``A^2`` for ``E``); tests/fp64_crps_ref.py has the rule.

Nothing here synchronises.

Out of scope: weighted or thresholded CRPS, other multivariate scores (``multivariate.py`` has the energy score and the variogram
score), CRPS against a parametric forecast, the
plotting, more than 64 members on the kernel (the general route takes them), and collectives -- members are rank-local.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch

from . import ops
from .ensemble_host import VariableReport, check_ensemble, chunk_step, dense32, scratch, variable_names
from .ensemble_host import on_device as _on_device


def consistency_factor(M: int) -> float:
    """``sqrt((M + 1) / M)``: what ``spread / rmse`` is multiplied by so that a statistically consistent ensemble of M members gives 1
    (the truth is one more draw: the mean-square error of the ensemble mean is ``(1 + 1/M)`` times the variance)."""
    return math.sqrt((M + 1) / M) if M > 0 else float("nan")


def _general(x: torch.Tensor, y: torch.Tensor, sums: torch.Tensor, cells: Optional[torch.Tensor]) -> None:
    """The definition for any shape, any M and any device, float64 end to end: x (M, T, F, hw), y (T, F, hw), sums (T, F, 4), cells
    (4, T, F, hw) or None."""
    M, T, F, hw = x.shape
    nan = float("nan")
    if M == 0:
        sums.fill_(nan)
        if cells is not None:
            cells.fill_(nan)
        return
    k = torch.arange(1, M, dtype=torch.float64, device=x.device)
    w = (k * (M - k))[:, None, None, None]
    step = chunk_step(M * F * hw)
    for i in range(0, T, step):
        xs, ys = x[:, i:i + step].double(), y[i:i + step].double()
        ok = torch.isfinite(xs).all(dim=0) & torch.isfinite(ys)
        xs = torch.where(ok[None], xs, torch.zeros_like(xs))  # the rule below writes those cells; keep inf - inf out of the way
        ys = torch.where(ok, ys, torch.zeros_like(ys))
        a = (xs - ys[None]).abs().sum(dim=0) / M
        srt = torch.sort(xs, dim=0).values
        b = (w * (srt[1:] - srt[:-1])).sum(dim=0)
        mean = xs.sum(dim=0) / M
        e = (mean - ys) ** 2
        v = ((xs - mean[None]) ** 2).sum(dim=0) / (M - 1) if M > 1 else torch.full_like(e, nan)
        terms = torch.stack([a, b, e, v])                       # (4, t, F, hw)
        terms = torch.where(ok[None], terms, torch.full_like(terms, nan))
        sums[i:i + step] = terms.sum(dim=-1).permute(1, 2, 0)
        if cells is not None:
            cells[:, i:i + step] = terms.to(cells.dtype)


def _launch(x, y, sums, cells, M, T, F, hw) -> bool:
    if not ops.crps_supported(hw, M):
        return False
    return ops.crps_terms(x, y, sums, cells, scratch(ops.crps_scratch_bytes(T, F, hw), x.device), M, T, F, hw)


def ensemble_terms(samples: torch.Tensor, truth: torch.Tensor, *, cells: bool = False):
    """``samples (M, T, F, H, W)`` against ``truth (T, F, H, W)`` -> ``sums (T, F, 4)`` float64 on the same device: per ``(t, f)`` plane
    the sums over its cells of the four terms ``A, B, E, V`` (module docstring).  With ``cells=True`` the pair ``(sums, per-cell terms
    (4, T, F, H, W) fp32)`` -- maps of time-mean CRPS are the standard figure.  Any float dtype and any strides: a strided or 16-bit
    input costs one dense fp32 copy.

    On the GPU, ``H W`` a multiple of 4 and ``1 <= M <= 64`` take the kernel; everything else and CPU tensors take the same definition
    in float64.  No members (``M = 0``) gives NaN throughout."""
    check_ensemble(samples, truth, floating=True)
    M, T, F, H, W = (int(s) for s in samples.shape)
    hw = H * W
    x, y = dense32(samples).view(M, T, F, hw), dense32(truth).view(T, F, hw)
    sums = torch.empty((T, F, 4), dtype=torch.float64, device=x.device)
    per_cell = torch.empty((4, T, F, hw), dtype=torch.float32, device=x.device) if cells else None
    if T * F * hw == 0:
        sums.zero_()
    elif not (_on_device(x) and _launch(x, y, sums, per_cell, M, T, F, hw)):
        _general(x, y, sums, per_cell)
    return (sums, per_cell.view(4, T, F, H, W)) if cells else sums


def _crps_of(sum_a: torch.Tensor, sum_b: torch.Tensor, n: int, M: int, fair: bool) -> torch.Tensor:
    pairs = M * (M - 1) if fair else M * M
    return (sum_a - sum_b / pairs) / n if pairs > 0 else torch.full_like(sum_a, float("nan"))


def crps(samples: torch.Tensor, truth: torch.Tensor, *, fair: bool = False) -> torch.Tensor:
    """``(T, F)`` float64: the mean CRPS over the cells of every plane, ``mean A - mean B / M^2``, or with ``fair=True`` the fair form
    ``mean A - mean B / (M (M - 1))`` (NaN for ``M = 1``)."""
    sums = ensemble_terms(samples, truth)
    M, hw = int(samples.shape[0]), int(samples.shape[3]) * int(samples.shape[4])
    return _crps_of(sums[..., 0], sums[..., 1], hw, M, fair)


def _spread_skill_of(sum_e: torch.Tensor, sum_v: torch.Tensor, n: int, M: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    rmse, spread = torch.sqrt(sum_e / n), torch.sqrt(sum_v / n)
    return rmse, spread, consistency_factor(M) * spread / rmse


def spread_skill(samples: torch.Tensor, truth: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(rmse, spread, ratio)``, each ``(F,)`` float64 over all times and cells: the RMSE of the ensemble mean, the square root of the
    mean ensemble variance, and ``consistency_factor(M) * spread / rmse``."""
    sums = ensemble_terms(samples, truth)
    M, T, hw = int(samples.shape[0]), int(samples.shape[1]), int(samples.shape[3]) * int(samples.shape[4])
    tot = sums.sum(dim=0)
    return _spread_skill_of(tot[:, 2], tot[:, 3], T * hw, M)


class CrpsReport(VariableReport):
    """Per variable, as device tensors: ``crps``, ``crps_fair``, ``rmse``, ``spread``, ``ratio`` (0-d float64, over all times and cells)
    and ``crps_by_time (T,)``.  There is no ``all_variables``: a score in a variable's own unit has no meaning across units."""

    KEYS = ("crps", "crps_fair", "rmse", "spread", "ratio")

    def as_dict(self, prefix: str = "crps") -> dict:
        """flat ``{f"{prefix}/{name}/{key}": float}`` for a logger, ``key`` in ``KEYS`` (one device-to-host copy)"""
        if not self.variables:
            return {}
        table = torch.stack([torch.stack([v[k] for k in self.KEYS]) for v in self.variables]).cpu().numpy()
        return {f"{prefix}/{name}/{k}": float(table[i, j]) for i, name in enumerate(self.names) for j, k in enumerate(self.KEYS)}


def crps_report(samples: torch.Tensor, truth: torch.Tensor, names: Optional[Sequence[str]] = None) -> CrpsReport:
    """The scores of an ensemble ``samples (M, L, F, H, W)`` against ``truth (L, F, H, W)`` per variable, from one pass over the fields.
    The fields are expected DE-NORMALISED, as the reference's are: CRPS, RMSE and spread carry the variable's unit.  ``names``: one per
    variable, default ``var0 ...``."""
    check_ensemble(samples, truth, floating=True)
    M, T, F, H, W = (int(s) for s in samples.shape)
    names = variable_names(names, F)
    sums = ensemble_terms(samples, truth)
    hw = H * W
    tot = sums.sum(dim=0)  # (F, 4)
    score, fair = _crps_of(tot[:, 0], tot[:, 1], T * hw, M, False), _crps_of(tot[:, 0], tot[:, 1], T * hw, M, True)
    rmse, spread, ratio = _spread_skill_of(tot[:, 2], tot[:, 3], T * hw, M)
    by_time = _crps_of(sums[..., 0], sums[..., 1], hw, M, False)  # (T, F)
    variables = [dict(crps=score[f], crps_fair=fair[f], rmse=rmse[f], spread=spread[f], ratio=ratio[f], crps_by_time=by_time[:, f]) for f in range(F)]
    return CrpsReport(names, variables)
