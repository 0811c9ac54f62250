"""Temporal increment scores of an ensemble on the device: what every member does from one hour to a later one, against what the truth
does.  Every other score here judges one ``(t, f)`` plane at a time; none compares a field at ``t`` with the same field at ``t + tau``.
The reference notes that only this method downscales in time (exp/metrics.py:237-240) and conditions on every ``t_step``-th hour
(exp/downscaling.py:131-132); its only temporal evidence is a plot of two grid cells over time (exp/figures.py::timeseries).  Three
questions follow from one small table of sums over increments:

1. do the members vary from hour to hour as much as the truth does, at every lag -- or are they too smooth, or too jittery, between the
   observations?  (``structure_functions``, ``variability_ratio``)
2. how wrong is each member's tendency ``x(t + tau) - x(t)`` against the truth's?  (``tendency_rmse``)
3. does the trajectory jump at the observation times, the known failure of a sampler guided every ``t_step`` hours?  (``by_phase``)

``run_ensemble`` leaves ``(M, L, F, H, W)`` on the device, and here it stays there: one HIP kernel (csrc/temporal.hip) forms every
increment in fp32 and sums in double in a fixed order, where torch keeps a temporary of the tensor's size per lag.

**The definitions**, in this project's words (include/c2w_hip.h: c2w_tincr_terms); they are elementary and checked by known answers
(README, statement 11).  fp32 inputs are read as exact numbers.  The rows are ``r_0`` = the truth, when one is given, then
``r_1 .. r_n`` = the data sets; ``D`` counts them.  For row ``d``, anchor ``t``, variable ``f`` and lag ``tau = 1 .. L`` with
``t + tau < T``, over the ``H W`` cells ``c``:

* ``dx_c = r_d[t + tau, f, c] - r_d[t, f, c]``, ``dy_c`` the same increment of the truth
* ``S[d, t, f, tau - 1] = (sum_c |dx_c|, sum_c dx_c^2, sum_c (dx_c - dy_c)^2)`` = ``(A1, A2, E2)`` -- the kernel's product, float64
  (``increment_terms``)
* the truth's own row has ``E2 = +0``; without a truth column 2 is ``+0``; an entry with ``t + tau >= T`` has no pair and is ``+0`` in
  all three columns
* ``S_p(tau) = sum_t A_p / ((T - tau) H W)``, ``p`` in {1, 2}: the structure functions; NaN where ``T <= tau``
* the variability ratio of member to truth, ``sqrt(S_2^m / S_2^y)`` at order 2 and ``S_1^m / S_1^y`` at order 1: 1 is the right
  hour-to-hour variability, below 1 is too smooth in time
* the tendency RMSE ``sqrt(sum_t E2 / ((T - tau) H W))``
* by phase: the means of the three columns over the anchors with ``(t - offset) mod period == phi`` that have a pair.  With
  ``period = t_step`` a jump at the observation times shows as a peak at lag 1 for ``phi = period - 1``.

A NaN or an infinity in plane ``(d, t, f)`` makes exactly the entries ``(d, t, f, tau)`` that have a pair and ``(d, t - tau, f, tau)``
NaN, and in a truth plane also column 2 of the same entries of every row; no other entry is touched.

On the GPU the kernel takes ``H W`` a multiple of 4 and ``1 <= max_lag <= 24``; everything else and CPU tensors take the same
definition in float64 torch, chunked over time.  Error of the kernel against float64 (tests/fp64_temporal_ref.py): ``A1`` within
``2 * 2^-24`` and ``A2`` within ``3 * 2^-24`` of themselves, ``E2`` within ``6 * 2^-24 sum (|dx| + |dy|)^2``.  No value of ``max_lag`` or
``period`` is the reference's, beyond its ``t_step``.

Nothing here synchronises.

Out of scope: increments in space (``multivariate.py`` has the variogram), spectra in time, lagged correlations, collectives -- members
are rank-local -- and the plotting.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import temporal_ops
from .ensemble_host import VariableReport, check_ensemble, chunk_step, datasets, member_mean_std, scratch, variable_names
from .ensemble_host import on_device as _on_device

NAN = float("nan")


def _check_lag(max_lag: int) -> int:
    L = int(max_lag)
    if L < 1:
        raise ValueError(f"max_lag {max_lag} must be at least 1")
    return L


def _general(x: torch.Tensor, y: Optional[torch.Tensor], S: torch.Tensor, L: int) -> None:
    """The definition for any shape, any lag and any device, float64 end to end: x (n_rep, T, F, hw), y (T, F, hw) or None,
    S (D, T, F, L, 3)."""
    T, F, hw = (int(s) for s in x.shape[1:])
    D = int(S.shape[0])
    S.zero_()
    step = chunk_step(D * F * hw)
    for t0 in range(0, T - 1, step):
        hi = min(T, t0 + step + L)  # the anchors t0 .. t0 + step - 1 and the planes their lags reach
        rows = x[:, t0:hi].double() if y is None else torch.cat([y[None, t0:hi], x[:, t0:hi]]).double()  # (D, t, F, hw)
        bad = ~torch.isfinite(rows).all(dim=-1)                                                            # (D, t, F)
        rows = torch.where(bad[..., None], torch.zeros_like(rows), rows)                                   # the rule below writes those entries
        for tau in range(1, min(L, hi - t0 - 1) + 1):
            n = min(step, hi - t0 - tau)
            dx = rows[:, tau:tau + n] - rows[:, :n]
            touched = bad[:, tau:tau + n] | bad[:, :n]
            cols = [dx.abs().sum(dim=-1), (dx * dx).sum(dim=-1)]
            if y is None:
                cols.append(torch.zeros_like(cols[0]))
                poisoned = torch.stack([touched, touched, torch.zeros_like(touched)], dim=-1)
            else:
                e = dx - dx[:1]
                cols.append((e * e).sum(dim=-1))
                poisoned = torch.stack([touched, touched, touched | touched[:1]], dim=-1)
            out = torch.stack(cols, dim=-1)                                                                # (D, n, F, 3)
            S[:, t0:t0 + n, :, tau - 1] = torch.where(poisoned, torch.full_like(out, NAN), out)


def _launch(x, y, S, n_rep, T, F, hw, L) -> bool:
    if not temporal_ops.tincr_supported(hw, L):
        return False
    rows = n_rep + (0 if y is None else 1)
    return temporal_ops.tincr_terms(x, y, S, scratch(temporal_ops.tincr_scratch_bytes(rows, T, F, hw, L), x.device), n_rep, T, F, hw, L)


def increment_terms(samples: torch.Tensor, truth: Optional[torch.Tensor] = None, max_lag: int = 6) -> torch.Tensor:
    """``samples (..., T, F, H, W)``, one data set per leading index, and ``truth (T, F, H, W)`` or None -> ``S (D, T, F, L, 3)`` float64
    on the same device, ``L = max_lag``: per row, anchor time, variable and lag the sums over the cells of ``(|dx|, dx^2, (dx - dy)^2)``
    (module docstring).  Row 0 is the truth when one is given, the data sets follow: ``D`` is their number, plus one with a truth.  Any
    float dtype and any strides: a strided or 16-bit input costs one dense fp32 copy.

    On the GPU, ``H W`` a multiple of 4 and ``max_lag <= 24`` take the kernel; everything else and CPU tensors take the same definition
    in float64."""
    L = _check_lag(max_lag)
    if not samples.is_floating_point() or (truth is not None and not truth.is_floating_point()):
        raise ValueError(f"samples ({samples.dtype}) and truth ({None if truth is None else truth.dtype}) must be floating point")
    x, y, _ = datasets(samples, truth)
    n_rep, T, F, hw = (int(s) for s in x.shape)
    D = n_rep + (0 if y is None else 1)
    S = torch.empty((D, T, F, L, 3), dtype=torch.float64, device=x.device)
    if S.numel() == 0:
        return S
    if n_rep == 0 or hw == 0:
        return S.zero_()
    if not (_on_device(x) and _launch(x, y, S, n_rep, T, F, hw, L)):
        _general(x, y, S, L)
    return S


def pair_counts(T: int, max_lag: int, device=None) -> torch.Tensor:
    """``(L,)`` float64: the anchors ``T - tau`` that have a pair at lag ``tau = 1 .. L``, 0 where ``T <= tau``"""
    return torch.tensor([max(0, T - tau) for tau in range(1, max_lag + 1)], dtype=torch.float64, device=device)


def _pooled(terms: torch.Tensor, hw: int) -> torch.Tensor:
    """(D, T, F, L, 3) -> (D, F, L, 3): the means over the pairs of every lag and the cells; 0 / 0 = NaN where a lag has no pair"""
    T, L = int(terms.shape[1]), int(terms.shape[3])
    return terms.sum(dim=1) / (pair_counts(T, L, terms.device) * hw)[None, None, :, None]


def _hw(samples: torch.Tensor) -> int:
    return int(samples.shape[-2]) * int(samples.shape[-1])


def structure_functions(samples: torch.Tensor, truth: Optional[torch.Tensor] = None, max_lag: int = 6) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(S_1, S_2)``, each ``(D, F, L)`` float64: ``S_p(tau) = sum_t A_p / ((T - tau) H W)``, the mean of ``|dx|^p`` over every pair of
    hours ``tau`` apart and every cell, per row (row 0 the truth when one is given).  NaN where ``T <= tau``."""
    pooled = _pooled(increment_terms(samples, truth, max_lag), _hw(samples))
    return pooled[..., 0], pooled[..., 1]


def _ratio_of(pooled: torch.Tensor, order: int) -> torch.Tensor:
    if order == 2:
        return torch.sqrt(pooled[1:, ..., 1] / pooled[:1, ..., 1])
    if order == 1:
        return pooled[1:, ..., 0] / pooled[:1, ..., 0]
    raise ValueError(f"order {order} must be 1 or 2")


def variability_ratio(samples: torch.Tensor, truth: torch.Tensor, max_lag: int = 6, order: int = 2) -> torch.Tensor:
    """``(M, F, L)`` float64: member over truth, ``sqrt(S_2^m / S_2^y)`` at ``order=2`` and ``S_1^m / S_1^y`` at ``order=1``.  1 is the
    right hour-to-hour variability, below 1 is too smooth in time.  NaN where the truth does not move at all."""
    if order not in (1, 2):
        raise ValueError(f"order {order} must be 1 or 2")
    check_ensemble(samples, truth, floating=True)
    return _ratio_of(_pooled(increment_terms(samples, truth, max_lag), _hw(samples)), order)


def tendency_rmse(samples: torch.Tensor, truth: torch.Tensor, max_lag: int = 6) -> torch.Tensor:
    """``(M, F, L)`` float64: ``sqrt(sum_t E2 / ((T - tau) H W))``, the root-mean-square error of every member's increment over ``tau``
    hours against the truth's, in the variable's unit."""
    check_ensemble(samples, truth, floating=True)
    return torch.sqrt(_pooled(increment_terms(samples, truth, max_lag), _hw(samples))[1:, ..., 2])


def by_phase(terms: torch.Tensor, period: int, offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """``terms (D, T, F, L, 3)`` from ``increment_terms`` -> ``(means (D, period, F, L, 3), counts (period, L))`` float64: the means of
    the three columns over the anchors ``t`` with ``(t - offset) mod period == phi`` that have a pair at the lag, and how many those
    are; NaN where there is none.  The means are of the plane sums: divide by ``H W`` for a mean per cell.  With ``period = t_step`` and
    the observations at ``offset, offset + period ..`` the anchor right before an observation has ``phi = period - 1``: a jump at the
    observation times is a peak there at lag 1."""
    if terms.dim() != 5 or int(terms.shape[-1]) != 3:
        raise ValueError(f"terms {tuple(terms.shape)} must be (D, T, F, L, 3)")
    period = int(period)
    if period < 1:
        raise ValueError(f"period {period} must be at least 1")
    D, T, F, L, _ = (int(s) for s in terms.shape)
    sums = torch.zeros((D, period, F, L, 3), dtype=torch.float64, device=terms.device)
    counts = []
    for phi in range(period):
        first = (phi + int(offset)) % period
        sums[:, phi] = terms[:, first::period].sum(dim=1)  # an anchor without a pair holds zeros
        counts.append([sum(1 for t in range(first, T, period) if t + tau < T) for tau in range(1, L + 1)])
    counts = torch.tensor(counts, dtype=torch.float64, device=terms.device).view(period, L)
    return sums / counts[None, :, None, :, None], counts


class TemporalReport(VariableReport):
    """Per variable, as device tensors over the lags ``1 .. L``: ``structure_1_truth``, ``structure_2_truth (L,)``, ``structure_1``,
    ``structure_2``, ``ratio_1``, ``ratio_2``, ``tendency_rmse (M, L)``; with a ``period`` also ``phase_mean (D, period, L, 3)`` -- the
    means per cell, row 0 the truth -- and ``phase_count (period, L)``."""

    KEYS = ("ratio_1", "ratio_2", "tendency_rmse")

    def as_dict(self, prefix: str = "temporal") -> dict:
        """flat ``{f"{prefix}/{name}/{key}_lag1": mean over the members, ..."_std": their population std}`` for a logger, ``key`` in
        ``KEYS``, at lag 1 (one device-to-host copy)"""
        if not self.variables:
            return {}
        return member_mean_std([v[k][:, 0] for v in self.variables for k in self.KEYS],
                               [f"{prefix}/{name}/{k}_lag1" for name in self.names for k in self.KEYS])


def temporal_report(samples: torch.Tensor, truth: torch.Tensor, names: Optional[Sequence[str]] = None, max_lag: int = 6,
                    period: Optional[int] = None) -> TemporalReport:
    """The temporal scores of an ensemble ``samples (M, L, F, H, W)`` against ``truth (L, F, H, W)`` per variable, from one pass of the
    kernel over the fields.  The fields are expected DE-NORMALISED, as the reference's are: structure functions and tendency RMSE
    carry the variable's unit.  ``period``: the observation period ``t_step`` of a conditioned run, for the means by phase.  ``names``:
    one per variable, default ``var0 ...``."""
    check_ensemble(samples, truth, time="L", members="M >= 1", floating=True)
    F, hw = int(samples.shape[2]), _hw(samples)
    names = variable_names(names, F)
    terms = increment_terms(samples, truth, max_lag)
    pooled = _pooled(terms, hw)  # (M + 1, F, L, 3)
    r1, r2, rmse = _ratio_of(pooled, 1), _ratio_of(pooled, 2), torch.sqrt(pooled[1:, ..., 2])
    phase = by_phase(terms, period) if period is not None else None
    variables = []
    for f in range(F):
        v = dict(structure_1_truth=pooled[0, f, :, 0], structure_2_truth=pooled[0, f, :, 1], structure_1=pooled[1:, f, :, 0],
                 structure_2=pooled[1:, f, :, 1], ratio_1=r1[:, f], ratio_2=r2[:, f], tendency_rmse=rmse[:, f])
        if phase is not None:
            v.update(phase_mean=phase[0][:, :, f] / hw, phase_count=phase[1])
        variables.append(v)
    return TemporalReport(names, variables)
