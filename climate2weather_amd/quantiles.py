"""Exact quantiles on the device: the numbers the quantile normalisation is built from, and the tail diagnostic of an ensemble.

The reference computes them on the host: ``data/xarray_preproc.py::compute_quantiles`` calls ``xds.quantile([0.0, 0.01, 0.05, 0.25,
0.5, 0.75, 0.95, 0.99, 1.0], dim=["time", "rlat", "rlon"])``, a sort per variable over decades of hourly fields (the third step of
``data/cdo_preproc.sh``), and all five modes of ``data/pipeline.py::normalize_ds`` / ``unnormalize_ds`` read the result.  Here the
fields stay where they are: a radix select (csrc/quantile.hip) finds the two order statistics around every level in three reads of the
data, for every (member, variable) and (truth, variable) in one launch sequence on the current stream, without a host read-back.

**The definition**, in this project's words (include/c2w_hip.h: c2w_quantiles).  A data set is every value of one variable -- all times
and cells of one leading index.  With ``nv`` its number of non-NaN values and a level ``q`` in ``[0, 1]``: ``v = (nv - 1) q`` in
float64, ``lo = floor(v)``, ``hi = min(lo + 1, nv - 1)``, ``t = v - lo``, ``a`` and ``b`` the ``lo``-th and ``hi``-th smallest non-NaN
values (exact fp32), and the result is the float64 ``a + (b - a) t`` where ``t < 0.5`` and ``b - (b - a) (1 - t)`` where ``t >= 0.5``.
This is ``numpy.quantile(x.astype(float64), q)`` -- ``method="linear"`` with numpy's own ``_lerp`` -- checked against the installed
numpy by tests/test_quantiles_cpu.py; a zero result may carry either sign, and an infinite neighbour gives what numpy gives (NaN at
``q = 0`` when the minimum is ``-inf``).

``skipna`` is the one switch: ``True`` (the default) has the ``numpy.nanquantile`` meaning -- NaNs are counted and left out -- and
``False`` makes any NaN turn its data set's whole row NaN, as ``numpy.quantile`` does.  A data set without a valid value is a NaN row.
That ``xarray.Dataset.quantile(skipna=None)`` skips NaNs for float data is recalled, not verified (README, seventh statement).

Nothing here synchronises.  Out of scope: netCDF I/O, more than 16 levels on the kernel (the general route takes them), and
collectives -- members are rank-local.  Per-cell quantiles over time and quantile mapping are ``biascorrect.py``.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch

from . import ops
from .ensemble_host import VariableReport, check_ensemble, datasets, scratch, variable_names
from .ensemble_host import on_device as _on_device

REFERENCE_LEVELS = (0.0, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 1.0)  # data/xarray_preproc.py::compute_quantiles
SORT_CHUNK_ELEMS = 1 << 24  # values per float64 sort of the general route (128 MiB of float64 and as much of indices alive at a time)


def _levels(q) -> List[float]:
    if isinstance(q, torch.Tensor):
        q = q.detach().reshape(-1).tolist()
    elif isinstance(q, (int, float)):
        q = [q]
    q = [float(v) for v in q]
    if len(q) < 1:
        raise ValueError("at least one level")
    for v in q:
        if math.isnan(v) or v < 0.0 or v > 1.0:
            raise ValueError(f"level {v!r} is not in [0, 1]")
    return q


def _general(x: torch.Tensor, y: Optional[torch.Tensor], q: Sequence[float], skipna: bool, out: torch.Tensor, stats: torch.Tensor,
             n_valid: torch.Tensor) -> None:
    """The definition for any shape, any number of levels and any device: x (n_rep, T, F, hw), y (T, F, hw) or None; a float64
    ``torch.sort`` per data set, several data sets a sort while they fit SORT_CHUNK_ELEMS, and the same interpolation."""
    n_rep, T, F, hw = x.shape
    n, D = T * hw, int(out.shape[0])
    levels = torch.tensor(q, dtype=torch.float64, device=x.device)
    step = max(1, SORT_CHUNK_ELEMS // max(1, n))
    for first in range(0, D, step):
        rows = []
        for ds in range(first, min(D, first + step)):
            rows.append((x[ds // F, :, ds % F] if ds < n_rep * F else y[:, ds - n_rep * F]).reshape(-1))
        v = torch.stack(rows).double()                      # (d, n)
        nan = torch.isnan(v)
        nv = n - nan.sum(dim=1)                             # (d,) int64
        # NaNs become +inf before the sort (where a sort puts a NaN depends on its sign bit and on the device): ranks below nv never
        # reach them, and a true +inf among the first nv is the same number
        s = torch.sort(torch.where(nan, torch.full_like(v, float("inf")), v), dim=1).values
        pos = (nv - 1).double()[:, None] * levels[None, :]  # (d, Q)
        lo = torch.floor(pos)
        t = pos - lo
        last = (nv - 1).clamp(min=0)[:, None]
        lo = lo.long().clamp(min=0)
        lo = torch.minimum(lo, last)
        hi = torch.minimum(lo + 1, last)
        a, b = torch.gather(s, 1, lo), torch.gather(s, 1, hi)
        diff = b - a
        res = torch.where(t >= 0.5, b - diff * (1.0 - t), a + diff * t)
        dead = nv == 0
        if not skipna:
            dead = dead | nan.any(dim=1)
        nan_row = torch.full_like(res, float("nan"))
        sl = slice(first, first + len(rows))
        out[sl] = torch.where(dead[:, None], nan_row, res)
        stats[sl] = torch.where(dead[:, None, None], nan_row[..., None].float(), torch.stack([a, b], dim=-1).float())
        n_valid[sl] = nv


def _launch(x, y, q, skipna, out, stats, n_valid, n_rep, T, F, hw) -> bool:
    if not ops.quantile_supported(hw, len(q)):
        return False
    ws = scratch(ops.quantile_scratch_bytes(int(out.shape[0]), len(q)), x.device, torch.int64, optional=False)
    return ops.quantiles(x, y, q, skipna, ws, out, stats, n_valid, n_rep, T, F, hw)


def quantile(values: torch.Tensor, q, *, truth: Optional[torch.Tensor] = None, skipna: bool = True, return_stats: bool = False):
    """The quantiles at the levels ``q`` (numbers in ``[0, 1]``, Q of them) of every data set of ``values (..., T, F, H, W)`` -- one per
    leading index and variable, over all times and cells: float64 of shape ``values.shape[:-4] + (F, Q)`` on the same device (module
    docstring: the definition).  With ``truth (T, F, H, W)`` its F data sets ride in the same launch and the result is the pair
    ``(quantiles of values, quantiles of truth (F, Q))``.  ``return_stats=True`` makes each result a triple ``(quantiles, stats
    (..., F, Q, 2) fp32, n_valid (..., F) int64)``: the two order statistics every quantile is interpolated from and the number of
    non-NaN values.  Any float dtype and any strides: a strided or 16-bit input costs one dense fp32 copy.

    On the GPU, ``H W`` a multiple of 4 and ``Q <= 16`` take the kernels; everything else and CPU tensors take the same definition
    through a float64 sort, and give the same numbers.  A level outside ``[0, 1]`` raises ``ValueError`` before anything is launched."""
    q = _levels(q)
    x, y, lead = datasets(values, truth)
    n_rep, T, F, hw = (int(s) for s in x.shape)
    Q = len(q)
    if T * hw < 1 or F < 1:
        raise ValueError("an empty data set has no quantile")
    D = n_rep * F + (F if y is not None else 0)
    out = torch.empty((D, Q), dtype=torch.float64, device=x.device)
    stats = torch.empty((D, Q, 2), dtype=torch.float32, device=x.device)
    n_valid = torch.empty((D,), dtype=torch.int64, device=x.device)
    if D > 0 and not (_on_device(x) and _launch(x, y, q, skipna, out, stats, n_valid, n_rep, T, F, hw)):
        _general(x, y, q, skipna, out, stats, n_valid)
    k = n_rep * F
    first = (out[:k].view(lead + (F, Q)), stats[:k].view(lead + (F, Q, 2)), n_valid[:k].view(lead + (F,)))
    second = (out[k:], stats[k:], n_valid[k:])
    if not return_stats:
        first, second = first[0], second[0]
    return first if truth is None else (first, second)


class QuantileReport(VariableReport):
    """Per variable the tails of an ensemble against the truth, as device tensors: ``truth (Q,)`` the truth's quantiles, ``samples
    (M, Q)`` every member's and ``diff (M, Q)`` = ``samples - truth``, all float64; ``levels`` the Q levels."""

    def __init__(self, names: Sequence[str], levels: Sequence[float], variables: List[dict]):
        super().__init__(names, variables)
        self.levels = tuple(levels)

    def as_dict(self, prefix: str = "quantiles") -> dict:
        """flat ``{name: float}`` for a logger (one device-to-host copy): per variable and level ``q<level>/truth``, ``/mean`` (the
        members' mean), ``/bias`` (the mean of ``diff``) and ``/max_abs_diff`` (the worst member)."""
        table = torch.stack([torch.cat([v["truth"][None], v["samples"]]) for v in self.variables]).cpu().numpy()  # (F, 1 + M, Q)
        out = {}
        for i, name in enumerate(self.names):
            truth, members = table[i, 0], table[i, 1:]  # the statistics are formed on the host: the same on every device
            diff = members - truth[None]
            for j, level in enumerate(self.levels):
                key = f"{prefix}/{name}/q{level:g}"
                out[f"{key}/truth"] = float(truth[j])
                out[f"{key}/mean"] = float(members[:, j].mean())
                out[f"{key}/bias"] = float(diff[:, j].mean())
                out[f"{key}/max_abs_diff"] = float(abs(diff[:, j]).max())
        return out


def quantile_report(samples: torch.Tensor, truth: torch.Tensor, q=REFERENCE_LEVELS, names: Optional[Sequence[str]] = None) -> QuantileReport:
    """The quantiles of every member of an ensemble ``samples (M, L, F, H, W)`` and of the ``truth (L, F, H, W)`` per variable -- by
    default at the reference's nine levels, 1 % and 99 % among them -- from one launch sequence.  The fields are expected
    DE-NORMALISED.  ``names``: one per variable, default ``var0 ...``."""
    check_ensemble(samples, truth, time="L", members="M >= 1")
    F = int(truth.shape[1])
    names = variable_names(names, F)
    levels = _levels(q)
    qs, qt = quantile(samples, levels, truth=truth)  # (M, F, Q), (F, Q)
    variables = [dict(truth=qt[f], samples=qs[:, f], diff=qs[:, f] - qt[f][None]) for f in range(F)]
    return QuantileReport(names, levels, variables)
