"""Empirical quantile mapping per cell on the device: the bias correction that turns a coarse climate-model series into the ``y`` of
``condition_on(A=..., y=...)``.

The reference's headline application is downscaling climate-model output: its ``exp/configs/001_clim-downscaling/*.yml`` runs condition
the sampler on ``debiased_hadgem.nc`` / ``debiased_mpi.nc``, and its ``downscaled_clim_dist`` figure compares "raw vs qm".  The quantile
mapping that makes those files happens outside the reference.  Here it is two kernels (csrc/qmap.hip): per-cell quantiles over time --
useful on their own, for per-cell 99th-percentile maps of members against the truth -- and a per-cell transfer function applied to
every value.

**The definition**, in this project's words (include/c2w_hip.h: c2w_qmap_nodes, c2w_qmap_apply).  A *series* is the values of one
variable at one cell over the times of one group; a group is, for example, a calendar month, and ``G = 1`` means no grouping.  Levels
are ``p_0 < ... < p_{K-1}`` in ``[0, 1]``, ``K >= 2``, by default the 101 levels ``k / 100``: including 0 and 1 makes the table span
the sample's range.

*Nodes.*  ``q[g, f, c, k]`` is ``numpy.nanquantile(series.astype(float64), p_k)``: the definition of ``quantiles.py`` (README,
statement 7) applied to a series -- the two order statistics exact fp32, the interpolation float64.  ``skipna=True`` leaves NaNs out;
``False`` makes the series' row NaN.  A series with no valid value, an empty group included, is a NaN row.  ``n_valid[g, f, c]`` is
int64.

*Mapping.*  ``xq`` is the nodes of the model's historical series, ``yq`` the nodes of the reference's, both float64.  An fp32 value
``x`` of that series' cell and group maps as follows, all in float64:

* ``j`` is the last node with ``xq[j] <= x``
* ``x < xq[0]``: ``y = x + (yq[0] - xq[0])``
* ``j = K - 1``: ``y = x + (yq[K-1] - xq[K-1])`` -- the additive constant extrapolation; it covers ``x == xq[K-1]`` and ``+inf``
* otherwise ``y = min(yq[j] + (x - xq[j]) * ((yq[j+1] - yq[j]) / (xq[j+1] - xq[j])), yq[j+1])``; no multiply is fused with an add, the
  interval is never degenerate because ``j`` is the last such node, and the ``min`` (``v > top ? top : v``) makes the map exactly
  non-decreasing across node boundaries
* ``y`` is then rounded once to fp32; a NaN ``x`` or a NaN table row gives NaN, and nothing else does.

``QuantileMapping.fit`` turns a table row with a NaN node in either table -- a series without a valid value, or one that held an
infinity (numpy's interpolation between two equal infinities is NaN) -- into a NaN row of both tables, so "a NaN table row" is the only
kind of NaN a fitted table holds.

This is empirical quantile mapping as commonly described; the definition is recalled, ``numpy.nanquantile`` and ``numpy.interp`` are
the verified parts, and the stated choices -- per cell, per group, levels including 0 and 1, additive constant tails, the clamp -- are
this project's own (README, statement 12).

On the GPU the kernels take ``H W`` a multiple of 4, ``2 <= K <= 128`` and groups of at most 16 384 times; everything else and CPU
tensors take the same definition in float64 torch (``torch.sort`` along time, chunked, ``searchsorted``, the same formula) and give the
same numbers.  The group ids are read on the host, once, to be checked and turned into the kernels' time lists; nothing else
synchronises.

Out of scope: trend-preserving variants (quantile delta mapping, detrended quantile mapping), multiplicative mapping, moving-window
groups, parametric fits, netCDF I/O, the on-device series sort beyond 16 384 values, and collectives.
"""
from __future__ import annotations

import datetime
import math
from typing import List, Optional, Sequence

import torch

from . import qmap_ops
from .ensemble_host import VariableReport, chunk_step, datasets, dense32, scratch, variable_names
from .ensemble_host import on_device as _on_device
from .quantiles import REFERENCE_LEVELS, quantile

NAN = float("nan")
DEFAULT_LEVELS = 101
GATHER_TILE = 64  # cells of a tile of the gather kernel: the cell blocks of the node fit are multiples of it


def _levels(levels) -> List[float]:
    """an int K -> the K levels k / (K - 1); else the levels themselves, checked"""
    if isinstance(levels, int):
        if levels < 2:
            raise ValueError(f"{levels} levels: at least 2")
        return [k / (levels - 1) for k in range(levels - 1)] + [1.0]
    if isinstance(levels, torch.Tensor):
        levels = levels.detach().reshape(-1).tolist()
    p = [float(v) for v in levels]
    if len(p) < 2:
        raise ValueError(f"{len(p)} levels: at least 2")
    for v in p:
        if math.isnan(v) or v < 0.0 or v > 1.0:
            raise ValueError(f"level {v!r} is not in [0, 1]")
    if any(b <= a for a, b in zip(p, p[1:])):
        raise ValueError("the levels must increase strictly")
    return p


class _GroupLists:
    """The groups of T times as the kernels and the general route read them: ``ids`` (host list), ``index[g]`` the times of group g in
    ascending order (host lists), ``tidx`` (T,) int32 the same lists one after the other and ``goff`` (G + 1,) int32 where each begins
    (on ``device``), ``max_len`` the longest."""

    def __init__(self, groups, n_groups: Optional[int], T: int, device):
        if groups is None:
            G = 1 if n_groups is None else int(n_groups)
            ids = [0] * T
        else:
            if not isinstance(groups, torch.Tensor) or groups.is_floating_point() or groups.dtype == torch.bool or groups.dim() != 1 \
                    or int(groups.shape[0]) != T:
                raise ValueError(f"groups must be an integer tensor of shape ({T},)")
            ids = [int(v) for v in groups.tolist()]
            G = (max(ids) + 1 if ids else 1) if n_groups is None else int(n_groups)
        if G < 1:
            raise ValueError(f"n_groups {G} must be at least 1")
        for t, g in enumerate(ids):
            if g < 0 or g >= G:
                raise ValueError(f"group id {g} of time {t} is not in [0, {G})")
        self.G, self.ids, self.T, self.device = G, ids, T, device
        self.index = [[t for t, v in enumerate(ids) if v == g] for g in range(G)]
        self.max_len = max(len(i) for i in self.index)
        offsets = [0]
        for i in self.index:
            offsets.append(offsets[-1] + len(i))
        self.tidx = torch.tensor([t for i in self.index for t in i], dtype=torch.int32, device=device)
        self.goff = torch.tensor(offsets, dtype=torch.int32, device=device)


# ---------------------------------------------------------------------------------------------------------------------- nodes

def _general_nodes(x: torch.Tensor, gl: _GroupLists, levels: torch.Tensor, skipna: bool, q: torch.Tensor, n_valid: torch.Tensor) -> None:
    """The definition for any shape, any number of levels and any device: x (n_rep, T, F, hw), q (n_rep, G, F, hw, K); a float64
    ``torch.sort`` along the times of a group, a block of cells at a time, and the interpolation of ``quantiles._general``."""
    n_rep, _, F, hw = (int(s) for s in x.shape)
    for g in range(gl.G):
        n = len(gl.index[g])
        if n == 0:
            q[:, g] = NAN
            n_valid[:, g] = 0
            continue
        idx = torch.tensor(gl.index[g], dtype=torch.int64, device=x.device)
        step = chunk_step(n_rep * n * F)
        for c0 in range(0, hw, step):
            v = x[:, idx, :, c0:c0 + step].double()                       # (n_rep, n, F, c)
            nan = torch.isnan(v)
            nv = n - nan.sum(dim=1)                                       # (n_rep, F, c) int64
            # NaNs become +inf before the sort: ranks below nv never reach them (quantiles._general)
            s = torch.sort(torch.where(nan, torch.full_like(v, float("inf")), v), dim=1).values.permute(0, 2, 3, 1)
            pos = (nv - 1).double()[..., None] * levels                   # (n_rep, F, c, K)
            lo = torch.floor(pos)
            t = pos - lo
            last = (nv - 1).clamp(min=0)[..., None]
            lo = torch.minimum(lo.long().clamp(min=0), last)
            hi = torch.minimum(lo + 1, last)
            a, b = torch.gather(s, -1, lo), torch.gather(s, -1, hi)
            diff = b - a
            res = torch.where(t >= 0.5, b - diff * (1.0 - t), a + diff * t)
            dead = nv == 0
            if not skipna:
                dead = dead | nan.any(dim=1)
            q[:, g, :, c0:c0 + step] = torch.where(dead[..., None], torch.full_like(res, NAN), res)
            n_valid[:, g, :, c0:c0 + step] = nv


def _launch_nodes(x, gl: _GroupLists, levels, skipna, q, n_valid) -> bool:
    n_rep, T, F, hw = (int(s) for s in x.shape)
    K = int(levels.shape[0])
    if not qmap_ops.qmap_supported(hw, K, gl.max_len):
        return False
    block = min(hw, max(GATHER_TILE, chunk_step(n_rep * F * T) // GATHER_TILE * GATHER_TILE))  # cells a launch pair: the scratch stays bounded
    ws = scratch(qmap_ops.qmap_scratch_bytes(n_rep * F, block, T), x.device, torch.float32, optional=False)
    for c0 in range(0, hw, block):
        if not qmap_ops.qmap_nodes(x, gl.tidx, gl.goff, levels, q, n_valid, ws, n_rep, T, F, hw, T, gl.G, K, gl.max_len, skipna, c0,
                                   min(hw, c0 + block)):
            return False
    return True


def _cell_quantiles(values, levels: List[float], gl_of, skipna: bool):
    if not values.is_floating_point():
        raise ValueError(f"values ({values.dtype}) must be floating point")
    x, _, lead = datasets(values, None)
    n_rep, T, F, hw = (int(s) for s in x.shape)
    if n_rep * F * hw < 1:
        raise ValueError(f"values {tuple(values.shape)} hold no series")
    gl = gl_of(T, x.device)
    K = len(levels)
    lv = torch.tensor(levels, dtype=torch.float64, device=x.device)
    q = torch.empty((n_rep, gl.G, F, hw, K), dtype=torch.float64, device=x.device)
    n_valid = torch.empty((n_rep, gl.G, F, hw), dtype=torch.int64, device=x.device)
    if T == 0:
        q.fill_(NAN), n_valid.zero_()
    elif not (_on_device(x) and _launch_nodes(x, gl, lv, skipna, q, n_valid)):
        _general_nodes(x, gl, lv, skipna, q, n_valid)
    H, W = (int(s) for s in values.shape[-2:])
    return q.view(lead + (gl.G, F, H, W, K)), n_valid.view(lead + (gl.G, F, H, W))


def cell_quantiles(values: torch.Tensor, levels=DEFAULT_LEVELS, *, groups: Optional[torch.Tensor] = None, n_groups: Optional[int] = None,
                   skipna: bool = True, return_counts: bool = False):
    """The quantiles over time of every cell of ``values (..., T, F, H, W)``: float64 ``(..., G, F, H, W, K)`` on the same device, per
    leading index, group, variable and cell the quantiles at the K ``levels`` (an int K: the levels ``k / (K - 1)``; or K >= 2 numbers
    in ``[0, 1]``, strictly increasing) of the series over the times of the group (module docstring: the definition).  ``groups``: an
    integer ``(T,)`` tensor of ids in ``[0, G)``, ``G = n_groups`` or the largest id plus one; None: one group.  ``return_counts=True``
    also returns ``n_valid (..., G, F, H, W)`` int64.  Leading dimensions -- members, say -- ride in one launch sequence.  Any float dtype and
    any strides: a strided or 16-bit input costs one dense fp32 copy.  Bad levels or a bad id raise ``ValueError`` before any launch."""
    levels = _levels(levels)
    q, n_valid = _cell_quantiles(values, levels, lambda T, device: _GroupLists(groups, n_groups, T, device), skipna)
    return (q, n_valid) if return_counts else q


# ---------------------------------------------------------------------------------------------------------------------- mapping

def _general_apply(x: torch.Tensor, out: torch.Tensor, xq: torch.Tensor, yq: torch.Tensor, gl: _GroupLists) -> None:
    """The mapping for any shape and device, float64: x, out (n_rep, T, F, hw), xq, yq (G, F, hw, K)."""
    n_rep, T, F, hw = (int(s) for s in x.shape)
    K = int(xq.shape[-1])
    gid = torch.tensor(gl.ids, dtype=torch.int64, device=x.device)
    step = chunk_step(F * hw * K)
    for t0 in range(0, T, step):
        tx, ty = xq[gid[t0:t0 + step]].contiguous(), yq[gid[t0:t0 + step]]                      # (t, F, hw, K)
        bottom, top = ty[..., 0] - tx[..., 0], ty[..., -1] - tx[..., -1]
        for r in range(n_rep):
            v = x[r, t0:t0 + step].double()                                                     # (t, F, hw)
            lo = torch.searchsorted(tx, v[..., None].contiguous(), right=True)                  # nodes with xq <= x: (t, F, hw, 1)
            j = (lo - 1).clamp(0, K - 2)
            xj, xj1 = torch.gather(tx, -1, j)[..., 0], torch.gather(tx, -1, j + 1)[..., 0]
            yj, yj1 = torch.gather(ty, -1, j)[..., 0], torch.gather(ty, -1, j + 1)[..., 0]
            slope = (yj1 - yj) / (xj1 - xj)
            inside = yj + (v - xj) * slope
            inside = torch.where(inside > yj1, yj1, inside)
            lo = lo[..., 0]
            y = torch.where(lo == 0, v + bottom, torch.where(lo == K, v + top, inside))
            # a NaN has no place in a sorted table: whatever the search said, a NaN x or a NaN row is NaN
            y = torch.where(torch.isnan(v) | torch.isnan(tx[..., 0]), torch.full_like(y, NAN), y)
            out[r, t0:t0 + step] = y.float()


class QuantileMapping:
    """A fitted mapping: ``levels`` (K,) float64, ``xq`` and ``yq`` ``(G, F, H, W, K)`` float64 -- the nodes of the model's and of the
    reference's historical series -- and ``n_valid_model``, ``n_valid_reference`` ``(G, F, H, W)`` int64."""

    KEYS = ("levels", "xq", "yq", "n_valid_model", "n_valid_reference")

    def __init__(self, levels: torch.Tensor, xq: torch.Tensor, yq: torch.Tensor, n_valid_model: torch.Tensor, n_valid_reference: torch.Tensor):
        if xq.dim() != 5 or xq.shape != yq.shape or xq.dtype != torch.float64 or yq.dtype != torch.float64:
            raise ValueError(f"xq {tuple(xq.shape)} and yq {tuple(yq.shape)} must be float64 (G, F, H, W, K)")
        if int(xq.shape[-1]) != int(levels.numel()) or int(levels.numel()) < 2:
            raise ValueError(f"{int(levels.numel())} levels for tables of {int(xq.shape[-1])} nodes")
        self.levels = levels.to(device=xq.device, dtype=torch.float64).reshape(-1)
        self.xq, self.yq = xq.contiguous(), yq.contiguous()
        self.n_valid_model, self.n_valid_reference = n_valid_model, n_valid_reference

    @property
    def n_groups(self) -> int:
        return int(self.xq.shape[0])

    @classmethod
    def fit(cls, model: torch.Tensor, reference: torch.Tensor, *, levels=DEFAULT_LEVELS, model_groups: Optional[torch.Tensor] = None,
            reference_groups: Optional[torch.Tensor] = None, n_groups: Optional[int] = None, skipna: bool = True) -> "QuantileMapping":
        """``model (T, F, H, W)`` and ``reference (T', F, H, W)``: the model's historical fields and the reference's (observations or a
        reanalysis, coarsened to the model's grid by the caller) over the calibration period; the two archives may differ in length.
        ``model_groups (T,)`` / ``reference_groups (T',)``: integer ids in ``[0, G)``, ``G = n_groups`` or the largest id of both plus
        one; None: one group.  Bad levels or a bad id raise ``ValueError`` before any launch."""
        levels = _levels(levels)
        if model.dim() != 4 or reference.dim() != 4 or tuple(model.shape[1:]) != tuple(reference.shape[1:]):
            raise ValueError(f"model {tuple(model.shape)} and reference {tuple(reference.shape)} must be (T, F, H, W) and (T', F, H, W)")
        if model.device != reference.device:
            raise ValueError(f"model ({model.device}) and reference ({reference.device}) must be on one device")
        if n_groups is None:
            n_groups = 1
            for g in (model_groups, reference_groups):
                if isinstance(g, torch.Tensor) and g.numel() > 0 and not g.is_floating_point():
                    n_groups = max(n_groups, int(g.max()) + 1)
        # both lists are checked before the first launch
        lists = [_GroupLists(g, n_groups, int(v.shape[0]), v.device) for g, v in ((model_groups, model), (reference_groups, reference))]
        xq, nx = _cell_quantiles(model, levels, lambda T, device: lists[0], skipna)
        yq, ny = _cell_quantiles(reference, levels, lambda T, device: lists[1], skipna)
        bad = (torch.isnan(xq).any(dim=-1) | torch.isnan(yq).any(dim=-1))[..., None]
        nan = torch.full_like(xq, NAN)
        return cls(torch.tensor(levels, dtype=torch.float64, device=xq.device), torch.where(bad, nan, xq), torch.where(bad, nan, yq), nx, ny)

    def apply(self, x: torch.Tensor, groups: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``x (..., T, F, H, W)`` mapped value by value through the tables of its cell and of its time's group: fp32 of the same shape.
        ``groups (T,)``: the ids of x's times (None only where the mapping has one group).  ``out``: a dense fp32 tensor of x's shape
        to write to; it may be ``x`` itself."""
        if not x.is_floating_point() or x.dim() < 4 or tuple(x.shape[-3:]) != tuple(self.xq.shape[1:4]):
            raise ValueError(f"x {tuple(x.shape)} ({x.dtype}) must be floating point (..., T, F, H, W) with (F, H, W) = {tuple(self.xq.shape[1:4])}")
        if x.device != self.xq.device:
            raise ValueError(f"x ({x.device}) and the tables ({self.xq.device}) must be on one device")
        if groups is None and self.n_groups != 1:
            raise ValueError(f"the mapping has {self.n_groups} groups: apply needs the group of every time")
        T, F, H, W = (int(s) for s in x.shape[-4:])
        gl = _GroupLists(groups, self.n_groups, T, x.device)
        if out is None:
            out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        elif out.dtype != torch.float32 or out.shape != x.shape or out.device != x.device or not out.is_contiguous() or out.data_ptr() % 16:
            raise ValueError("out must be a dense, 16-byte aligned fp32 tensor of x's shape on x's device")
        if x.numel() == 0:
            return out
        xs = dense32(x).view(-1, T, F, H * W)
        res, K = out.view(-1, T, F, H * W), int(self.xq.shape[-1])
        xq, yq = self.xq.view(self.n_groups, F, H * W, K), self.yq.view(self.n_groups, F, H * W, K)
        n_rep = int(xs.shape[0])
        if not (_on_device(xs) and qmap_ops.qmap_supported(H * W, K, gl.max_len) and
                qmap_ops.qmap_apply(xs, res, xq, yq, gl.tidx, gl.goff, n_rep, T, F, H * W, T, gl.G, K, gl.max_len)):
            _general_apply(xs, res, xq, yq, gl)
        return out

    def state_dict(self) -> dict:
        return {k: getattr(self, k) for k in self.KEYS}

    @classmethod
    def from_state_dict(cls, state: dict) -> "QuantileMapping":
        return cls(*(state[k] for k in cls.KEYS))

    def to(self, device) -> "QuantileMapping":
        return QuantileMapping(*(getattr(self, k).to(device) for k in self.KEYS))


# ---------------------------------------------------------------------------------------------------------------------- calendar, report

def calendar_groups(start: str, num: int, step_hours: int = 1, by: Optional[str] = "month") -> torch.Tensor:
    """The group id of each of ``num`` times ``step_hours`` apart from ``start`` (the reference's ``YYYY-MM-DD-HH``), as an int64
    ``(num,)`` host tensor: ``by="month"`` 0 .. 11 (January 0), ``"season"`` 0 .. 3 (DJF, MAM, JJA, SON), None all 0.  The calendar is
    ``datetime``'s proleptic Gregorian one; a model on a 360-day or no-leap calendar needs ids of the caller's own."""
    if by not in ("month", "season", None):
        raise ValueError(f"by {by!r} must be 'month', 'season' or None")
    if int(num) < 0 or int(step_hours) < 1:
        raise ValueError(f"num {num} must be >= 0 and step_hours {step_hours} >= 1")
    t0 = datetime.datetime.strptime(start, "%Y-%m-%d-%H")
    ids = []
    for i in range(int(num)):
        month = (t0 + datetime.timedelta(hours=i * int(step_hours))).month
        ids.append(0 if by is None else month - 1 if by == "month" else (month % 12) // 3)
    return torch.tensor(ids, dtype=torch.int64)


def bias_report(model: torch.Tensor, reference: torch.Tensor, mapping: QuantileMapping, *, groups: Optional[torch.Tensor] = None,
                names: Optional[Sequence[str]] = None, levels=REFERENCE_LEVELS) -> VariableReport:
    """Per variable the pooled quantile bias of ``model (T, F, H, W)`` against ``reference (T', F, H, W)`` before and after the
    correction, through ``quantiles.quantile`` -- all times and cells of a variable -- at ``levels`` (the reference's nine by default):
    ``reference``, ``before``, ``after`` (Q,) and ``bias_before = before - reference``, ``bias_after = after - reference``, float64
    device tensors; ``report.levels`` the levels.  ``groups``: the ids of the model's times."""
    if model.dim() != 4 or reference.dim() != 4 or tuple(model.shape[1:]) != tuple(reference.shape[1:]):
        raise ValueError(f"model {tuple(model.shape)} and reference {tuple(reference.shape)} must be (T, F, H, W) and (T', F, H, W)")
    names = variable_names(names, int(model.shape[1]))
    levels = [float(v) for v in levels]
    corrected = mapping.apply(model, groups)
    ref, before, after = quantile(reference, levels), quantile(model, levels), quantile(corrected, levels)  # (F, Q) each
    report = VariableReport(names, [dict(reference=ref[f], before=before[f], after=after[f], bias_before=before[f] - ref[f],
                                         bias_after=after[f] - ref[f]) for f in range(len(names))])
    report.levels = tuple(levels)
    return report
