"""Dependence of an ensemble on the device: *do the variables still belong together, and does each member move with the truth?*  Every
other score of the evaluation side judges a variable on its own (``windpower`` pairs ``u`` and ``v`` for one purpose, ``multivariate``
folds all variables into one number).  This module streams, per cell, the co-moments of the ``F`` variables of every member and of the
truth, and of every member WITH the truth: the inter-variable correlation a jointly trained downscaler is bought for, and the
elementary climatology maps -- mean bias, standard-deviation ratio, temporal correlation with the truth, centred RMSE (the
Taylor-diagram triple).  These run along time, and a year of hourly fields does not arrive at once: ``DependenceAccumulator.update``
takes them in calls of any length, next to ``spells.SpellAccumulator`` and ``extremes.ExtremeAccumulator``.  Its carried state is
floating point.

**Rows.**  ``d = 0`` is the truth if one is given, then the ``M`` members: ``D = M + 1``, or ``M`` without a truth.  A series is one
``(d, f, cell)`` over time; ``F`` is the number of variables.

**Valid hour.**  Hour ``t`` is valid for ``(d, cell)`` iff all ``F`` values of row ``d`` at that cell are finite and, with a truth, all
``F`` truth values at that cell are finite too.  Finite is decided on the fp32 bits -- a float64 or 16-bit input is rounded / widened
to fp32 once --: exponent field not all ones.  An invalid hour adds nothing to any entry of that ``(d, cell)`` and is counted in
``invalid (D,)`` int64, in cell-hours.  Infinities are invalid, not values.

**Pivots.**  At the first valid hour of ``(d, cell)`` ``P[d, f, cell]`` becomes the row's own fp32 value and, with a truth,
``PT[d, f, cell]`` the truth's fp32 value at that same hour.  Both are fp32 and never change afterwards.  ``n[d, cell]`` (int32) counts
the valid hours; ``n == 0`` means "no pivot yet".

**Sums** (include/c2w_hip.h: c2w_comoments_update).  ``e_f = (double)x_f - (double)P_f`` and ``eT_f = (double)y_f - (double)PT_f``.
Per valid hour, in hour order, with no multiply fused with an add, each accumulator is a plain ``s = s + term``:

    S[f] += e_f                      F entries
    C[f, g] += e_f e_g   (f <= g)    F (F + 1) / 2 entries, in the order (0,0), (0,1) .. (0,F-1), (1,1) ..
    ST[f] += eT_f                    F entries  }
    QT[f] += eT_f eT_f               F entries  }  with a truth only
    X[f] += e_f eT_f                 F entries  }

``NS = 4 F + F (F + 1) / 2`` entries with a truth, ``F + F (F + 1) / 2`` without.  Row 0 carries the same layout; there ``eT = e``, so
``X = QT = C_ff``.  ``sums (D, NS, hw)`` float64, ``pivot`` and ``truth_pivot (D, F, hw)`` fp32, ``n (D, hw)`` int32.  The first valid
hour contributes ``e = 0`` exactly; an all-invalid series keeps ``n = 0``, zero sums and a pivot of ``+0.0``.

**Bit for bit on every route.**  Every accumulator receives its terms one at a time in hour order and the state carries the doubles
themselves, so the tables are the same bits on the kernel (csrc/comoments.hip: one thread owns a cell's series), on the torch route,
in the NumPy reference of the tests and for every cut of the hours into updates.  The general route (``_general``) therefore also adds
hour by hour: a loop over ``t`` of element-wise float64 torch ops, ``mul`` then ``add``, chunked over the cells.  **That route is slow,
and it is the definition.**

**Why the pivot.**  It removes the field's magnitude before any product.  At 101325 +- 0.5 Pa over 400 hours the unpivoted one-pass
float64 form ``sum xy - sum x sum y / n`` misses the bound below by about 1e8; csrc/comoments_maps.h derives the bound
``(n + 1) 2^-53 sum |e_f|`` for ``S`` and ``ST`` and ``(n + 2) 2^-53 sum |e_f e_g|`` for the product sums (plus one denormal each)
against exact rational arithmetic, and the tests hold every route to it.

**merge** adds another accumulator over OTHER hours of the same cells (another rank's time shard): the other's sums are re-based
onto this one's pivots in float64, ``S' = S_o + n d_f``, ``C'_fg = C_o,fg + d_f S_o,g + d_g S_o,f + n d_f d_g`` with
``d = P_other - P_self``, likewise ``ST``, ``QT`` and ``X``.  A series with ``n_self = 0`` takes the other's state as it is.  The result
is no longer bit-identical to one pass; it lies within the merge bound the header derives.

On the GPU ``H W`` a multiple of 4 and ``F <= 8`` take the kernel (no instantiation uses scratch memory, so the device limit is the
issue's 8).  Everything else and CPU tensors take ``_general``.  The statistics below are float64 tensor algebra on the tables; they
stay on the device and never synchronise.

Out of scope: rank (Spearman) correlation, lagged cross-correlation, spatial correlation between cells and EOFs, per-time pattern
correlation (ACC), higher co-moments, a time split over workgroups for grids with few cells.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import dependence_ops
from .ensemble_host import VariableReport, check_ensemble, chunk_step, datasets, member_mean_std, variable_names
from .ensemble_host import on_device as _on_device

MAX_CALL = 1 << 20  # hours one launch takes (csrc/comoments_maps.h: MAX_T); a longer update is walked in parts
MAX_F = 8           # variables the kernel takes (csrc/comoments_maps.h: MAX_F)
_EXP = 0x7F800000


class CoMomentTables(NamedTuple):
    """What ``DependenceAccumulator.tables`` returns (module docstring)"""
    n: torch.Tensor                      # (D, H, W) int32
    pivot: torch.Tensor                  # (D, F, H, W) fp32
    truth_pivot: Optional[torch.Tensor]  # (D, F, H, W) fp32, None without a truth
    sums: torch.Tensor                   # (D, NS, H, W) float64
    invalid: torch.Tensor                # (D,) int64
    with_truth: bool


# ---------------------------------------------------------------------------------------------------------------------- the layout

def pair_list(F: int) -> List[Tuple[int, int]]:
    """the pairs ``(f, g)``, ``f <= g``, in the order of the ``C`` block"""
    return [(f, g) for f in range(F) for g in range(f, F)]


def entries(F: int, with_truth: bool) -> int:
    return F + F * (F + 1) // 2 + (3 * F if with_truth else 0)


def _blocks(F: int):
    """where the blocks S, C, ST, QT, X of a series' entries begin and end"""
    NP = F * (F + 1) // 2
    return dict(S=(0, F), C=(F, F + NP), ST=(F + NP, 2 * F + NP), QT=(2 * F + NP, 3 * F + NP), X=(3 * F + NP, 4 * F + NP))


def _variables_of(t: CoMomentTables) -> int:
    return int(t.pivot.shape[1])


def _block(t: CoMomentTables, name: str) -> torch.Tensor:
    a, b = _blocks(_variables_of(t))[name]
    return t.sums[:, a:b]


def _pair_matrix(F: int, device) -> torch.Tensor:
    """``(F, F)`` int64: the entry of the ``C`` block that holds the pair ``(min(f, g), max(f, g))``"""
    at = {p: k for k, p in enumerate(pair_list(F))}
    return torch.tensor([[at[(min(f, g), max(f, g))] for g in range(F)] for f in range(F)], dtype=torch.int64, device=device)


def _finite(rows: torch.Tensor) -> torch.Tensor:
    """fp32 -> bool: the exponent field is not all ones"""
    return (rows.view(torch.int32) & _EXP) != _EXP


# ---------------------------------------------------------------------------------------------------------------------- one call

def _general(x, y, n, pivot, truth_pivot, sums, invalid) -> None:
    """The definition for any shape and any device, hour by hour: x (M, T, F, hw), y (T, F, hw) or None; the state as
    ``dependence_ops.comoments_update`` takes it.  Slow, and the definition (module docstring)."""
    M, T, F, hw = (int(s) for s in x.shape)
    D, NS = int(sums.shape[0]), int(sums.shape[1])
    if T == 0:
        return
    with_truth = y is not None
    pf = torch.tensor([p[0] for p in pair_list(F)], dtype=torch.int64, device=x.device)
    pg = torch.tensor([p[1] for p in pair_list(F)], dtype=torch.int64, device=x.device)
    blk = _blocks(F)
    step = chunk_step(2 * D * NS)
    for c0 in range(0, hw, step):
        c1 = min(hw, c0 + step)
        nc, P, s = n[:, c0:c1].clone(), pivot[:, :, c0:c1].clone(), sums[:, :, c0:c1].clone()
        PT = truth_pivot[:, :, c0:c1].clone() if with_truth else None
        for t in range(T):
            rows = x[:, t, :, c0:c1] if not with_truth else torch.cat([y[None, t, :, c0:c1], x[:, t, :, c0:c1]])     # (D, F, c)
            valid = _finite(rows.contiguous()).all(dim=1)                                                              # (D, c)
            if with_truth:
                yt = y[t, :, c0:c1].contiguous()
                valid = valid & _finite(yt).all(dim=0)[None]
            first = (valid & (nc == 0))[:, None]
            nc += valid.to(torch.int32)
            invalid += (~valid).sum(dim=1)
            v = valid[:, None]
            P = torch.where(first, rows, P)
            e = torch.where(v, rows.to(torch.float64) - P.to(torch.float64), 0.0)
            s[:, blk["S"][0]:blk["S"][1]] += e
            s[:, blk["C"][0]:blk["C"][1]] += torch.mul(e[:, pf], e[:, pg])
            if with_truth:
                PT = torch.where(first, yt[None], PT)
                eT = torch.where(v, yt[None].to(torch.float64) - PT.to(torch.float64), 0.0)
                s[:, blk["ST"][0]:blk["ST"][1]] += eT
                s[:, blk["QT"][0]:blk["QT"][1]] += torch.mul(eT, eT)
                s[:, blk["X"][0]:blk["X"][1]] += torch.mul(e, eT)
        n[:, c0:c1], pivot[:, :, c0:c1], sums[:, :, c0:c1] = nc, P, s
        if with_truth:
            truth_pivot[:, :, c0:c1] = PT


def _launch(x, y, n, pivot, truth_pivot, sums, invalid) -> bool:
    M, T, F, hw = (int(s) for s in x.shape)
    if not dependence_ops.supported(hw, F):
        return False
    return dependence_ops.comoments_update(x, y, n, pivot, truth_pivot, sums, invalid, M, T, F, hw)


# ---------------------------------------------------------------------------------------------------------------------- the accumulator

def _count(value, name: str, low: int) -> int:
    if isinstance(value, bool) or int(value) != value or int(value) < low:
        raise ValueError(f"{name} {value!r} must be an integer >= {low}")
    return int(value)


class DependenceAccumulator:
    """Co-moments of ``M`` members (and the truth) of ``F`` variables on ``H x W`` cells, carried from update to update:

        acc = DependenceAccumulator(M, F, H, W, device=samples.device)
        for samples, truth in calls:           # (M, T, F, H, W), (T, F, H, W); any T >= 0
            acc.update(samples, truth)
        tables = acc.tables()

    ``with_truth=False``: the rows are the members alone and ``update`` takes no truth.  The memory is that of the state,
    ``8 NS + 8 F + 4`` bytes a series' cell and row."""

    def __init__(self, M: int, F: int, H: int, W: int, *, with_truth: bool = True, device=None):
        self.M, self.F, self.H, self.W = _count(M, "M", 1), _count(F, "F", 1), _count(H, "H", 1), _count(W, "W", 1)
        self.with_truth = bool(with_truth)
        self.device = torch.device("cpu" if device is None else device)
        self.D = self.M + (1 if self.with_truth else 0)
        self.NS = entries(self.F, self.with_truth)
        D, hw = self.D, self.H * self.W
        self.n = torch.zeros((D, hw), dtype=torch.int32, device=self.device)
        self.pivot = torch.zeros((D, self.F, hw), dtype=torch.float32, device=self.device)
        self.truth_pivot = torch.zeros((D, self.F, hw), dtype=torch.float32, device=self.device) if self.with_truth else None
        self.sums = torch.zeros((D, self.NS, hw), dtype=torch.float64, device=self.device)
        self.invalid = torch.zeros((D,), dtype=torch.int64, device=self.device)
        self.n_times = 0

    def update(self, samples: torch.Tensor, truth: Optional[torch.Tensor] = None) -> "DependenceAccumulator":
        """``samples (M, T, F, H, W)`` and, with a truth, ``truth (T, F, H, W)``: the next ``T >= 0`` hours.  Any float dtype and any
        strides: a strided or non-fp32 input costs one dense fp32 copy of the call."""
        if self.with_truth != (truth is not None):
            raise ValueError("this accumulator was made with a truth: update(samples, truth)" if self.with_truth else
                             "this accumulator was made without a truth: update(samples)")
        if truth is not None:
            check_ensemble(samples, truth, members="M >= 1", floating=True)
        elif samples.dim() != 5 or not samples.is_floating_point():
            raise ValueError(f"samples {tuple(samples.shape)} ({samples.dtype}) must be floating point (M, T, F, H, W)")
        want = (self.M, self.F, self.H, self.W)
        if (int(samples.shape[0]),) + tuple(int(s) for s in samples.shape[2:]) != want:
            raise ValueError(f"samples {tuple(samples.shape)} must be (M, T, F, H, W) = ({self.M}, T, {self.F}, {self.H}, {self.W})")
        if samples.device != self.device or (truth is not None and truth.device != self.device):
            raise ValueError(f"the call must be on {self.device}, the accumulator's device")
        T = int(samples.shape[1])
        for s in range(0, T, MAX_CALL):
            self._call(samples[:, s:s + MAX_CALL], None if truth is None else truth[s:s + MAX_CALL])
        return self

    def _call(self, samples, truth) -> None:
        x, y, _ = datasets(samples, truth)
        args = (x, y, self.n, self.pivot, self.truth_pivot, self.sums, self.invalid)
        if not (_on_device(x) and _launch(*args)):
            _general(*args)
        self.n_times += int(x.shape[1])

    def tables(self) -> CoMomentTables:
        """The state as a copy, shaped ``(..., H, W)``; the accumulator is left alone."""
        H, W = self.H, self.W
        return CoMomentTables(self.n.clone().view(self.D, H, W), self.pivot.clone().view(self.D, self.F, H, W),
                              self.truth_pivot.clone().view(self.D, self.F, H, W) if self.with_truth else None,
                              self.sums.clone().view(self.D, self.NS, H, W), self.invalid.clone(), self.with_truth)

    def merge(self, other: "DependenceAccumulator") -> "DependenceAccumulator":
        """Add ``other``, an accumulator over OTHER hours of the same cells (another rank's time shard): its sums are re-based onto
        this one's pivots in float64 (csrc/comoments_maps.h, MERGE: the formulas, their order and the bound).  A series this one has
        no valid hour of takes the other's state as it is.  ``other`` is left alone."""
        mine, theirs = (self.M, self.F, self.H, self.W, self.with_truth), (other.M, other.F, other.H, other.W, other.with_truth)
        if mine != theirs:
            raise ValueError(f"the other accumulator is (M, F, H, W, with_truth) = {theirs}, this one {mine}")
        if other.device != self.device:
            raise ValueError(f"the other accumulator is on {other.device}, this one on {self.device}")
        F, blk = self.F, _blocks(self.F)
        pf = torch.tensor([p[0] for p in pair_list(F)], dtype=torch.int64, device=self.device)
        pg = torch.tensor([p[1] for p in pair_list(F)], dtype=torch.int64, device=self.device)
        m = other.n.to(torch.float64)[:, None]                                         # (D, 1, hw)
        d = other.pivot.to(torch.float64) - self.pivot.to(torch.float64)               # (D, F, hw)
        So = other.sums[:, blk["S"][0]:blk["S"][1]]
        Co = other.sums[:, blk["C"][0]:blk["C"][1]]
        md = torch.mul(m, d)
        parts = [So + md, ((Co + torch.mul(d[:, pf], So[:, pg])) + torch.mul(d[:, pg], So[:, pf])) + torch.mul(md[:, pf], d[:, pg])]
        if self.with_truth:
            dT = other.truth_pivot.to(torch.float64) - self.truth_pivot.to(torch.float64)
            STo = other.sums[:, blk["ST"][0]:blk["ST"][1]]
            QTo = other.sums[:, blk["QT"][0]:blk["QT"][1]]
            Xo = other.sums[:, blk["X"][0]:blk["X"][1]]
            mdT = torch.mul(m, dT)
            parts += [STo + mdT, ((QTo + torch.mul(dT, STo)) + torch.mul(dT, STo)) + torch.mul(mdT, dT),
                      ((Xo + torch.mul(d, STo)) + torch.mul(dT, So)) + torch.mul(md, dT)]
        take = (self.n == 0)[:, None]
        self.sums = torch.where(take, other.sums, self.sums + torch.cat(parts, dim=1))
        self.pivot = torch.where(take, other.pivot, self.pivot)
        if self.with_truth:
            self.truth_pivot = torch.where(take, other.truth_pivot, self.truth_pivot)
        self.n = self.n + other.n
        self.invalid = self.invalid + other.invalid
        self.n_times += other.n_times
        return self


def comoments(samples: torch.Tensor, truth: Optional[torch.Tensor] = None) -> CoMomentTables:
    """One update plus ``tables()``: ``samples (M, T, F, H, W)``, ``truth (T, F, H, W)`` or None"""
    if samples.dim() != 5:
        raise ValueError(f"samples {tuple(samples.shape)} must be (M, T, F, H, W)")
    M, T, F, H, W = (int(s) for s in samples.shape)
    return DependenceAccumulator(M, F, H, W, with_truth=truth is not None, device=samples.device).update(samples, truth).tables()


# ---------------------------------------------------------------------------------------------------------------------- statistics

def _nf(t: CoMomentTables) -> torch.Tensor:
    return t.n.to(torch.float64)


def _central(t: CoMomentTables) -> torch.Tensor:
    """the central co-moment sums ``C_fg - S_f S_g / n`` as a full matrix ``(D, F, F, H, W)``; NaN where ``n = 0``"""
    F = _variables_of(t)
    S, C = _block(t, "S"), _block(t, "C")
    full = C[:, _pair_matrix(F, C.device).view(-1)].view(C.shape[0], F, F, *C.shape[2:])
    return full - S[:, :, None] * S[:, None, :] / _nf(t)[:, None, None]


def means(t: CoMomentTables) -> torch.Tensor:
    """``(D, F, H, W)`` float64: the temporal mean ``P + S / n`` of every series over its valid hours; NaN where there is none"""
    return t.pivot.to(torch.float64) + _block(t, "S") / _nf(t)[:, None]


def covariance(t: CoMomentTables, ddof: int = 0) -> torch.Tensor:
    """``(D, F, F, H, W)`` float64: ``(C_fg - S_f S_g / n) / (n - ddof)`` per row and cell"""
    return _central(t) / (_nf(t) - float(ddof))[:, None, None]


def _quotient(cross: torch.Tensor, a: torch.Tensor, b: torch.Tensor, enough: torch.Tensor) -> torch.Tensor:
    """``cross / sqrt(a b)``, NaN where a variance is not positive or ``enough`` is false"""
    ok = enough & (a > 0) & (b > 0)
    return torch.where(ok, cross / torch.sqrt(a * b), float("nan"))


def correlation(t: CoMomentTables) -> torch.Tensor:
    """``(D, F, F, H, W)`` float64: Pearson's correlation of the variables of a row over its valid hours, per cell.  NaN where
    ``n < 2`` or a variance is not positive."""
    c = _central(t)
    var = torch.diagonal(c, dim1=1, dim2=2).permute(0, 3, 1, 2)                       # (D, F, H, W)
    return _quotient(c, var[:, :, None], var[:, None, :], (t.n >= 2)[:, None, None])


def _need_truth(t: CoMomentTables, what: str) -> None:
    if not t.with_truth:
        raise ValueError(f"{what} needs tables with a truth")


def _truth_central(t: CoMomentTables):
    """the members' central sums against the truth over each member's own valid hours: ``(own, truth, cross)``, each ``(M, F, H, W)``"""
    F = _variables_of(t)
    n = _nf(t)[1:, None]
    S, ST = _block(t, "S")[1:], _block(t, "ST")[1:]
    diag = torch.tensor([k for k, p in enumerate(pair_list(F)) if p[0] == p[1]], dtype=torch.int64, device=t.sums.device)
    own = _block(t, "C")[1:, diag] - S * S / n
    tru = _block(t, "QT")[1:] - ST * ST / n
    cross = _block(t, "X")[1:] - S * ST / n
    return own, tru, cross


class TruthStatistics(NamedTuple):
    mean_bias: torch.Tensor     # (M, F, H, W) float64
    std_ratio: torch.Tensor
    correlation: torch.Tensor
    centred_rmse: torch.Tensor


def truth_statistics(t: CoMomentTables) -> TruthStatistics:
    """Per member, variable and cell, over the member's own valid hours: ``mean_bias = (P - PT) + (S - ST) / n``, ``std_ratio =
    sigma_m / sigma_t``, Pearson's ``correlation`` with the truth and ``centred_rmse`` with ``centred_rmse^2 = sigma_m^2 + sigma_t^2 -
    2 cov`` clamped at 0 (population moments).  NaN where there is no valid hour; ratio and correlation also where a variance is not
    positive (the correlation where ``n < 2``)."""
    _need_truth(t, "truth_statistics")
    n = _nf(t)[1:, None]
    own, tru, cross = _truth_central(t)
    bias = (t.pivot[1:].to(torch.float64) - t.truth_pivot[1:].to(torch.float64)) + (_block(t, "S")[1:] - _block(t, "ST")[1:]) / n
    ratio = torch.where(tru > 0, torch.sqrt(own / tru), float("nan"))
    corr = _quotient(cross, own, tru, (t.n[1:] >= 2)[:, None])
    vm, vt, cv = own / n, tru / n, cross / n
    return TruthStatistics(bias, ratio, corr, torch.sqrt(((vm + vt) - 2.0 * cv).clamp(min=0.0)))


def _over_cells(a: torch.Tensor, ok: torch.Tensor) -> torch.Tensor:
    return torch.where(ok, a, 0.0).sum(dim=(-1, -2))


def pooled_correlation(t: CoMomentTables) -> torch.Tensor:
    """``(D, F, F)`` float64: the central co-moment sums added over the cells BEFORE the quotient -- the pooled within-cell
    correlation.  A central sum does not depend on the pivot, so the cells need no common one.  Cells without a valid hour do not
    enter; NaN where a pooled variance is not positive."""
    c = _central(t)
    pooled = _over_cells(c, (t.n >= 1)[:, None, None].expand_as(c))
    var = torch.diagonal(pooled, dim1=1, dim2=2)
    return _quotient(pooled, var[:, :, None], var[:, None, :], torch.ones_like(pooled, dtype=torch.bool))


def taylor(t: CoMomentTables) -> torch.Tensor:
    """``(M, F, 3)`` float64: the Taylor-diagram triple of every member and variable, pooled over the cells: standard-deviation
    ratio, correlation with the truth, centred RMSE (``sqrt((sum own + sum truth - 2 sum cross) / sum n)``)"""
    _need_truth(t, "taylor")
    own, tru, cross = _truth_central(t)
    ok = (t.n[1:] >= 1)[:, None].expand_as(own)
    a, b, c = _over_cells(own, ok), _over_cells(tru, ok), _over_cells(cross, ok)
    hours = t.n[1:].to(torch.float64).sum(dim=(-1, -2))[:, None]
    ratio = torch.where(b > 0, torch.sqrt(a / b), float("nan"))
    corr = _quotient(c, a, b, torch.ones_like(a, dtype=torch.bool))
    return torch.stack([ratio, corr, torch.sqrt((((a + b) - 2.0 * c) / hours).clamp(min=0.0))], dim=-1)


def correlation_error(t: CoMomentTables) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(bias, rmse, cells)``: bias and RMSE ``(M, F, F)`` float64 over the cells of ``corr_member - corr_truth`` per pair of
    variables, and the number of cells ``(M, F, F)`` int64 that entered: those where both correlations are numbers"""
    _need_truth(t, "correlation_error")
    corr = correlation(t)
    diff = corr[1:] - corr[:1]
    ok = ~torch.isnan(diff)
    cells = ok.sum(dim=(-1, -2))
    count = cells.to(torch.float64)
    return _over_cells(diff, ok) / count, torch.sqrt(_over_cells(diff * diff, ok) / count), cells


# ---------------------------------------------------------------------------------------------------------------------- the report

class DependenceReport(VariableReport):
    """Per variable, as device tensors, ``M`` members, ``F`` variables (the variable itself included, in their order): ``mean_bias``
    (the mean over the cells of the bias map), ``std_ratio``, ``correlation``, ``centred_rmse`` (the pooled Taylor triple), each
    ``(M,)``; the maps ``mean_bias_map``, ``std_ratio_map``, ``correlation_map``, ``centred_rmse_map (M, H, W)``;
    ``pair_correlation_truth (F,)`` and ``pair_correlation (M, F)``, the pooled correlation with every variable; ``pair_error_bias``,
    ``pair_error_rmse (M, F)`` and ``pair_error_cells (M, F)`` int64, the per-cell correlation's error against the truth's; and
    ``invalid (D,)``, the invalid cell-hours."""

    def as_dict(self, prefix: str = "dependence") -> dict:
        """flat ``{f"{prefix}/{name}/mean_bias": mean over the members, ..."_std": their population std}``, the same for
        ``std_ratio``, ``correlation``, ``centred_rmse`` and, per other variable, ``corr_{other}``, ``corr_{other}_error``; the
        truth's ``corr_{other}_truth`` is one number.  For a logger (one device-to-host copy)."""
        if not self.variables:
            return {}
        rows, keys, single = [], [], []
        for i, (name, v) in enumerate(self):
            for key in ("mean_bias", "std_ratio", "correlation", "centred_rmse"):
                rows.append(v[key])
                keys.append(f"{prefix}/{name}/{key}")
            for j, other in enumerate(self.names):
                if j == i:
                    continue
                rows += [v["pair_correlation"][:, j], v["pair_error_bias"][:, j], v["pair_correlation_truth"][j].expand_as(v["mean_bias"])]
                keys += [f"{prefix}/{name}/corr_{other}", f"{prefix}/{name}/corr_{other}_error", f"{prefix}/{name}/corr_{other}_truth"]
                single.append(keys[-1])
        out = member_mean_std(rows, keys)
        for key in single:
            del out[f"{key}_std"]
        return out


def dependence_report(samples: torch.Tensor, truth: torch.Tensor, names: Optional[Sequence[str]] = None) -> DependenceReport:
    """The dependence of an ensemble ``samples (M, L, F, H, W)`` on ``truth (L, F, H, W)`` and among its variables, per variable.
    ``names``: one per variable, default ``var0 ...``."""
    check_ensemble(samples, truth, time="L", members="M >= 1", floating=True)
    F = int(samples.shape[2])
    names = variable_names(names, F)
    t = comoments(samples, truth)
    stats, tay, pooled = truth_statistics(t), taylor(t), pooled_correlation(t)
    e_bias, e_rmse, e_cells = correlation_error(t)
    variables = []
    for f in range(F):
        variables.append(dict(mean_bias=stats.mean_bias[:, f].nanmean(dim=(-1, -2)), std_ratio=tay[:, f, 0], correlation=tay[:, f, 1],
                              centred_rmse=tay[:, f, 2], mean_bias_map=stats.mean_bias[:, f], std_ratio_map=stats.std_ratio[:, f],
                              correlation_map=stats.correlation[:, f], centred_rmse_map=stats.centred_rmse[:, f],
                              pair_correlation_truth=pooled[0, f], pair_correlation=pooled[1:, f], pair_error_bias=e_bias[:, f],
                              pair_error_rmse=e_rmse[:, f], pair_error_cells=e_cells[:, f], invalid=t.invalid))
    return DependenceReport(names, variables)
