"""Event verification of an ensemble on the device: *was the event forecast?*  Every other score here is an average over the whole
distribution; a storm, a frost, a wind above cut-out or a pressure below 990 hPa is an event, and a downscaler is bought for those.
The reference ships a storm case (exp/configs/000_on-model-eval/s16_t6_storm.yml, exp/figures.py::storm_grid) and only looks at it.

``run_ensemble`` leaves ``(M, T, F, H, W)`` on the device, and here it stays there.  Two HIP kernels (csrc/events.hip) turn the fields
into small **integer tables**; every score is float64 algebra on those tables afterwards.  Integer adds commute, so the tables of the
device equal the definition bit for bit, with no tolerance, wherever a plane lies in the launch.

**The event.**  ``thresholds (F, K)`` are fp32 numbers (a float64 threshold is rounded to fp32 once, here) with a direction per entry:
``"above"`` is ``x >= thr``, ``"below"`` is ``x <= thr``.  Every route compares exact fp32 values with IEEE comparisons: infinities
compare as numbers, a NaN is no event in its own row.  ``thresholds_from_quantiles`` gives climatological thresholds (the 95th and
99th percentile of the truth per variable, say); a derived field such as the hub-height speed of ``windpower.wind_fields`` is passed as
a variable.

**The tables** (include/c2w_hip.h: c2w_event_counts, c2w_fss_sums).

* ``counts[t, f, k, o, j]``, int64 ``(T, F, K, 2, M + 1)``: the cells of plane ``(t, f)`` whose truth indicator is ``o`` and in which
  exactly ``j`` of the ``M`` members have the event.  ``invalid[t, f]`` counts the cells with a NaN among their ``M + 1`` values; they
  are in no bin.
* ``sums[t, f, k, s, d, 0..1] = (sum_c n_d(c)^2, sum_c n_d(c) n_0(c))``, int64 ``(T, F, K, S, M + 2, 2)``: the rows are ``d = 0`` the
  truth, ``1 .. M`` the members and ``M + 1`` the ensemble, whose cell value is the member count; ``n_d(c)`` is the sum of row ``d`` over
  the ``(2r + 1)^2`` window centred on ``c``, cells outside the domain counting 0 (zero padding), ``r = radii[s]``.

**The scores.**  With ``N = counts`` (any leading shape; sum over time first for a pooled score), ``p_j = j / M`` and ``n = sum N``:

* Brier score ``sum N[o][j] (p_j - o)^2 / n``; the fair form subtracts ``j (M - j) / (M^2 (M - 1))`` per cell (Ferro's correction for
  the finite ensemble, recalled; NaN at ``M = 1``)
* its decomposition with the ``M + 1`` attainable probabilities as the bins, so that ``BS = REL - RES + UNC`` holds exactly; the skill
  score ``1 - BS / UNC``; the reliability curve
* the ROC: hit rate and false-alarm rate of "at least ``j`` members", ``j = 0 .. M + 1``, and the trapezoid area over those points
* the fractions skill score of Roberts & Lean (2008, recalled) ``2 PO / (PP + OO)``, per member and for the ensemble probability
  (``PP / M^2``, ``PO / M``), per time or pooled by summing the three integers first; the smallest useful radius; and the contingency
  table of every member from the radius-0 entries.

On the GPU the counts kernel takes ``H W`` a multiple of 4, ``M <= 64`` and ``K <= 8``; the FSS kernel ``W`` a multiple of 4,
``H, W >= 4``, ``H W <= 2^20``, ``M <= 64``, ``K <= 8`` and at most 8 radii in ``0 .. 16``.  Everything else and CPU tensors take the
same integers from torch, chunked over time.  Nothing here synchronises.

Out of scope: events joint over variables, neighbourhoods other than the box, extreme-value fits, collectives -- members are
rank-local -- and the plotting.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import torch

from . import event_ops
from .ensemble_host import VariableReport, check_ensemble, chunk_step, datasets, member_mean_std, variable_names
from .ensemble_host import on_device as _on_device
from .quantiles import quantile

NAN = float("nan")
MAX_RADIUS_GENERAL = 1 << 20  # any radius the window arithmetic of the general route can hold


# ---------------------------------------------------------------------------------------------------------------------- the event

def thresholds_from_quantiles(truth: torch.Tensor, levels: Sequence[float] = (0.95, 0.99)) -> torch.Tensor:
    """``(F, K)`` fp32: the quantiles of ``truth (T, F, H, W)`` at ``levels`` per variable over all times and cells
    (``quantiles.quantile``), rounded to fp32 -- climatological thresholds"""
    if truth.dim() != 4:
        raise ValueError(f"truth {tuple(truth.shape)} must be (T, F, H, W)")
    return quantile(truth, list(levels)).to(torch.float32)


def _event_spec(thresholds, direction, F: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """thr (F, K) fp32 and dir (F, K) int32 (1 above, 0 below) on ``device``"""
    thr = torch.as_tensor(thresholds)
    if thr.dim() != 2 or int(thr.shape[0]) != F or int(thr.shape[1]) < 1:
        raise ValueError(f"thresholds {tuple(thr.shape)} must be (F, K) = ({F}, K >= 1)")
    if not (thr.is_floating_point() or thr.dtype in (torch.int32, torch.int64)):
        raise ValueError(f"thresholds ({thr.dtype}) must be numbers")
    K = int(thr.shape[1])
    thr = thr.to(device=device, dtype=torch.float32).contiguous()  # a float64 threshold is rounded once, here
    if isinstance(direction, str):
        rows = [[direction] * K] * F
    else:
        rows = [list(r) if not isinstance(r, str) else r for r in direction]
        if len(rows) == K and all(isinstance(r, str) for r in rows):
            rows = [rows] * F  # one direction per threshold, the same for every variable
        if len(rows) != F or any(isinstance(r, str) or len(r) != K for r in rows):
            raise ValueError(f"direction must be 'above', 'below', K = {K} of them or (F, K) = ({F}, {K}) of them")
    flat = [d for r in rows for d in r]
    if any(d not in ("above", "below") for d in flat):
        raise ValueError(f"direction {sorted(set(map(str, flat)))} must be 'above' or 'below'")
    dirn = torch.tensor([1 if d == "above" else 0 for d in flat], dtype=torch.int32).view(F, K).to(device)
    return thr, dirn


def _indicator(v: torch.Tensor, thr: torch.Tensor, dirn: torch.Tensor) -> torch.Tensor:
    """v (..., F, 1, cells...) against thr, dirn (F, K, 1...): bool (..., F, K, cells...)"""
    return torch.where(dirn != 0, v >= thr, v <= thr)


def _inputs(samples, truth, thresholds, direction):
    check_ensemble(samples, truth, members="M >= 1", floating=True)
    x, y, _ = datasets(samples, truth)
    F = int(x.shape[2])
    thr, dirn = _event_spec(thresholds, direction, F, x.device)
    return x, y, thr, dirn


# ---------------------------------------------------------------------------------------------------------------------- the joint table

def _general_counts(x, y, thr, dirn, counts, invalid) -> None:
    """The definition for any shape and any device: x (M, T, F, hw), y (T, F, hw), counts (T, F, K, 2, M + 1), invalid (T, F)"""
    M, T, F, hw = (int(s) for s in x.shape)
    K = int(thr.shape[1])
    counts.zero_()
    nb = 2 * (M + 1)
    step = chunk_step((M + 1) * F * K * hw)
    th, dr = thr[:, :, None], dirn[:, :, None]
    for t0 in range(0, T, step):
        xs, ys = x[:, t0:t0 + step], y[t0:t0 + step]
        n = int(ys.shape[0])
        nan = torch.isnan(ys) | torch.isnan(xs).any(dim=0)                       # (n, F, hw)
        j = _indicator(xs[:, :, :, None, :], th, dr).sum(dim=0)                  # (n, F, K, hw) int64
        o = _indicator(ys[:, :, None, :], th, dr).to(torch.int64)
        plane = torch.arange(n * F * K, device=x.device).view(n, F, K, 1)
        idx = plane * nb + o * (M + 1) + j
        valid = (~nan)[:, :, None, :].expand(n, F, K, hw).to(torch.int64)
        counts[t0:t0 + n].view(-1).scatter_add_(0, idx.reshape(-1), valid.reshape(-1))
        invalid[t0:t0 + n] = nan.sum(dim=-1)


def _launch_counts(x, y, thr, dirn, counts, invalid, M, T, F, hw, K) -> bool:
    if not event_ops.counts_supported(hw, M, K):
        return False
    return event_ops.event_counts(x, y, thr, dirn, counts, invalid, M, T, F, hw, K)


def event_counts(samples: torch.Tensor, truth: torch.Tensor, thresholds, direction="above") -> Tuple[torch.Tensor, torch.Tensor]:
    """``samples (M, T, F, H, W)``, ``truth (T, F, H, W)``, ``thresholds (F, K)`` -> ``(counts (T, F, K, 2, M + 1), invalid (T, F))``
    int64 on the same device: per plane and threshold the cells by truth indicator ``o`` and number ``j`` of members with the event, and
    the cells with a NaN among their ``M + 1`` values, which are in no bin (module docstring).  ``direction``: ``"above"`` (``x >= thr``),
    ``"below"`` (``x <= thr``), one per threshold or ``(F, K)`` of them.  Any float dtype and any strides: a strided or 16-bit input costs
    one dense fp32 copy.

    On the GPU ``H W`` a multiple of 4, ``M <= 64`` and ``K <= 8`` take the kernel; everything else and CPU tensors take the same
    integers from torch."""
    x, y, thr, dirn = _inputs(samples, truth, thresholds, direction)
    M, T, F, hw = (int(s) for s in x.shape)
    K = int(thr.shape[1])
    counts = torch.empty((T, F, K, 2, M + 1), dtype=torch.int64, device=x.device)
    invalid = torch.empty((T, F), dtype=torch.int64, device=x.device)
    if counts.numel() == 0:
        return counts, invalid
    if hw == 0:
        return counts.zero_(), invalid.zero_()
    if not (_on_device(x) and _launch_counts(x, y, thr, dirn, counts, invalid, M, T, F, hw, K)):
        _general_counts(x, y, thr, dirn, counts, invalid)
    return counts, invalid


# ---------------------------------------------------------------------------------------------------------------------- the FSS sums

def _check_radii(radii) -> list:
    rr = [int(r) for r in radii]
    if not rr or any(r < 0 or r > MAX_RADIUS_GENERAL for r in rr) or any(int(r) != r for r in radii):
        raise ValueError(f"radii {list(radii)} must be at least one integer >= 0")
    return rr


def _general_fss(x, y, thr, dirn, sums, radii, H, W) -> None:
    """The definition for any shape and any device: the int64 summed-area table of every row, padded with a zero row and column, and
    corner differences clipped to the domain.  x (M, T, F, hw), y (T, F, hw), sums (T, F, K, S, M + 2, 2)"""
    M, T, F, hw = (int(s) for s in x.shape)
    K = int(thr.shape[1])
    th, dr = thr[:, :, None, None], dirn[:, :, None, None]
    step = chunk_step((M + 2) * F * K * hw * 2)
    ar_h, ar_w = torch.arange(H, device=x.device), torch.arange(W, device=x.device)
    for t0 in range(0, T, step):
        xs, ys = x[:, t0:t0 + step].view(M, -1, F, 1, H, W), y[t0:t0 + step].view(-1, F, 1, H, W)
        e = _indicator(xs, th, dr).to(torch.int64)                               # (M, n, F, K, H, W)
        rows = torch.cat([_indicator(ys, th, dr).to(torch.int64)[None], e, e.sum(dim=0, keepdim=True)])
        table = torch.nn.functional.pad(rows.cumsum(dim=-1).cumsum(dim=-2), (1, 0, 1, 0))
        for s, r in enumerate(radii):
            a0, a1 = (ar_h - r).clamp(min=0)[:, None], (ar_h + r + 1).clamp(max=H)[:, None]
            b0, b1 = (ar_w - r).clamp(min=0)[None, :], (ar_w + r + 1).clamp(max=W)[None, :]
            n = table[..., a1, b1] - table[..., a0, b1] - table[..., a1, b0] + table[..., a0, b0]   # (M + 2, n, F, K, H, W)
            sums[t0:t0 + step, :, :, s, :, 0] = (n * n).sum(dim=(-1, -2)).permute(1, 2, 3, 0)
            sums[t0:t0 + step, :, :, s, :, 1] = (n * n[:1]).sum(dim=(-1, -2)).permute(1, 2, 3, 0)


def _launch_fss(x, y, thr, dirn, sums, radii, M, T, F, H, W, K) -> bool:
    if not event_ops.fss_supported(H, W, M, K, radii):
        return False
    return event_ops.fss_sums(x, y, thr, dirn, sums, radii, M, T, F, H, W, K)


def fss_sums(samples: torch.Tensor, truth: torch.Tensor, thresholds, radii: Sequence[int] = (0, 1, 2, 4, 8), direction="above") -> torch.Tensor:
    """``sums (T, F, K, S, M + 2, 2)`` int64 on the same device: per plane, threshold, radius and row -- 0 the truth, ``1 .. M`` the
    members, ``M + 1`` the ensemble's member count -- ``(sum_c n_d(c)^2, sum_c n_d(c) n_0(c))`` with ``n_d(c)`` the row's sum over the
    zero-padded ``(2r + 1)^2`` window centred on ``c`` (module docstring).  Row 0 holds ``(OO, OO)``.

    On the GPU ``W`` a multiple of 4, ``H, W >= 4``, ``H W <= 2^20``, ``M <= 64``, ``K <= 8`` and at most 8 radii in ``0 .. 16`` take the
    kernel; everything else and CPU tensors take the same integers from torch."""
    rr = _check_radii(radii)
    x, y, thr, dirn = _inputs(samples, truth, thresholds, direction)
    M, T, F, hw = (int(s) for s in x.shape)
    H, W = int(samples.shape[-2]), int(samples.shape[-1])
    K = int(thr.shape[1])
    sums = torch.empty((T, F, K, len(rr), M + 2, 2), dtype=torch.int64, device=x.device)
    if sums.numel() == 0:
        return sums
    if hw == 0:
        return sums.zero_()
    if not (_on_device(x) and _launch_fss(x, y, thr, dirn, sums, rr, M, T, F, H, W, K)):
        _general_fss(x, y, thr, dirn, sums, rr, H, W)
    return sums


# ---------------------------------------------------------------------------------------------------------------------- the algebra

def _table(counts: torch.Tensor) -> Tuple[torch.Tensor, int, torch.Tensor, torch.Tensor]:
    """N (..., 2, M + 1) float64, M, p (M + 1,), o (2, 1)"""
    if counts.dim() < 2 or int(counts.shape[-2]) != 2 or int(counts.shape[-1]) < 2:
        raise ValueError(f"counts {tuple(counts.shape)} must be (..., 2, M + 1)")
    M = int(counts.shape[-1]) - 1
    p = torch.arange(M + 1, dtype=torch.float64, device=counts.device) / M
    o = torch.tensor([[0.0], [1.0]], dtype=torch.float64, device=counts.device)
    return counts.to(torch.float64), M, p, o


def brier_score(counts: torch.Tensor, fair: bool = False) -> torch.Tensor:
    """``counts (..., 2, M + 1)`` -> ``(...)`` float64: ``sum N[o][j] (j / M - o)^2 / n``.  ``fair``: less ``j (M - j) / (M^2 (M - 1))``
    per cell, the score an infinite ensemble of the same distribution would get in expectation; NaN at ``M = 1``.  NaN without a cell."""
    N, M, p, o = _table(counts)
    n = N.sum(dim=(-1, -2))
    bs = (N * (p - o) ** 2).sum(dim=(-1, -2)) / n
    if not fair:
        return bs
    if M == 1:
        return torch.full_like(bs, NAN)
    j = p * M
    return bs - (N * (j * (M - j) / (M * M * (M - 1)))).sum(dim=(-1, -2)) / n


def brier_decomposition(counts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(reliability, resolution, uncertainty)``, each ``(...)`` float64, with the ``M + 1`` attainable probabilities as the bins:
    ``REL = sum_j n_j (p_j - obar_j)^2 / n``, ``RES = sum_j n_j (obar_j - obar)^2 / n``, ``UNC = obar (1 - obar)``; an empty bin adds
    nothing.  ``BS = REL - RES + UNC`` holds exactly, since every cell of a bin has the bin's probability."""
    N, M, p, _ = _table(counts)
    nj = N.sum(dim=-2)                                                   # (..., M + 1)
    n = nj.sum(dim=-1)
    base = N[..., 1, :].sum(dim=-1) / n
    obar = torch.where(nj > 0, N[..., 1, :] / nj.clamp(min=1.0), torch.zeros_like(nj))
    rel = (nj * (p - obar) ** 2).sum(dim=-1) / n
    res = (nj * (obar - base[..., None]) ** 2).sum(dim=-1) / n
    return rel, res, base * (1.0 - base)


def brier_skill_score(counts: torch.Tensor) -> torch.Tensor:
    """``1 - BS / UNC`` against the truth's base rate; NaN where the truth has no event or only events"""
    bs = brier_score(counts)
    unc = brier_decomposition(counts)[2]
    return torch.where(unc > 0, 1.0 - bs / torch.where(unc > 0, unc, torch.ones_like(unc)), torch.full_like(bs, NAN))


def reliability_curve(counts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(probability (M + 1,), observed frequency (..., M + 1), count (..., M + 1))``: per bin ``j`` the forecast probability ``j / M``,
    the fraction of its cells in which the truth has the event (NaN for an empty bin), and its cells"""
    N, _, p, _ = _table(counts)
    nj = N.sum(dim=-2)
    return p, N[..., 1, :] / nj, counts.sum(dim=-2)


def roc_curve(counts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(hit rate, false-alarm rate)``, each ``(..., M + 2)`` float64, of the forecast "at least ``j`` members have the event",
    ``j = 0 .. M + 1``: from ``(1, 1)`` down to ``(0, 0)``.  NaN where the truth has no event (hit rate) or only events (false alarms)."""
    N, _, _, _ = _table(counts)
    tail = N.flip(-1).cumsum(dim=-1).flip(-1)                            # sum_{i >= j}
    tail = torch.cat([tail, torch.zeros_like(tail[..., :1])], dim=-1)    # j = M + 1
    rate = tail / tail[..., :1]
    return rate[..., 1, :], rate[..., 0, :]


def roc_area(counts: torch.Tensor) -> torch.Tensor:
    """the trapezoid area under the ``M + 2`` points of ``roc_curve``"""
    hit, fa = roc_curve(counts)
    return ((fa[..., :-1] - fa[..., 1:]) * (hit[..., :-1] + hit[..., 1:]) * 0.5).sum(dim=-1)


def _sums(sums: torch.Tensor) -> Tuple[torch.Tensor, int]:
    if sums.dim() != 6 or int(sums.shape[-1]) != 2 or int(sums.shape[-2]) < 3:
        raise ValueError(f"sums {tuple(sums.shape)} must be (T, F, K, S, M + 2, 2)")
    return sums, int(sums.shape[-2]) - 2


def fss(sums: torch.Tensor, pooled: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """``sums (T, F, K, S, M + 2, 2)`` -> ``(per member (T, F, K, S, M), ensemble (T, F, K, S))`` float64: ``2 PO / (PP + OO)``, for the
    ensemble probability with ``PP / M^2`` and ``PO / M``.  ``pooled``: the three integers are summed over time first and the time
    axis is gone.  NaN where ``PP + OO = 0``: neither field has an event within reach."""
    sums, M = _sums(sums)
    if pooled:
        sums = sums.sum(dim=0)
    s = sums.to(torch.float64)
    oo = s[..., 0, 0]
    pp, po = s[..., 1:M + 1, 0], s[..., 1:M + 1, 1]
    member = 2.0 * po / (pp + oo[..., None])
    ens = 2.0 * (s[..., M + 1, 1] / M) / (s[..., M + 1, 0] / (M * M) + oo)
    return member, ens


def _radius_zero(radii: Sequence[int]) -> int:
    rr = [int(r) for r in radii]
    if 0 not in rr:
        raise ValueError(f"radii {rr} must contain 0")
    return rr.index(0)


def fss_useful_scale(sums: torch.Tensor, radii: Sequence[int], cells: int) -> torch.Tensor:
    """``(F, K)`` int64: the smallest radius at which the pooled FSS of the ensemble probability reaches ``0.5 + f0 / 2``, ``f0`` the
    truth's base rate -- the radius-0 ``OO`` over ``T cells``, ``cells = H W``; -1 where none of ``radii`` reaches it"""
    sums, _ = _sums(sums)
    rr = [int(r) for r in radii]
    if len(rr) != int(sums.shape[3]):
        raise ValueError(f"{len(rr)} radii for sums {tuple(sums.shape)} with S = {int(sums.shape[3])}")
    zero = _radius_zero(rr)
    T = int(sums.shape[0])
    f0 = sums[:, :, :, zero, 0, 0].sum(dim=0).to(torch.float64) / (T * int(cells))
    ens = fss(sums, pooled=True)[1]                                      # (F, K, S)
    big = max(rr) + 1
    r = torch.tensor(rr, dtype=torch.int64, device=sums.device)
    best = torch.where(ens >= (0.5 + f0 / 2.0)[..., None], r, torch.full_like(r, big)).min(dim=-1).values
    return torch.where(best == big, torch.full_like(best, -1), best)


def member_contingency(sums: torch.Tensor, radii: Sequence[int], cells: int) -> dict:
    """The contingency table of every member from the radius-0 entries, where a window is the cell itself: ``PP_m`` = forecast yes,
    ``PO_m`` = hits, ``OO`` = observed yes.  ``cells``: the cells an entry covers (``H W``; ``T H W`` for sums summed over time with the
    axis kept).  A dict of ``(T, F, K, M)`` tensors: ``hits``, ``false_alarms``, ``misses``, ``correct_negatives`` (int64),
    ``frequency_bias = forecast yes / observed yes`` and ``csi = hits / (hits + false alarms + misses)`` (float64, NaN at 0 / 0).
    ``radii`` must contain 0."""
    sums, M = _sums(sums)
    zero = _radius_zero(radii)
    at = sums[:, :, :, zero]
    oo = at[..., 0, 0][..., None]
    pp, hits = at[..., 1:M + 1, 0], at[..., 1:M + 1, 1]
    fa, miss = pp - hits, oo - hits
    d = lambda t: t.to(torch.float64)
    return dict(hits=hits, false_alarms=fa, misses=miss, correct_negatives=int(cells) - hits - fa - miss,
                frequency_bias=d(pp) / d(oo), csi=d(hits) / d(hits + fa + miss))


# ---------------------------------------------------------------------------------------------------------------------- the report

class EventsReport(VariableReport):
    """Per variable, as device tensors pooled over time, ``K`` thresholds, ``S`` radii: ``thresholds (K,)``, ``base_rate``, ``brier``,
    ``brier_fair``, ``reliability``, ``resolution``, ``uncertainty``, ``brier_skill``, ``roc_area (K,)``, ``reliability_probability
    (M + 1,)``, ``reliability_frequency``, ``reliability_count (K, M + 1)``, ``hit_rate``, ``false_alarm_rate (K, M + 2)``,
    ``fss (K, S)`` of the ensemble probability, ``fss_member (K, S, M)``, ``fss_time (T, K, S)``, ``fss_useful_scale (K,)``, the
    members' ``hits``, ``false_alarms``, ``misses``, ``correct_negatives``, ``frequency_bias``, ``csi (K, M)`` where ``radii`` contains
    0, and ``invalid``, the cells left out for a NaN."""

    def __init__(self, names, variables, radii):
        super().__init__(names, variables)
        self.radii = list(radii)

    def as_dict(self, prefix: str = "events") -> dict:
        """flat ``{f"{prefix}/{name}/fss_k{k}_r{r}": mean over the members, ..."_std": their population std}`` for a logger (one
        device-to-host copy)"""
        if not self.variables:
            return {}
        rows, keys = [], []
        for name, v in self:
            for k in range(int(v["fss_member"].shape[0])):
                for s, r in enumerate(self.radii):
                    rows.append(v["fss_member"][k, s])
                    keys.append(f"{prefix}/{name}/fss_k{k}_r{r}")
        return member_mean_std(rows, keys)


def events_report(samples: torch.Tensor, truth: torch.Tensor, thresholds=None, levels: Sequence[float] = (0.95, 0.99),
                  radii: Sequence[int] = (0, 1, 2, 4, 8), names: Optional[Sequence[str]] = None,
                  direction: Union[str, Sequence] = "above") -> EventsReport:
    """The event scores of an ensemble ``samples (M, L, F, H, W)`` against ``truth (L, F, H, W)`` per variable, from one pass of each
    kernel over the fields.  ``thresholds (F, K)``, or None for the truth's quantiles at ``levels``.  ``names``: one per variable,
    default ``var0 ...``."""
    check_ensemble(samples, truth, time="L", members="M >= 1", floating=True)
    F, cells = int(samples.shape[2]), int(samples.shape[-2]) * int(samples.shape[-1])
    names = variable_names(names, F)
    rr = _check_radii(radii)
    thr = thresholds_from_quantiles(truth, levels) if thresholds is None else thresholds
    thr, _ = _event_spec(thr, direction, F, samples.device)
    counts, invalid = event_counts(samples, truth, thr, direction)
    sums = fss_sums(samples, truth, thr, rr, direction)
    T = int(counts.shape[0])
    C = counts.sum(dim=0)                                                # (F, K, 2, M + 1)
    rel, res, unc = brier_decomposition(C)
    prob, freq, cnt = reliability_curve(C)
    hit, fa = roc_curve(C)
    member, ens = fss(sums, pooled=True)
    per_time = fss(sums)[1]                                              # (T, F, K, S)
    table = member_contingency(sums.sum(dim=0, keepdim=True), rr, T * cells) if 0 in rr else {}
    useful = fss_useful_scale(sums, rr, cells) if 0 in rr else None
    Cd = C.to(torch.float64)
    base = Cd[..., 1, :].sum(dim=-1) / Cd.sum(dim=(-1, -2))
    bs, fair, bss, area = brier_score(C), brier_score(C, fair=True), brier_skill_score(C), roc_area(C)
    variables = []
    for f in range(F):
        v = dict(thresholds=thr[f], base_rate=base[f], brier=bs[f], brier_fair=fair[f], reliability=rel[f], resolution=res[f],
                 uncertainty=unc[f], brier_skill=bss[f], roc_area=area[f], reliability_probability=prob, reliability_frequency=freq[f],
                 reliability_count=cnt[f], hit_rate=hit[f], false_alarm_rate=fa[f], fss=ens[f], fss_member=member[f],
                 fss_time=per_time[:, f], invalid=invalid[:, f].sum())
        if useful is not None:
            v["fss_useful_scale"] = useful[f]
        for key, t in table.items():
            v[key] = t[0, f]
        variables.append(v)
    return EventsReport(names, variables, rr)
